"""Child-process case runner for the kernels that only a runtime switch selects (docs/SWITCHES.md).

    python tests/fallback_cases.py CASE      every shape of one case on the GPU, one JSON line per shape
    python tests/fallback_cases.py --list    the case table (no GPU, no native library)

Most native switches are read ONCE per process and have no setter, so the in-process kernel tests only ever see the
default side.  tests/test_fallback_paths_gpu.py starts this file once per case, in a fresh process whose environment carries the
case's switches.  Each JSON line holds the shape, the errors per output (against the float64 CPU reference, or against the path
the mirrored test compares with) and, for every switch the case sets, what mmnas_switch_info reports AFTER the kernels ran:
a switch that was never consulted still carries the 'unread' flag there.  The process exits 0 when it ran to the end, whatever
the errors: the parent judges them against BOUNDS.  Importable without a GPU (tests/test_switches_host.py reads CASES)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# attention shapes: (B, H, Sq, Sk, mask, bias, p), d_h = 64; with a mask the last sample is fully padded.
# ('packed', B, H, Sq_max, Sk_max, bias, p): q_off + k_off, checked sequence by sequence.
_MHA_MID = [(2, 4, 100, 100, True, True, 0.1), (3, 1, 128, 65, True, True, 0.0), (2, 2, 1, 96, False, False, 0.0),
            (2, 4, 97, 128, True, False, 0.3), (2, 2, 36, 100, True, False, 0.1), (2, 3, 33, 97, True, True, 0.0),
            ('packed', 5, 4, 100, 100, True, 0.1)]
_MHA_UNFUSED = [(2, 4, 100, 100, True, True, 0.1), (2, 8, 100, 14, True, False, 0.1), (3, 4, 14, 14, True, False, 0.0),
                (2, 2, 36, 50, True, False, 0.0), (2, 4, 97, 128, True, False, 0.3), (2, 2, 20, 100, False, True, 0.0)]
_MANY_QUERIES = lambda shapes: [s for s in shapes if s[0] != 'packed' and s[2] > 64]
# relation shapes: ('dense', B, Sq, Sk, C, H) / ('ragged', B, S, C, H, lens): the H <= 4 rows of test_rel_fused_lazy_handle and
# test_rel_fused_ragged (tests/test_kernels_gpu.py), and one dense H = 1 problem (no row of those tests has one head)
_REL_FUSED = [('dense', 2, 7, 7, 4, 2), ('dense', 3, 5, 9, 3, 4), ('dense', 3, 5, 5, 4, 1),
              ('ragged', 4, 100, 4, 4, (100, 37, 10, 1)), ('ragged', 5, 14, 3, 4, (14, 3, 7, 1, 9))]
# (B, S, C, H, n_ops, lens): the smallest dense and the smallest ragged row of test_rel_multi_all_relation_operators_in_one_launch
_REL_MULTI = [(2, 7, 4, 2, 3, None), (4, 23, 4, 4, 9, (23, 1, 7, 16))]
# architecture step, mixed chain against the per-candidate path: (seed, HSIZE, B, Sx, Sy, mode, dropout).  The first row is
# the configuration of test_arch_step_through_the_mixed_chain_equals_the_per_candidate_path (tests/test_harness_gpu.py).
_ARCH_SMALL = [(4242, 128, 3, 5, 7, 'full', 0.0), (4242, 128, 3, 5, 7, 'full', 0.1), (4242, 128, 3, 5, 7, 'two', 0.1)]
# HSIZE 512: wider than the 256 columns the node's mix kernel carries a LayerNorm backward for -- its own launch by that rule
_ARCH_WIDE = [(4242, 512, 3, 5, 7, 'full', 0.1)]
# weight step, chain (with its side stream) against the per-operator path: (task, plan seed, B, Sx, Sy, dropout) -- the vqa case of
# test_chain_equals_per_operator_path_supernet_weight_step (tests/test_chain_gpu.py)
_WEIGHT = [('vqa', 1, 3, 6, 9, 0.1), ('vqa', 2, 3, 6, 9, 0.1)]
# MMNAS_MHA_PAIR is consulted by the mixed chain's forward only, and decides something only where two attention candidates of a
# node share a geometry with more than 64 queries and 65..128 keys: an architecture step ('full': every candidate) at 100 regions
_ARCH_PAIR = [(4242, 128, 2, 5, 100, 'full', 0.1)]
# HSIZE 256: the smallest width the short-sequence kernels take (sa_small_applies: d in {256, 512}, <= 16 rows, heads of 64);
# _ARCH_SMALL's 128 never reaches them
_ARCH_SHORT = [(4242, 256, 3, 5, 7, 'full', 0.1), (4242, 256, 3, 5, 7, 'two', 0.1)]

CASES = {
    'mha_fp32_mid': dict(env={'MMNAS_MHA_FWD_B16': '0', 'MMNAS_MHA_BWD_B16': '0'}, kind='mha', shapes=_MHA_MID),
    'mha_fp32_mid_nw2': dict(env={'MMNAS_MHA_FWD_B16': '0', 'MMNAS_MHA_BWD_B16': '0', 'MMNAS_MHA_NW': '2'}, kind='mha',
                             shapes=_MANY_QUERIES(_MHA_MID)),
    # the fp32 mha_fwd_pair_kernel<64,4,4>: two attention candidates of one geometry in the mixed chain's forward, bf16 forward off
    'mha_fp32_pair': dict(env={'MMNAS_MHA_FWD_B16': '0', 'MMNAS_MHA_BWD_B16': '0'}, kind='arch', shapes=_ARCH_PAIR),
    'mha_unfused': dict(env={'MMNAS_MHA_BWD_FUSED': '0'}, kind='mha', shapes=_MHA_UNFUSED),
    'mha_unfused_nw2': dict(env={'MMNAS_MHA_BWD_FUSED': '0', 'MMNAS_MHA_NW': '2'}, kind='mha', shapes=_MANY_QUERIES(_MHA_UNFUSED)),
    'mha_b16_two': dict(env={'MMNAS_MHA_FWD_B16_TWO': '0'}, kind='mha',
                        shapes=[(2, 4, 100, 100, True, True, 0.1), (3, 1, 128, 65, True, True, 0.0), (1, 1, 1, 96, False, False, 0.0)]),
    'rel_bwd_mfma': dict(env={'MMNAS_REL_BWD_VALU': '0'}, kind='rel_fused', shapes=_REL_FUSED),
    'rel_multi_yield1': dict(env={'MMNAS_REL_MULTI_YIELD': '1'}, kind='rel_multi', shapes=_REL_MULTI),
    'rel_multi_yield3': dict(env={'MMNAS_REL_MULTI_YIELD': '3'}, kind='rel_multi', shapes=_REL_MULTI),
    'rel_multi_wgs1': dict(env={'MMNAS_REL_MULTI_WGS': '1'}, kind='rel_multi', shapes=_REL_MULTI),
    'chain_node_lnb0': dict(env={'MMNAS_NODE_LNB': '0'}, kind='arch', shapes=_ARCH_SMALL + _ARCH_WIDE),
    # a sampled language-stream SelfAtt through the one-launch forward and then the GENERAL backward, inside the mixed chain
    'chain_small_bwd0': dict(env={'MMNAS_SMALL_BWD': '0'}, kind='arch', shapes=_ARCH_SHORT),
    'chain_misc': dict(env={'MMNAS_MHA_PAIR': '0', 'MMNAS_HEAD_OVERLAP': '1', 'MMNAS_SIDE_FLUSH': 'op', 'MMNAS_SIDE_PRIO': '0'},
                       kind='chain_misc', shapes=_WEIGHT + _ARCH_PAIR),
}

# The kernels each case reaches that the default setting does not, read from the dispatch code (launch_fwd / launch_bwd,
# mmnas_mha_core_fwd / _bwd and mha_core_fwd_pair in attention.hip; mha_fwd_b16_launch in attention_bwd16.hip; rf_bwd_impl in
# relfused.hip; mmnas_rel_multi_fwd / _bwd in relmulti.hip; att_ln_place, chain_cand_view, chain_bwd_mixed, mmnas_chain_bwd, side_ctx and the head
# in ops.hip).
REACHES = {
    'mha_fp32_mid': 'mha_fwd_kernel<64,4,1> (1 query), <64,4,2> (33, 36 queries), <64,4,4> (97, 100, 128 queries; packed rows); '
                    'mha_bwd_fused_kernel<4,true|false> (dense and packed rows)',
    'mha_fp32_mid_nw2': 'mha_fwd_kernel<64,4,2> at more than 64 queries; the backward is mha_bwd_fused_kernel<4,*> as above',
    'mha_fp32_pair': 'mha_fwd_pair_kernel<64,4,4> (self + relation-self candidate of a decoder node, 100 regions); mha_bwd_fused_kernel<4,*>',
    'mha_unfused': 'mha_bwd_q_kernel<64,1,1> (14x14), <64,1,4> (100x14), <64,2,1> (20x100), <64,2,2> (36x50), <64,2,4> (100x100, 97x128); '
                   'mha_bwd_kv_kernel<64,1,1> (14x14), <64,1,4> (100x14), <64,2,1> (36x50), <64,4,1> (100, 128 keys)',
    'mha_unfused_nw2': 'mha_bwd_q_kernel<64,1,2>, <64,2,2> and mha_bwd_kv_kernel<64,2,1> at more than 64 queries',
    'mha_b16_two': 'mha_fwd_b16_two_kernel with one problem per launch (grid H x B, nh0 = H)',
    'rel_bwd_mfma': 'rel_fused_bwd_kernel<4,1> and <3,1> at 1, 2 and 4 heads, dense and ragged',
    'rel_multi_yield1': 'rel_multi_fwd_kernel<4,1,1>, <4,2,1>; rel_multi_bwd_kernel<4,1>',
    'rel_multi_yield3': 'rel_multi_fwd_kernel<4,1,3>, <4,2,3>; rel_multi_bwd_kernel<4,3>',
    'rel_multi_wgs1': 'the default instantiations on the grid of one workgroup per CU (forward)',
    'chain_node_lnb0': "node_mix_bwd without its LayerNorm part, then the candidate's LayerNorm backward as its own launch inside "
                       'att_bwd_impl / mlp_bwd_impl; at HSIZE 512 that is the route with the switch on or off',
    'chain_small_bwd0': "sa_small_fwd for the sampled encoder SelfAtt (it normalises its own output: the node epilogue gets no LayerNorm for "
                        "it), then node_mix_bwd without a LayerNorm part for that node and att_bwd_impl's general path from its own "
                        'LayerNorm backward on (att_ln_place: forward yes, backward no)',
    'chain_misc': 'two mha_fwd_b16_kernel launches where the pair launch would run (arch step); the head with its two AttFlat sides '
                  'on two streams; side-stream parameter-gradient work flushed behind every operator; stream pairs without priorities',
}

# What the parent holds every error to: the bounds of the default-path tests the cases borrow their shapes from.
#   mha        test_mha_core / test_mha_core_packed_rows: 1e-5 on the output, 1e-4 on dQ / dK / dV / dbias
#   rel_fused  test_rel_fused_lazy_handle: 1e-3 (tests/util.py TOL; every dense shape here has B Sq Sk < 5000);
#              test_rel_fused_ragged: forward bitwise the dense call inside the corners and nothing written outside ('exact'
#              errors are 0 or 1), backward within 2e-4 of the dense call
#   rel_multi  test_rel_multi_all_relation_operators_in_one_launch: max(r, 1e-6) within 2e-5, gradients within 1e-4 of float64
#              and within 3e-4 of the per-operator kernels
#   arch       test_arch_step_through_the_mixed_chain_equals_the_per_candidate_path: the errors arrive divided by that test's
#              per-key bound (REL_PATH_SELF_TOL on the relation-path keys, 1e-4 elsewhere), so 1 is the bound
#   weight     test_chain_equals_per_operator_path_supernet_weight_step (_compare): likewise, 1e-6 on the logits
BOUNDS = {
    'mha': {'O': 1e-5, 'dQ': 1e-4, 'dK': 1e-4, 'dV': 1e-4, 'dbias': 1e-4},
    'rel_fused': {'bias': 1e-3, 'dWr': 1e-3, 'dbr': 1e-3, 'dWy': 1e-3, 'dby': 1e-3, 'fwd_differs_from_dense': 0.5, 'fwd_wrote_outside': 0.5,
                  'ragged_dWy': 2e-4, 'ragged_dby': 2e-4, 'ragged_dWr': 2e-4, 'ragged_dbr': 2e-4, 'nonfinite': 0.5},
    'rel_multi': {'r': 2e-5, 'fwd_wrote_outside': 0.5, 'dWr': 1e-4, 'dbr': 1e-4, 'dWy': 1e-4, 'dby': 1e-4,
                  'r_vs_per_op': 2e-5, 'dWr_vs_per_op': 3e-4, 'dbr_vs_per_op': 3e-4, 'dWy_vs_per_op': 3e-4, 'dby_vs_per_op': 3e-4},
    'arch': {'loss': 1e-5, 'gate_grads': 1e-4, 'gate_grads_all_zero': 0.5, 'alpha': 1e-5, 'grads_over_bound': 1.0, 'too_few_grads': 0.5},
    'weight': {'out': 1e-6, 'grads_over_bound': 1.0, 'chain_not_taken': 0.5},
}


def bounds_of(case, shape):
    kind = CASES[case]['kind']
    if kind == 'chain_misc':
        kind = 'weight' if isinstance(shape[0], str) else 'arch'
    return BOUNDS[kind]


# ------------------------------------------------------------------------------------------------------------- GPU half
DEV = 'cuda'


def _g(t):
    import torch
    return torch.as_tensor(t).to(DEV).contiguous()


def _rnd(rs, *shape):
    import numpy as np
    return rs.standard_normal(shape).astype(np.float32)


def _switches(env):
    """What the native table reports for the case's switches now (after the kernels ran)."""
    from mmnas_amd import switches as S
    t = S.native()
    return {k: {'value': t[k]['value'], 'source': t[k]['source'], 'read': bool(t[k]['read'])} for k in env}


def _mha_desc(L, B, H, Sq, Sk, di, Qd, Kd, Vd, m8, bd, O_, stats, p, seed):
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, 64
    d.ldq = d.ldk = d.ldv = d.ldo = di
    d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = L.fptr(Qd), L.fptr(Kd), L.fptr(Vd), L.ptr(m8), L.fptr(bd), L.fptr(O_), L.fptr(stats)
    d.drop_p, d.drop_site, d.drop_seed = p, 0, seed
    return d


def run_mha(shape):
    """test_mha_core's problem and reference at d_h = 64 (tests/test_kernels_gpu.py)."""
    import ctypes as C
    import numpy as np
    import torch
    import mmnas_amd._lib as L
    from oracle import dropout_rng
    from tests.kernel_refs import mha_ref
    from tests.util import rel_err
    if shape[0] == 'packed':
        return run_mha_packed(*shape[1:])
    B, H, Sq, Sk, use_mask, use_bias, p = shape
    dh, di = 64, H * 64
    rs = np.random.RandomState(B + H * 3 + Sq * 5 + Sk * 7 + dh)
    Q, K, V, dO = _rnd(rs, B, Sq, di), _rnd(rs, B, Sk, di), _rnd(rs, B, Sk, di), _rnd(rs, B, Sq, di)
    mask = np.zeros((B, Sk), np.bool_)
    if use_mask:
        for b in range(1, B):
            mask[b, int(rs.randint(1, Sk)):] = True
        mask[B - 1] = True      # fully padded sample: uniform softmax
    biasT = (_rnd(rs, B, H, Sk, Sq) * 2) if use_bias else None
    seed = 31337
    Qd, Kd, Vd, dOd = _g(Q), _g(K), _g(V), _g(dO)
    m8 = _g(mask.astype(np.uint8)) if use_mask else None
    bd = _g(biasT) if use_bias else None
    O_ = torch.full((B, Sq, di), float('nan'), device=DEV)
    stats = torch.empty(B, H, Sq, 2, device=DEV)
    d = _mha_desc(L, B, H, Sq, Sk, di, Qd, Kd, Vd, m8, bd, O_, stats, p, seed)
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    dQ, dK, dV = (torch.full_like(t, float('nan')) for t in (Qd, Kd, Vd))
    dbT = torch.full((B, H, Sk, Sq), float('nan'), device=DEV) if use_bias else None
    delta = torch.empty(B, H, Sq, device=DEV)
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQ), L.fptr(dK), L.fptr(dV), L.fptr(dbT), L.fptr(delta)
    L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
    torch.cuda.synchronize()
    Qt, Kt, Vt = (torch.from_numpy(v).double().requires_grad_(True) for v in (Q, K, V))
    bt = torch.from_numpy(biasT).double().requires_grad_(True) if use_bias else None
    dm = torch.from_numpy(dropout_rng.scaled_mask(seed, 0, (B, H, Sq, Sk), p)).double() if p > 0 else None
    ref = mha_ref(Qt, Kt, Vt, torch.from_numpy(mask) if use_mask else None, bt, H, dh, dm)
    ref.backward(torch.from_numpy(dO).double())
    err = {'O': rel_err(O_.cpu().numpy(), ref.detach().numpy()), 'dQ': rel_err(dQ.cpu().numpy(), Qt.grad.numpy()),
           'dK': rel_err(dK.cpu().numpy(), Kt.grad.numpy()), 'dV': rel_err(dV.cpu().numpy(), Vt.grad.numpy())}
    if use_bias:
        err['dbias'] = rel_err(dbT.cpu().numpy(), bt.grad.numpy())
    return err


def run_mha_packed(B, H, Sqm, Skm, use_bias, p):
    """test_mha_core_packed_rows' problem with q_off and k_off: the worst error over the sequences, each against the float64
    reference of that sequence alone."""
    import ctypes as C
    import numpy as np
    import torch
    import mmnas_amd._lib as L
    from oracle import dropout_rng
    from tests.kernel_refs import mha_ref
    from tests.util import rel_err
    rs = np.random.RandomState(B * 7 + H + Sqm + Skm)
    dh, di = 64, H * 64
    lq = [int(rs.randint(1, Sqm + 1)) for _ in range(B)]
    lq[0], lq[-1] = Sqm, 1                       # the longest and the shortest
    lk = list(lq) if Sqm == Skm else [int(rs.randint(1, Skm + 1)) for _ in range(B)]
    qoff = np.concatenate([[0], np.cumsum(lq)]).astype(np.int32)
    koff = np.concatenate([[0], np.cumsum(lk)]).astype(np.int32)
    Nq, Nk = int(qoff[-1]), int(koff[-1])
    Q, dO, K, V = _rnd(rs, Nq, di), _rnd(rs, Nq, di), _rnd(rs, Nk, di), _rnd(rs, Nk, di)
    biasT = (_rnd(rs, B, H, Skm, Sqm) * 2) if use_bias else None
    seed = 777
    Qd, Kd, Vd, dOd = _g(Q), _g(K), _g(V), _g(dO)
    bd = _g(biasT) if use_bias else None
    O_ = torch.full((Nq, di), float('nan'), device=DEV)
    stats = torch.zeros(B, H, Sqm, 2, device=DEV)
    qo, ko = _g(qoff), _g(koff)
    d = _mha_desc(L, B, H, Sqm, Skm, di, Qd, Kd, Vd, None, bd, O_, stats, p, seed)
    d.q_off, d.k_off = L.ptr(qo), L.ptr(ko)
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    dQ, dK, dV = (torch.full_like(t, float('nan')) for t in (Qd, Kd, Vd))
    dbT = torch.zeros(B, H, Skm, Sqm, device=DEV) if use_bias else None
    delta = torch.empty(B, H, Sqm, device=DEV)
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQ), L.fptr(dK), L.fptr(dV), L.fptr(dbT), L.fptr(delta)
    L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
    torch.cuda.synchronize()
    dm_all = dropout_rng.scaled_mask(seed, 0, (B, H, Sqm, Skm), p) if p > 0 else None
    Oc, dQc, dKc, dVc = O_.cpu().numpy(), dQ.cpu().numpy(), dK.cpu().numpy(), dV.cpu().numpy()
    dbc = dbT.cpu().numpy() if use_bias else None
    err = {'O': 0.0, 'dQ': 0.0, 'dK': 0.0, 'dV': 0.0}
    if use_bias:
        err['dbias'] = 0.0
    worst = lambda k, e: err.__setitem__(k, e if not np.isfinite(e) else max(err[k], e))
    for b in range(B):
        q0, q1, k0, k1 = int(qoff[b]), int(qoff[b + 1]), int(koff[b]), int(koff[b + 1])
        nq, nk = q1 - q0, k1 - k0
        Qt, Kt, Vt = (torch.from_numpy(a).double().unsqueeze(0).requires_grad_(True) for a in (Q[q0:q1], K[k0:k1], V[k0:k1]))
        bt = torch.from_numpy(biasT[b:b + 1, :, :nk, :nq].copy()).double().requires_grad_(True) if use_bias else None
        dm = torch.from_numpy(dm_all[b:b + 1, :, :nq, :nk].copy()).double() if p > 0 else None
        ref = mha_ref(Qt, Kt, Vt, None, bt, H, dh, dm)
        ref.backward(torch.from_numpy(dO[q0:q1]).double().unsqueeze(0))
        worst('O', rel_err(Oc[q0:q1], ref[0].detach().numpy()))
        worst('dQ', rel_err(dQc[q0:q1], Qt.grad[0].numpy()))
        worst('dK', rel_err(dKc[k0:k1], Kt.grad[0].numpy()))
        worst('dV', rel_err(dVc[k0:k1], Vt.grad[0].numpy()))
        if use_bias:
            worst('dbias', rel_err(dbc[b, :, :nk, :nq], bt.grad[0].numpy()))
    return err


def run_rel_fused(shape):
    import numpy as np
    import torch
    import mmnas_amd._lib as L
    from tests.kernel_refs import rel_fused_ref
    from tests.util import rel_err
    lib = L.lib()
    R = 64
    if shape[0] == 'dense':      # test_rel_fused_lazy_handle
        _, B, Sq, Sk, C, H = shape
        rs = np.random.RandomState(B * 131 + Sq + H + C)
        raw = _rnd(rs, B, Sq, Sk, C)
        raw[:, Sq // 2:, :, :] *= (rs.uniform(size=(B, Sq - Sq // 2, Sk, 1)) < 0.7)   # zero-padded rows, as the loader makes
        Wy, by, Wr, br = _rnd(rs, R, C) / 2, 0.1 * _rnd(rs, R), _rnd(rs, H, R) / 8, 0.1 * _rnd(rs, H)
        gb = _rnd(rs, B, H, Sk, Sq)
        rawd, Wyd, byd, Wrd, brd, gbd = _g(raw), _g(Wy), _g(by), _g(Wr), _g(br), _g(gb)
        assert lib.mmnas_rel_fused_supported(C, R, H) == 1
        biasT = torch.full((B, H, Sk, Sq), float('nan'), device=DEV)
        L.check(lib.mmnas_rel_fused_fwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(biasT), B, Sq, Sk, C, R, H, L.stream()))
        dWy, dby = torch.zeros(R, C, device=DEV), torch.zeros(R, device=DEV)
        dWr, dbr = torch.zeros(H, R, device=DEV), torch.zeros(H, device=DEV)
        ws = torch.empty(lib.mmnas_rel_fused_bwd_ws_floats(B, Sq, Sk), device=DEV)
        L.check(lib.mmnas_rel_fused_bwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(gbd),
                                        L.fptr(dWy), L.fptr(dby), L.fptr(dWr), L.fptr(dbr), L.fptr(ws), B, Sq, Sk, C, R, H, L.stream()))
        torch.cuda.synchronize()
        bias, rWy, rby, rWr, rbr = rel_fused_ref(raw, Wy, by, Wr, br, gb)
        return {'bias': rel_err(biasT.cpu().numpy(), bias), 'dWr': rel_err(dWr.cpu().numpy(), rWr), 'dbr': rel_err(dbr.cpu().numpy(), rbr),
                'dWy': rel_err(dWy.cpu().numpy(), rWy), 'dby': rel_err(dby.cpu().numpy(), rby)}
    _, B, S, C, H, lens = shape      # test_rel_fused_ragged
    rs = np.random.RandomState(B * 17 + S + H + C)
    raw = _rnd(rs, B, S, S, C)
    Wy, by, Wr, br = _rnd(rs, R, C) / 2, 0.1 * _rnd(rs, R), _rnd(rs, H, R) / 8, 0.1 * _rnd(rs, H)
    gb = _rnd(rs, B, H, S, S)
    valid = np.zeros((B, 1, S, S), np.float32)
    for b, n in enumerate(lens):
        valid[b, :, :n, :n] = 1
    rawd, Wyd, byd, Wrd, brd = _g(raw), _g(Wy), _g(by), _g(Wr), _g(br)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    toff = np.concatenate([[0], np.cumsum([(n * n + 31) // 32 for n in lens])]).astype(np.int32)
    offd, toffd = _g(off), _g(toff)
    dense = torch.empty(B, H, S, S, device=DEV)
    L.check(lib.mmnas_rel_fused_fwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(dense), B, S, S, C, R, H, L.stream()))
    rag = torch.full((B, H, S, S), 12345.0, device=DEV)
    L.check(lib.mmnas_rel_fused_fwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(rag), B, S, C, R, H,
                                           L.ptr(offd), L.stream()))
    v = torch.from_numpy(valid).to(DEV).bool().expand(B, H, S, S)
    err = {'fwd_differs_from_dense': float(not torch.equal(rag[v], dense[v])), 'fwd_wrote_outside': float(not bool((rag[~v] == 12345.0).all()))}
    outs = []
    for ragged in (False, True):
        dWy, dby = torch.zeros(R, C, device=DEV), torch.zeros(R, device=DEV)
        dWr, dbr = torch.zeros(H, R, device=DEV), torch.zeros(H, device=DEV)
        ws = torch.empty(lib.mmnas_rel_fused_bwd_ws_floats(B, S, S), device=DEV)
        if ragged:
            gbd = _g(np.where(valid > 0, gb, np.nan).astype(np.float32))      # outside the corners: never read
            L.check(lib.mmnas_rel_fused_bwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(gbd),
                                                   L.fptr(dWy), L.fptr(dby), L.fptr(dWr), L.fptr(dbr), L.fptr(ws), B, S, C, R, H,
                                                   L.ptr(offd), L.ptr(toffd), int(toff[-1]), L.stream()))
        else:
            gbd = _g(gb * valid)
            L.check(lib.mmnas_rel_fused_bwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(gbd),
                                            L.fptr(dWy), L.fptr(dby), L.fptr(dWr), L.fptr(dbr), L.fptr(ws), B, S, S, C, R, H, L.stream()))
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (dWy, dby, dWr, dbr)])
    err['nonfinite'] = float(not all(np.isfinite(a).all() for a in outs[1]))
    for name, a, c in zip(('dWy', 'dby', 'dWr', 'dbr'), outs[1], outs[0]):
        err['ragged_' + name] = rel_err(a, c)
    return err


def run_rel_multi(shape):
    """test_rel_multi_all_relation_operators_in_one_launch's problem (tests/test_kernels_gpu.py)."""
    import ctypes as C_
    import numpy as np
    import torch
    import mmnas_amd._lib as L
    from tests.kernel_refs import rel_multi_pre, rel_multi_ref
    from tests.util import rel_err
    lib = L.lib()
    B, S, C, H, n_ops, lens = shape
    rs = np.random.RandomState(B * 31 + S + 7 * H + C + n_ops)
    R = 64
    assert lib.mmnas_rel_multi_supported(C, R, H) == 1
    raw = _rnd(rs, B, S, S, C)
    Wy, by = _rnd(rs, R, C) / 2, 0.1 * _rnd(rs, R)
    Wrs = [_rnd(rs, H, R) / 8 for _ in range(n_ops)]
    brs = [0.1 * _rnd(rs, H) for _ in range(n_ops)]
    gbs = [_rnd(rs, B, H, S, S) for _ in range(n_ops)]
    valid = np.ones((B, 1, S, S), np.float32)
    offd = toffd = None
    ntiles = 0
    if lens is not None:
        valid[:] = 0
        for b, n in enumerate(lens):
            valid[b, :, :n, :n] = 1
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        toff = np.concatenate([[0], np.cumsum([(n * n + 31) // 32 for n in lens])]).astype(np.int32)
        offd, toffd, ntiles = _g(off), _g(toff), int(toff[-1])
    vmask = torch.from_numpy(valid).bool().expand(B, H, S, S)
    rawd, Wyd, byd = _g(raw), _g(Wy), _g(by)
    Wrd, brd = [_g(w) for w in Wrs], [_g(b) for b in brs]
    # elements whose pre-activation sits next to the clamp's jump stay out of the gradient (see the mirrored test)
    for i in range(n_ops):
        gbs[i] = np.where(np.abs(rel_multi_pre(raw, Wy, by, Wrs[i], brs[i])) < 0.05, 0.0, gbs[i]).astype(np.float32)
    gbd = [_g(np.where(valid > 0, gb, np.nan).astype(np.float32)) for gb in gbs]      # outside the corners: never read
    bias = [torch.full((B, H, S, S), 12345.0, device=DEV) for _ in range(n_ops)]
    dWr, dbr = [torch.zeros(H, R, device=DEV) for _ in range(n_ops)], [torch.zeros(H, device=DEV) for _ in range(n_ops)]
    dWy, dby = torch.zeros(R, C, device=DEV), torch.zeros(R, device=DEV)
    ws = torch.empty(lib.mmnas_rel_multi_bwd_ws_floats(B, S), device=DEV)
    m = L.RelMulti()
    m.B, m.S, m.C, m.R, m.H, m.n_ops = B, S, C, R, H, n_ops
    m.raw, m.Wy, m.by, m.dWy, m.dby, m.ws = L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(dWy), L.fptr(dby), L.fptr(ws)
    for i in range(n_ops):
        m.Wr[i], m.br[i], m.biasT[i], m.dbiasT[i] = L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(bias[i]), L.fptr(gbd[i])
        m.dWr[i], m.dbr[i] = L.fptr(dWr[i]), L.fptr(dbr[i])
    if lens is not None:
        m.off, m.tile_off, m.ntiles = L.ptr(offd), L.ptr(toffd), ntiles
    L.check(lib.mmnas_rel_multi_fwd(C_.byref(m), L.stream()))
    L.check(lib.mmnas_rel_multi_bwd(C_.byref(m), L.stream()))
    torch.cuda.synchronize()
    r_ref, rWr, rbr, rWy, rby = rel_multi_ref(raw, Wy, by, Wrs, brs, gbs, valid)
    vm = valid.astype(np.float64)
    err = {k: 0.0 for k in BOUNDS['rel_multi']}
    up = lambda k, e: err.__setitem__(k, e if not np.isfinite(e) else max(err[k], e))
    for i in range(n_ops):
        got = bias[i].cpu()
        up('fwd_wrote_outside', float(not bool((got[~vmask] == 12345.0).all())))
        rr = torch.exp(torch.where(vmask, got, torch.zeros(())).double()).numpy()
        up('r', float((np.abs(rr - r_ref[i]) * vm).max()) / float(np.abs(r_ref[i]).max()))
        up('dWr', rel_err(dWr[i].cpu().numpy(), rWr[i]))
        up('dbr', rel_err(dbr[i].cpu().numpy(), rbr[i]))
    up('dWy', rel_err(dWy.cpu().numpy(), rWy))
    up('dby', rel_err(dby.cpu().numpy(), rby))
    # ... and the per-operator kernels of relfused.hip: same numbers to round-off
    p_dWy, p_dby = torch.zeros(R, C, device=DEV), torch.zeros(R, device=DEV)
    ws1 = torch.empty(lib.mmnas_rel_fused_bwd_ws_floats(B, S, S), device=DEV)
    vd = vmask.to(DEV)
    for i in range(n_ops):
        pb = torch.full((B, H, S, S), 12345.0, device=DEV)
        p_dWr, p_dbr = torch.zeros(H, R, device=DEV), torch.zeros(H, device=DEV)
        if lens is None:
            L.check(lib.mmnas_rel_fused_fwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(pb), B, S, S, C, R, H, L.stream()))
            L.check(lib.mmnas_rel_fused_bwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(gbd[i]),
                                            L.fptr(p_dWy), L.fptr(p_dby), L.fptr(p_dWr), L.fptr(p_dbr), L.fptr(ws1), B, S, S, C, R, H, L.stream()))
        else:
            L.check(lib.mmnas_rel_fused_fwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(pb), B, S, C, R, H,
                                                   L.ptr(offd), L.stream()))
            L.check(lib.mmnas_rel_fused_bwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(gbd[i]),
                                                   L.fptr(p_dWy), L.fptr(p_dby), L.fptr(p_dWr), L.fptr(p_dbr), L.fptr(ws1), B, S, C, R, H,
                                                   L.ptr(offd), L.ptr(toffd), ntiles, L.stream()))
        torch.cuda.synchronize()
        a, c = torch.exp(torch.where(vd, bias[i], 0.0).double()), torch.exp(torch.where(vd, pb, 0.0).double())
        up('r_vs_per_op', float((a - c).abs().max()) / float(c.abs().max()))
        up('dWr_vs_per_op', rel_err(dWr[i].cpu().numpy(), p_dWr.cpu().numpy()))
        up('dbr_vs_per_op', rel_err(dbr[i].cpu().numpy(), p_dbr.cpu().numpy()))
    up('dWy_vs_per_op', rel_err(dWy.cpu().numpy(), p_dWy.cpu().numpy()))
    up('dby_vs_per_op', rel_err(dby.cpu().numpy(), p_dby.cpu().numpy()))
    return err


def _build_net(cls, c):
    import numpy as np
    import torch
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()})
    return net.to('cuda:0').train()


def run_arch(shape):
    """The architecture step through the mixed chain (MMNAS_MIXED_CHAIN=1) against the per-candidate path (=0) in this process:
    loss, gate gradients, the alpha update, every weight gradient -- the comparison of
    test_arch_step_through_the_mixed_chain_equals_the_per_candidate_path, with the same dropout masks on both paths."""
    import numpy as np
    import torch
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd import ops
    from mmnas_amd.harness import SearchLoop
    from tests.golden import cases
    from tests.util import REL_PATH_SELF_TOL, is_rel_path, rel_err
    seed, hsize, B, Sx, Sy, mode, dropout = shape
    c = cases.net_case('vqa', None, seed, search=True, HSIZE=hsize, B=B, Sx=Sx, Sy=Sy)
    c['cfg'].DROPOUT_R = dropout
    pl = cases.search_plan(np.random.RandomState(6), mode)
    plan = pl['enc'] + pl['dec']
    if os.environ.get('MMNAS_SMALL_BWD') == '0':      # the switch decides something only for a sampled SelfAtt (candidate 0) of an encoder node
        assert hsize in (256, 512) and Sx <= 16 and any(act == [0] for act, _ in pl['enc']), (shape, pl['enc'])
    inp = tuple(torch.from_numpy(a).to('cuda:0') for a in c['inputs'])
    tgt = torch.from_numpy(c['target']).to('cuda:0')
    res = {}
    # The per-candidate path draws its dropout seeds sampled candidate first, the chain in candidate order: with the running
    # seed counter the same operator would get different masks on the two paths.  One fixed seed for every operator gives each
    # operator the same masks on both (a mask depends on seed, site and element index only).
    draw, ops.next_seed = ops.next_seed, (lambda: 0x0BADC0DE12345678)
    for chain in ('0', '1'):
        os.environ['MMNAS_MIXED_CHAIN'] = chain      # (read at every call on the Python side)
        net = _build_net(Net_Search, c)
        loop = SearchLoop(net, arch_mode=mode)
        try:
            loss = loop.arch_step(inp, tgt, plan=plan)
            torch.cuda.synchronize()
            gg, _ = net._flat_grads
            res[chain] = dict(loss=float(loss), gg=gg.cpu().numpy().copy(),
                              alpha=np.stack([np.pad(m.alpha_prob.detach().cpu().numpy(), (0, 4 - m.n_choices)) for m in net.redundant_modules]),
                              grads={k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_net_parameters() if p.grad is not None})
        finally:
            loop.reducer.fg.disable_sinks()
    ops.next_seed = draw
    os.environ.pop('MMNAS_MIXED_CHAIN', None)
    a, b = res['0'], res['1']
    top = max(float(np.abs(v).max()) for v in a['grads'].values())
    worst, worst_key = 0.0, None
    for k, v in a['grads'].items():
        bound = (REL_PATH_SELF_TOL if is_rel_path(k) else 1e-4) * max(float(np.abs(v).max()), 1e-3 * top)
        e = float(np.abs(b['grads'][k] - v).max()) / bound
        if not e <= worst:
            worst, worst_key = e, k
    nz = sum(float(np.abs(v).max()) > 0 for v in a['grads'].values())
    return {'loss': abs(a['loss'] - b['loss']) / abs(a['loss']), 'gate_grads': rel_err(b['gg'], a['gg']),
            'gate_grads_all_zero': float(not float(np.abs(a['gg']).max()) > 0), 'alpha': rel_err(b['alpha'], a['alpha']),
            'grads_over_bound': worst, 'worst_key': worst_key, 'too_few_grads': float(not nz > 60)}


def run_weight(shape):
    """The supernet's weight step: the backbone chain with its side stream against the per-operator path -- _run / _compare of
    tests/test_chain_gpu.py."""
    import importlib
    import numpy as np
    import torch
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import dp, ops
    from tests.golden import cases
    from tests.util import REL_PATH_SELF_TOL, is_rel_path, rel_err
    task, plan_seed, B, Sx, Sy, dropout = shape
    pl = cases.search_plan(np.random.RandomState(plan_seed), None)
    plan = pl['enc'] + pl['dec']
    calls = []
    orig = ops.backbone_chain
    ops.backbone_chain = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    res = {}
    try:
        for chain in (False, True):
            os.environ.update(MMNAS_CHAIN='1' if chain else '0', MMNAS_SIDE_STREAM='1' if chain else '0', MMNAS_HEAD_GLIMPSE1='1')
            c = cases.net_case(task, None, 31337, search=True, B=B, Sx=Sx, Sy=Sy)
            c['cfg'].DROPOUT_R = dropout
            net = _build_net(importlib.import_module('mmnas.model.hygr_%s' % task).Net_Search, c)
            inp = tuple(torch.from_numpy(a).to('cuda:0') for a in c['inputs'])
            tgt = torch.from_numpy(c['target']).to('cuda:0')
            ops.manual_seed(99)
            MixedOp.MODE = None
            net.set_sampled(plan)
            red = dp.SupernetReducer(net)
            red.begin_weight_step()
            n0 = len(calls)
            try:
                pred = net(inp)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, tgt, reduction='sum')
                loss.backward()
                red.finish_weight_step()
                torch.cuda.synchronize()
                res[chain] = (pred.detach().cpu().numpy(), {k: (p.grad.detach().cpu().numpy().copy() if p.grad is not None else None)
                                                            for k, p in net.named_parameters()}, len(calls) - n0)
            finally:
                red.fg.disable_sinks()
    finally:
        ops.backbone_chain = orig
        for k in ('MMNAS_CHAIN', 'MMNAS_SIDE_STREAM', 'MMNAS_HEAD_GLIMPSE1'):
            os.environ.pop(k, None)
    (out_a, g_a, n_a), (out_b, g_b, n_b) = res[True], res[False]
    top = max(float(np.abs(g).max()) for g in g_b.values() if g is not None)
    worst, worst_key = 0.0, None
    for k in g_b:
        if g_b[k] is None:
            e = float(g_a[k] is not None and bool(np.any(g_a[k]))) * 2.0
        elif g_a[k] is None:
            e = 2.0
        else:
            e = float(np.abs(g_a[k] - g_b[k]).max()) / ((REL_PATH_SELF_TOL if is_rel_path(k) else 2e-5) * max(float(np.abs(g_b[k]).max()), 1e-3 * top))
        if not e <= worst:
            worst, worst_key = e, k
    return {'out': rel_err(out_a, out_b), 'grads_over_bound': worst, 'worst_key': worst_key, 'chain_not_taken': float(not (n_a == 1 and n_b == 0))}


def run_chain_misc(shape):
    return run_weight(shape) if isinstance(shape[0], str) else run_arch(shape)


RUNNERS = {'mha': run_mha, 'rel_fused': run_rel_fused, 'rel_multi': run_rel_multi, 'arch': run_arch, 'chain_misc': run_chain_misc}


def main(argv):
    if len(argv) != 2 or (argv[1] != '--list' and argv[1] not in CASES):
        print('usage: python tests/fallback_cases.py CASE | --list\ncases: ' + ' '.join(CASES), file=sys.stderr)
        return 2
    if argv[1] == '--list':
        for name, c in CASES.items():
            print(json.dumps({'case': name, 'env': c['env'], 'kind': c['kind'], 'shapes': c['shapes']}))
        return 0
    case = CASES[argv[1]]
    for k, v in case['env'].items():
        assert os.environ.get(k) == v, 'start this process with %s=%s (it has %r)' % (k, v, os.environ.get(k))
    import torch
    assert torch.cuda.is_available(), 'the cases run on the GPU'
    for shape in case['shapes']:
        err = RUNNERS[case['kind']](shape)
        notes = {k: err.pop(k) for k in list(err) if not isinstance(err[k], float)}
        print(json.dumps({'case': argv[1], 'shape': shape, 'errors': err, 'notes': notes, 'switches': _switches(case['env'])}), flush=True)
    print(json.dumps({'case': argv[1], 'done': len(case['shapes'])}), flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
