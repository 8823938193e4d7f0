"""Packed rows (mmnas_mha_desc.q_off / k_off) of the attention cores at every head size but 64: d_h in {16, 32, 128, 256}.

The body of tests/test_kernels_gpu.py::test_mha_core_packed_rows generalised over d_h.  d_h = 64 runs the fused / bf16-pipe kernels
(checked there); the other head sizes run mha_fwd_kernel and the general backward pair mha_bwd_q_kernel + mha_bwd_kv_kernel (d_h > 64:
behind mha_delta_packed_kernel), which take a sequence's length and row base from the offsets and keep the padded strides for
stats / delta / bias / mask / the dropout index.

Every sequence is checked against the float64 reference of that sequence alone, at the bars of test_mha_core: relative error < 1e-5 on
O, < 1e-4 on dQ / dK / dV / the n_k x n_q corner of dbiasT.  O, dQ, dK, dV start as NaN; every row-indexed buffer carries GUARD rows
behind its last row -- NaN behind the inputs (a read that counts shows as NaN), a sentinel behind the outputs (a write shows) -- so a
wrong clamp or row base is seen there or as NaN in a neighbouring sequence."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.kernel_refs import mha_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 4
GUARD = 3
SENTINEL = 7777.0
SEED = 777
HEADS = [(16, 3), (32, 2), (128, 2), (256, 1)]
# (Sq_max, Sk_max, packed_q, packed_k, bias, p)
SHAPES = [
    (100, 100, True, True, True, 0.1),     # self: two key blocks, four-wave groups, relation-style bias, dropout replay
    (36, 50, True, True, False, 0.0),      # both sides packed at different lengths
    (100, 14, True, False, False, 0.0),    # packed queries, padded masked keys: the QS = 4 key-owner form
    (14, 100, False, True, False, 0.2),    # dense queries over packed keys: the guided operator over a ragged language stream
    (33, 33, True, True, True, 0.0),       # one row past a block edge
    (128, 128, True, True, False, 0.0),    # the longest
]
MMNAS_E_SHAPE, MMNAS_E_ARG = -1, -2


def g(t):
    return torch.as_tensor(t).to(DEV).contiguous()


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(dh, H, Sqm, Skm, packed_q, packed_k, use_bias, p):
    """Inputs and the per-sequence float64 references of one case: computed once, shared by the tests that run it, never written."""
    from oracle import dropout_rng
    rs = np.random.RandomState(B * 7 + H + Sqm + Skm + dh)
    di = H * dh
    lq = [int(rs.randint(1, Sqm + 1)) for _ in range(B)]
    lq[0], lq[-1] = Sqm, 1                       # the longest and the shortest
    self_att = packed_q and packed_k and Sqm == Skm
    if self_att:
        lk = list(lq)
    else:
        lk = [int(rs.randint(1, Skm + 1)) for _ in range(B)]
        lk[0], lk[-1] = 1, Skm                   # (the other way round: 1 key under the most queries)
    if not packed_q:
        lq = [Sqm] * B
    qoff = np.concatenate([[0], np.cumsum(lq)]).astype(np.int32)
    koff = np.concatenate([[0], np.cumsum(lk)]).astype(np.int32)
    Nq, Nk = int(qoff[-1]), (int(koff[-1]) if packed_k else B * Skm)
    Q, dO, K, V = rnd(rs, Nq, di), rnd(rs, Nq, di), rnd(rs, Nk, di), rnd(rs, Nk, di)
    mask = None
    if not packed_k:                             # padded keys with their mask (the guided operators: keys = the language stream)
        mask = np.zeros((B, Skm), np.bool_)
        for b in range(B):
            mask[b, lk[b]:] = True
    biasT = (rnd(rs, B, H, Skm, Sqm) * 2) if use_bias else None
    dm_all = dropout_rng.scaled_mask(SEED, 0, (B, H, Sqm, Skm), p) if p > 0 else None
    refs = []
    for b in range(B):
        q0, q1 = int(qoff[b]), int(qoff[b + 1])
        k0, k1 = (int(koff[b]), int(koff[b + 1])) if packed_k else (b * Skm, b * Skm + lk[b])
        nq, nk = q1 - q0, k1 - k0
        Qt, Kt, Vt = (torch.from_numpy(a).double().unsqueeze(0).requires_grad_(True) for a in (Q[q0:q1], K[k0:k1], V[k0:k1]))
        bt = torch.from_numpy(biasT[b:b + 1, :, :nk, :nq].copy()).double().requires_grad_(True) if use_bias else None
        dm = torch.from_numpy(dm_all[b:b + 1, :, :nq, :nk].copy()).double() if p > 0 else None
        ref = mha_ref(Qt, Kt, Vt, None, bt, H, dh, dm)
        ref.backward(torch.from_numpy(dO[q0:q1]).double().unsqueeze(0))
        refs.append(dict(q=(q0, q1), k=(k0, k1), O=ref[0].detach().numpy(), dQ=Qt.grad[0].numpy(), dK=Kt.grad[0].numpy(),
                         dV=Vt.grad[0].numpy(), db=bt.grad[0].numpy() if use_bias else None))
    return dict(dh=dh, H=H, Sqm=Sqm, Skm=Skm, packed_q=packed_q, packed_k=packed_k, p=p, lk=lk, qoff=qoff, koff=koff, Nq=Nq, Nk=Nk,
                Q=Q, dO=dO, K=K, V=V, mask=mask, biasT=biasT, refs=refs)


def _guarded(a, fill):
    """[N, di] host rows -> [N + GUARD, di] device rows, the guard rows filled with `fill`."""
    t = torch.full((a.shape[0] + GUARD, a.shape[1]), fill, device=DEV)
    t[:a.shape[0]] = g(a)
    return t


def _desc(c, bufs):
    import mmnas_amd._lib as L
    di = c['H'] * c['dh']
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, c['H'], c['Sqm'], c['Skm'], c['dh']
    d.ldq = d.ldk = d.ldv = d.ldo = di
    d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = (L.fptr(bufs['Q']), L.fptr(bufs['K']), L.fptr(bufs['V']), L.ptr(bufs['m8']),
                                                 L.fptr(bufs['bias']), L.fptr(bufs['O']), L.fptr(bufs['stats']))
    d.q_off = L.ptr(bufs['qo']) if c['packed_q'] else None
    d.k_off = L.ptr(bufs['ko']) if c['packed_k'] else None
    d.drop_p, d.drop_site, d.drop_seed = c['p'], 0, SEED
    return d


def _launch(c):
    """Forward + backward of one case -> the output buffers (guard rows included) on the host."""
    import mmnas_amd._lib as L
    H, Sqm, Skm, di = c['H'], c['Sqm'], c['Skm'], c['H'] * c['dh']
    nan = float('nan')
    bufs = dict(Q=_guarded(c['Q'], nan), K=_guarded(c['K'], nan), V=_guarded(c['V'], nan), dO=_guarded(c['dO'], nan),
                m8=g(c['mask'].astype(np.uint8)) if c['mask'] is not None else None,
                bias=g(c['biasT']) if c['biasT'] is not None else None, qo=g(c['qoff']), ko=g(c['koff']),
                stats=torch.zeros(B, H, Sqm, 2, device=DEV))
    out = dict(O=torch.full((c['Nq'] + GUARD, di), nan, device=DEV), dQ=torch.full((c['Nq'] + GUARD, di), nan, device=DEV),
               dK=torch.full((c['Nk'] + GUARD, di), nan, device=DEV), dV=torch.full((c['Nk'] + GUARD, di), nan, device=DEV))
    for k, n in (('O', c['Nq']), ('dQ', c['Nq']), ('dK', c['Nk']), ('dV', c['Nk'])):
        out[k][n:] = SENTINEL
    bufs['O'] = out['O']
    d = _desc(c, bufs)
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    dbT = torch.zeros(B, H, Skm, Sqm, device=DEV) if c['biasT'] is not None else None
    delta = torch.empty(B, H, Sqm, device=DEV)
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = (L.fptr(bufs['dO']), L.fptr(out['dQ']), L.fptr(out['dK']), L.fptr(out['dV']),
                                                 L.fptr(dbT), L.fptr(delta))
    L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['db'] = dbT.cpu().numpy() if dbT is not None else None
    return res


def _check(c, res):
    tag = 'dh=%d H=%d %dx%d' % (c['dh'], c['H'], c['Sqm'], c['Skm'])
    for k, n in (('O', c['Nq']), ('dQ', c['Nq']), ('dK', c['Nk']), ('dV', c['Nk'])):
        assert np.all(res[k][n:] == SENTINEL), (tag, k, 'guard rows written')
    worst = dict(O=0.0, dQ=0.0, dK=0.0, dV=0.0, db=0.0)
    fails = []
    for b, r in enumerate(c['refs']):
        (q0, q1), (k0, k1) = r['q'], r['k']
        nq, nk = q1 - q0, k1 - k0
        got = dict(O=res['O'][q0:q1], dQ=res['dQ'][q0:q1], dK=res['dK'][k0:k1], dV=res['dV'][k0:k1])
        if r['db'] is not None:
            got['db'] = res['db'][b, :, :nk, :nq]
        for k, a in got.items():
            if not np.isfinite(a).all():
                fails.append((b, k, 'not finite', nq, nk))
                continue
            e = rel_err(a, r[k])
            worst[k] = max(worst[k], e)
            if not e < (1e-5 if k == 'O' else 1e-4):
                fails.append((b, k, e, nq, nk))
    print('packed heads %s: worst rel_err O %.2e (bar 1e-5)  dQ %.2e  dK %.2e  dV %.2e  dbiasT %.2e (bar 1e-4)' %
          (tag, worst['O'], worst['dQ'], worst['dK'], worst['dV'], worst['db']))
    assert not fails, (tag, fails)
    if not c['packed_k']:    # padded keys: the rows behind a sequence's keys are masked keys -- their dK / dV are exact zeros
        for b in range(B):
            assert not np.any(res['dK'][b * c['Skm'] + c['lk'][b]:(b + 1) * c['Skm']]), (tag, b)
            assert not np.any(res['dV'][b * c['Skm'] + c['lk'][b]:(b + 1) * c['Skm']]), (tag, b)


@pytest.mark.parametrize('Sqm,Skm,packed_q,packed_k,use_bias,p', SHAPES)
@pytest.mark.parametrize('dh,H', HEADS)
def test_packed_rows_every_head_size(dh, H, Sqm, Skm, packed_q, packed_k, use_bias, p):
    c = _case(dh, H, Sqm, Skm, packed_q, packed_k, use_bias, p)
    _check(c, _launch(c))


@pytest.mark.parametrize('dh,H', HEADS)
def test_packed_rows_two_wave_workgroups(dh, H, monkeypatch):
    """MMNAS_MHA_NW=2 (read at every call): 100 queries on two-wave groups in the forward and the query-owner kernel, two-wave
    key-owner groups over the four key blocks."""
    monkeypatch.setenv('MMNAS_MHA_NW', '2')
    c = _case(dh, H, *SHAPES[0])
    _check(c, _launch(c))


@pytest.mark.parametrize('dh,H,shape', [(16, 3, SHAPES[2]), (32, 2, SHAPES[0]), (128, 2, SHAPES[3]), (256, 1, SHAPES[0])])
def test_packed_rows_run_to_run_identical(dh, H, shape):
    """No atomics, no order-dependent sums in these kernels: the same call twice gives the same bits (NaN-prefilled rows that a run
    left out would differ from themselves)."""
    c = _case(dh, H, *shape)
    a, b = _launch(c), _launch(c)
    for k in ('O', 'dQ', 'dK', 'dV', 'db'):
        if a[k] is not None:
            assert np.array_equal(a[k], b[k]), k


def _rc(call, d):
    import mmnas_amd._lib as L
    return int(call(C.byref(d), L.stream()))


@pytest.mark.parametrize('dh,H', HEADS)
def test_refusals_stay(dh, H):
    """A mask beside k_off is still MMNAS_E_ARG; 129 rows under q_off is still MMNAS_E_SHAPE; nothing is launched for either."""
    import mmnas_amd._lib as L
    c = _case(dh, H, *SHAPES[1])
    di = H * dh
    bufs = dict(Q=g(c['Q']), K=g(c['K']), V=g(c['V']), m8=g(np.zeros((B, c['Skm']), np.uint8)), bias=None, qo=g(c['qoff']), ko=g(c['koff']),
                stats=torch.zeros(B, H, 129, 2, device=DEV), O=torch.full((c['Nq'], di), SENTINEL, device=DEV))
    d = _desc(c, bufs)
    assert _rc(L.lib().mmnas_mha_core_fwd, d) == MMNAS_E_ARG
    d.mask = None
    d.Sq = 129
    assert _rc(L.lib().mmnas_mha_core_fwd, d) == MMNAS_E_SHAPE
    torch.cuda.synchronize()
    assert bool((bufs['O'] == SENTINEL).all())
