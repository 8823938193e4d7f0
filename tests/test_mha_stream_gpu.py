"""The streaming attention forward (mha_fwd_stream_kernel: the keys in blocks of 128, running maximum and sum) and everything
that rides on it at more than 256 keys: the core with its general backward, the four attention operators, the fixed-architecture
networks of the three tasks and one supernet step.  References are float64 (tests/kernel_refs.mha_ref, the CPU oracle); the
bounds are those of the tests whose set-up this file follows (test_kernels_gpu.py::test_mha_core: 1e-5 forward, 1e-4 backward;
test_small_gpu.py::_check and test_nets_gpu.py for operators and networks).

MMNAS_MHA_STREAM_MINK (read at every call) lowers the key count from which the forward streams, so one build runs the
streaming kernel and the one-shot kernels on the same problem.

When MMNAS_MHA_STREAM_STATS names a file, the worst errors of the core tests are written there at the end of the module
(profiles/r11_mha_stream_error_stats.json is one such run)."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import mmnas_oracle as O
from tests import oracle_runner as R
from tests.golden import cases
from tests.guardband import Arena
from tests.kernel_refs import mha_ref
from tests.test_ops_gpu import _drop_sites, run_hip_op
from tests.test_small_gpu import _check
from tests.util import TOL, check_grad_samples, esample, is_rel_path, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = torch.from_numpy
SEED = 31337
ERR = {}


def _note(group, what, e):
    k = '%s|%s' % (group, what)
    ERR[k] = max(ERR.get(k, 0.0), float(e))
    return e


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_MHA_STREAM_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


def _L():
    import mmnas_amd._lib as L
    return L


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def g(a):
    return None if a is None else T(np.ascontiguousarray(a)).to(DEV)


def ragged_mask(rs, B, Sk):
    """test_mha_core's masks: sample 0 unpadded, ragged tails, the last sample fully padded."""
    mask = np.zeros((B, Sk), np.bool_)
    for b in range(1, B if Sk > 1 else 1):
        mask[b, int(rs.randint(1, Sk)):] = True
    if B > 1:
        mask[B - 1] = True
    return mask


def inputs(B, H, Sq, Sk, dh, use_mask, use_bias):
    rs = np.random.RandomState(B + H * 3 + Sq * 5 + Sk * 7 + dh)
    di = H * dh
    Q, K, V, dO = rnd(rs, B, Sq, di), rnd(rs, B, Sk, di), rnd(rs, B, Sk, di), rnd(rs, B, Sq, di)
    mask = ragged_mask(rs, B, Sk) if use_mask else None
    biasT = (rnd(rs, B, H, Sk, Sq) * 2) if use_bias else None
    return dict(B=B, H=H, Sq=Sq, Sk=Sk, dh=dh, Q=Q, K=K, V=V, dO=dO, mask=mask, biasT=biasT)


def reference(c, p):
    """float64: O, (m, 1 / l) of the undropped softmax, dQ, dK, dV, dbiasT."""
    from oracle import dropout_rng
    B, H, Sq, Sk, dh = (c[k] for k in ('B', 'H', 'Sq', 'Sk', 'dh'))
    Qt, Kt, Vt = (T(c[k]).double().requires_grad_(True) for k in ('Q', 'K', 'V'))
    bt = T(c['biasT']).double().requires_grad_(True) if c['biasT'] is not None else None
    mt = T(c['mask']) if c['mask'] is not None else None
    dm = T(dropout_rng.scaled_mask(SEED, 0, (B, H, Sq, Sk), p)).double() if p > 0 else None
    ref = mha_ref(Qt, Kt, Vt, mt, bt, H, dh, dm)
    ref.backward(T(c['dO']).double())
    with torch.no_grad():
        z = Qt.reshape(B, Sq, H, dh).permute(0, 2, 1, 3) @ Kt.reshape(B, Sk, H, dh).permute(0, 2, 3, 1) / np.sqrt(dh)
        if bt is not None:
            z = z + bt.permute(0, 1, 3, 2)
        if mt is not None:
            z = z.masked_fill(mt.reshape(B, 1, 1, Sk), -1e9)
        m = z.max(-1).values
        inv = 1.0 / torch.exp(z - m.unsqueeze(-1)).sum(-1)
    return dict(O=ref.detach().numpy(), m=m.numpy(), inv=inv.numpy(), dQ=Qt.grad.numpy(), dK=Kt.grad.numpy(), dV=Vt.grad.numpy(),
                dbiasT=bt.grad.numpy() if bt is not None else None)


def run_core(c, p, bwd=True):
    """mmnas_mha_core_fwd (+ _bwd on the statistics it left) on dense tensors -> numpy results."""
    L = _L()
    B, H, Sq, Sk, dh = (c[k] for k in ('B', 'H', 'Sq', 'Sk', 'dh'))
    di = H * dh
    Qd, Kd, Vd, dOd = g(c['Q']), g(c['K']), g(c['V']), g(c['dO'])
    m8 = g(c['mask'].astype(np.uint8)) if c['mask'] is not None else None
    bd = g(c['biasT'])
    O_ = torch.empty(B, Sq, di, device=DEV)
    stats = torch.empty(B, H, Sq, 2, device=DEV)
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, dh
    d.ldq = d.ldk = d.ldv = d.ldo = di
    d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = L.fptr(Qd), L.fptr(Kd), L.fptr(Vd), L.ptr(m8), L.fptr(bd), L.fptr(O_), L.fptr(stats)
    d.drop_p, d.drop_site, d.drop_seed = p, 0, SEED
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    res = dict(O=O_.cpu().numpy(), m=stats[..., 0].cpu().numpy(), inv=stats[..., 1].cpu().numpy())
    if bwd:
        dQ, dK, dV = torch.empty_like(Qd), torch.empty_like(Kd), torch.empty_like(Vd)
        dbT = torch.empty(B, H, Sk, Sq, device=DEV) if bd is not None else None
        delta = torch.empty(B, H, Sq, device=DEV)
        d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQ), L.fptr(dK), L.fptr(dV), L.fptr(dbT), L.fptr(delta)
        L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
        res.update(dQ=dQ.cpu().numpy(), dK=dK.cpu().numpy(), dV=dV.cpu().numpy(), dbiasT=dbT.cpu().numpy() if dbT is not None else None)
    return res


def judge(group, got, ref, bwd=True):
    """test_mha_core's bounds; every figure is printed (and recorded) before it is asserted."""
    errs = {'O': rel_err(got['O'], ref['O'])}
    if bwd:
        for k in ('dQ', 'dK', 'dV', 'dbiasT'):
            if ref[k] is not None:
                errs[k] = rel_err(got[k], ref[k])
    print(group, ' '.join('%s %.2e' % kv for kv in errs.items()))
    for k, e in errs.items():
        _note(group, k, e)
    assert errs['O'] < 1e-5, errs
    assert all(e < 1e-4 for k, e in errs.items() if k != 'O'), errs


# ------------------------------------------------------------------------------------- 1. long keys, default threshold
# KB = 128 divides 384 and 640: 384 = 256 + KB is the case without a partial last block; 257, 513 leave one key in it.
LONG = [(2, 2, 1, 257, 64, True, False, 0.0), (2, 2, 33, 257, 64, True, True, 0.2), (2, 4, 100, 300, 64, True, True, 0.1),
        (3, 1, 130, 384, 64, True, False, 0.0), (2, 2, 40, 513, 32, True, True, 0.0), (2, 8, 9, 290, 16, False, False, 0.0),
        (2, 2, 35, 260, 128, True, False, 0.0), (2, 1, 7, 300, 256, True, True, 0.0), (1, 2, 150, 640, 64, True, False, 0.3)]


@pytest.mark.parametrize('B,H,Sq,Sk,dh,use_mask,use_bias,p', LONG)
def test_long_keys(B, H, Sq, Sk, dh, use_mask, use_bias, p):
    c = inputs(B, H, Sq, Sk, dh, use_mask, use_bias)
    judge('long', run_core(c, p), reference(c, p))


# ------------------------------------------------------------------------------------- 2. mask placement
@functools.lru_cache(maxsize=None)
def _placement(use_bias):
    B, H, Sq, Sk, dh = 4, 2, 33, 300, 64
    c = inputs(B, H, Sq, Sk, dh, False, True)
    mask = np.zeros((B, Sk), np.bool_)
    mask[0, 5:] = True            # only keys 0..4 live: every later block is wholly masked
    mask[1, :295] = True          # only keys 295..299 live: every earlier block is wholly masked
    mask[2] = True                # fully masked
    c['mask'] = mask              # sample 3: no padding
    if use_bias:
        c['biasT'][3, :, Sk - 1, :] = 30.0      # the maximum is raised in the last block: a rescale by a non-zero factor
        c['biasT'][3, :, 0, :] = -30.0
    else:
        c['biasT'] = None
    return c, reference(c, 0.0)


@pytest.mark.parametrize('use_bias', [True, False])
def test_mask_placement(use_bias):
    c, ref = _placement(use_bias)
    assert np.isfinite(ref['O']).all()
    got = run_core(c, 0.0)
    assert np.isfinite(got['O']).all() and np.isfinite(got['m']).all() and np.isfinite(got['inv']).all()
    for b in range(4):
        print('placement sample', b, 'O %.2e' % _note('placement', 'O|sample%d' % b, rel_err(got['O'][b], ref['O'][b])))
    judge('placement', got, ref)
    for b in range(4):
        assert rel_err(got['O'][b], ref['O'][b]) < 1e-5, b
    # the fully masked sample: a uniform map -- the mean of its V rows per head, statistics (-1e9, 1 / Sk)
    H, Sq, Sk, dh = c['H'], c['Sq'], c['Sk'], c['dh']
    mean_v = c['V'][2].astype(np.float64).mean(0)
    assert rel_err(got['O'][2], np.broadcast_to(mean_v, (Sq, H * dh))) < 1e-5
    assert np.all(got['m'][2] == np.float32(-1e9))
    assert np.allclose(got['inv'][2], 1.0 / Sk, rtol=1e-6, atol=0)
    if use_bias:      # sample 3's statistics: the late maximum
        assert np.abs(got['m'][3] - ref['m'][3]).max() <= 1e-5 * max(1.0, np.abs(ref['m'][3]).max())


# ------------------------------------------------------------------------------------- 3. streaming against the one-shot kernels
SHORT = [(7, 1, 64), (14, 14, 64), (40, 31, 64), (100, 33, 64), (100, 100, 64), (50, 200, 64), (130, 256, 64), (9, 15, 16), (7, 12, 256)]


@pytest.mark.parametrize('Sq,Sk,dh', SHORT)
def test_streaming_against_one_shot(Sq, Sk, dh, monkeypatch):
    B, H, p = 2, 2, 0.1
    c = inputs(B, H, Sq, Sk, dh, True, True)
    ref = reference(c, p)
    monkeypatch.delenv('MMNAS_MHA_STREAM_MINK', raising=False)
    one = run_core(c, p, bwd=False)
    monkeypatch.setenv('MMNAS_MHA_STREAM_MINK', '1')
    st = run_core(c, p)
    e1, e2 = rel_err(one['O'], ref['O']), rel_err(st['O'], ref['O'])
    e12 = rel_err(st['O'], one['O'])
    e_inv = float(np.max(np.abs(st['inv'] - ref['inv']) / ref['inv']))
    e_m = float(np.max(np.abs(st['m'] - ref['m']) / np.maximum(1.0, np.abs(ref['m']))))
    e_inv1 = float(np.max(np.abs(st['inv'] - one['inv']) / np.abs(one['inv'])))
    e_m1 = float(np.max(np.abs(st['m'] - one['m']) / np.maximum(1.0, np.abs(one['m']))))
    print('one-shot %.2e streaming %.2e apart %.2e; 1/l %.2e (%.2e) m %.2e (%.2e)' % (e1, e2, e12, e_inv, e_inv1, e_m, e_m1))
    for k, e in (('one_shot_O', e1), ('stream_O', e2), ('apart_O', e12), ('inv', e_inv), ('m', e_m), ('inv_apart', e_inv1), ('m_apart', e_m1)):
        _note('ab', k, e)
    assert e1 < 1e-5 and e2 < 1e-5
    assert e12 < 2e-5
    assert e_inv <= 1e-5 and e_m <= 1e-5 and e_inv1 <= 1e-5 and e_m1 <= 1e-5
    judge('ab', st, ref)          # the backward read the streaming kernel's statistics


# ------------------------------------------------------------------------------------- 4. strides and purity
@pytest.fixture
def ar():
    yield Arena(DEV)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a fault on the device: nothing more is started on it
        pytest.exit('GPU error in a guard-band case, the session ends here: %s' % e, returncode=3)


@pytest.mark.parametrize('Sq,Sk', [(33, 257), (100, 300)])
def test_strides_and_purity(ar, Sq, Sk):
    """K and V are column slices of ONE wider product (ldk = ldv = 2 di + 8), Q / O rows are padded; the forward may write O and
    the statistics only, the backward dQ, dK, dV, dbiasT and delta only; a second run gives the same bits."""
    L = _L()
    B, H, dh, p = 2, 2, 64, 0.1
    c = inputs(B, H, Sq, Sk, dh, True, True)
    di = H * dh
    ldkv, ldq, ldo = 2 * di + 8, di + 4, di + 12
    ref = reference(c, p)
    kv = np.concatenate([c['K'].reshape(B * Sk, di), c['V'].reshape(B * Sk, di)], 1)
    Qd, _ = ar.inp(c['Q'].reshape(B * Sq, di), ld=ldq, name='Q')
    KVd, _ = ar.inp(kv, ld=ldkv, name='KV')
    m8, _ = ar.inp(c['mask'].astype(np.uint8), name='mask')
    bd, _ = ar.inp(c['biasT'], name='biasT')
    dOd, _ = ar.inp(c['dO'].reshape(B * Sq, di), ld=ldo, name='dO')
    runs = []
    for rep in range(2):
        Od, Ov = ar.out((B * Sq, di), ld=ldo, name='O%d' % rep)
        sd, sv = ar.out((B, H, Sq, 2), name='lse%d' % rep)
        d = L.MhaDesc()
        d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, dh
        d.ldq, d.ldk, d.ldv, d.ldo = ldq, ldkv, ldkv, ldo
        d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = L.fptr(Qd), L.fptr(KVd), L.fptr(KVd[di:]), L.ptr(m8), L.fptr(bd), L.fptr(Od), L.fptr(sd)
        d.drop_p, d.drop_site, d.drop_seed = p, 0, SEED
        L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
        ar.check()
        dQd, dQv = ar.out((B * Sq, di), ld=ldq, name='dQ%d' % rep)
        dKVd, dKVv = ar.out((B * Sk, 2 * di), ld=ldkv, name='dKV%d' % rep)
        dbd, dbv = ar.out((B, H, Sk, Sq), name='dbiasT%d' % rep)
        dl, dlv = ar.out((B, H, Sq), name='delta%d' % rep)
        d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQd), L.fptr(dKVd), L.fptr(dKVd[di:]), L.fptr(dbd), L.fptr(dl)
        L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
        ar.check()
        dKV = dKVv.cpu().numpy()
        runs.append(dict(O=Ov.cpu().numpy().reshape(B, Sq, di), stats=sv.cpu().numpy(), dQ=dQv.cpu().numpy().reshape(B, Sq, di),
                         dK=dKV[:, :di].reshape(B, Sk, di), dV=dKV[:, di:].reshape(B, Sk, di), dbiasT=dbv.cpu().numpy()))
    judge('strided', runs[0], ref)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ------------------------------------------------------------------------------------- 5. operators
OPS = [('rel_self_att_64', dict(B=3, Sx=300, Sy=3, HSIZE=256)), ('guided_att_64', dict(B=3, Sx=33, Sy=257, HSIZE=256)),
       ('uniimg_att_64', dict(B=3, Sx=200, Sy=120, HSIZE=256)), ('self_att_16', dict(B=2, Sx=290, Sy=3, HSIZE=128)),
       ('self_att_256', dict(B=2, Sx=260, Sy=3, HSIZE=256))]


@pytest.mark.parametrize('name,dims', OPS, ids=[n for n, _ in OPS])
def test_operator_vs_oracle(name, dims):
    case = cases.op_case(name, True, True, 1100 + dims['Sx'], dims)
    _check(run_hip_op(case), R.run_oracle_op(case, dtype=torch.float64))


def test_rel_self_att_lazy_relation_form():
    """RelSelfAtt over 300 regions fed the raw relations (RelHandle: the [B, S, S, 64] tensor is never built), against the
    materialised chain in float64 -- test_ops_gpu.py::test_rel_self_att_with_lazy_handle at 300 regions, with that test's own
    assertions: TOL on the output and the input gradient, 3e-3 on the parameter gradients.  (The relation-path gradients are
    1 / r-weighted sums of random sign over B S^2 = 270 000 elements, tests/util.py::KAPPA; measured on an MI355X at this
    shape: linear_r.bias 1.4e-3 of its largest entry, every other key below 1e-3.  The materialised form of the same operator
    is held to _check's 1e-3 on every key in test_operator_vs_oracle.)"""
    from mmnas_amd.model.modules import RelHandle
    from mmnas_amd.utils.ops_adapter import OpsAdapter
    dims = dict(B=3, Sx=300, Sy=3, HSIZE=256)
    case = cases.op_case('rel_self_att_64', True, True, 2025, dims)
    rs = np.random.RandomState(7)
    B, S = dims['B'], dims['Sx']
    raw = rs.standard_normal((B, S, S, 4)).astype(np.float32)
    raw[:, S - 2:] = 0
    raw[:, :, S - 2:] = 0
    Wy = (rs.standard_normal((64, 4)) / 2).astype(np.float32)
    by = (0.1 * rs.standard_normal(64)).astype(np.float32)
    cfg = case['cfg']
    op = OpsAdapter().OPS['rel_self_att_64'](cfg, norm=True, residual=True)
    op.load_state_dict({k: T(v) for k, v in case['P'].items()})
    op = op.to(DEV).train()
    x = T(case['x']).to(DEV).requires_grad_(True)
    Wyd, byd = T(Wy).to(DEV).requires_grad_(True), T(by).to(DEV).requires_grad_(True)
    h = RelHandle(T(raw).to(DEV), Wyd, byd)
    out = op(x, None, T(case['x_mask']).to(DEV), None, h)
    out.backward(T(case['gout']).to(DEV))
    assert h._dense is None
    P = {k: T(v).double().requires_grad_(True) for k, v in case['P'].items()}
    xt, Wyt, byt = T(case['x']).double().requires_grad_(True), T(Wy).double().requires_grad_(True), T(by).double().requires_grad_(True)
    rel = torch.relu(T(raw).double() @ Wyt.t() + byt)
    ref = O.op_forward('rel_self_att_64', P, cfg, xt, None, T(case['x_mask']), None, rel)
    (ref * T(case['gout']).double()).sum().backward()
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= TOL
    assert rel_err(x.grad.cpu().numpy(), xt.grad.numpy()) <= TOL
    assert rel_err(Wyd.grad.cpu().numpy(), Wyt.grad.numpy()) <= 3e-3
    assert rel_err(byd.grad.cpu().numpy(), byt.grad.numpy()) <= 3e-3
    for k, p_ in op.named_parameters():
        e = rel_err(p_.grad.cpu().numpy(), P[k].grad.numpy())
        print(k, '%.2e' % e)
        assert e <= 3e-3, (k, e)


def test_operator_dropout_replay(monkeypatch):
    from mmnas_amd import ops
    seed, p = 0x1234ABCD0F0F0F0F, 0.1
    monkeypatch.setattr(ops, 'next_seed', lambda: seed)
    case = cases.op_case('rel_self_att_64', True, True, 4242, dict(B=3, Sx=300, Sy=3, HSIZE=256))
    got = run_hip_op(case, train=True, drop_p=p)
    case['cfg'].DROPOUT_R = 0.0
    ref = R.run_oracle_op(case, drops=_drop_sites(case, seed, p), dtype=torch.float64)
    _check(got, ref)
    ref0 = R.run_oracle_op(case, dtype=torch.float64)
    assert rel_err(got['out'], ref0['out']) > 1e-2


# ------------------------------------------------------------------------------------- 6. networks
def _init(c):
    return {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}


def _loss(task, pred, target):
    t = T(target).to(DEV)
    if task == 'vqa':
        return torch.nn.functional.binary_cross_entropy_with_logits(pred, t, reduction='sum')
    if task == 'itm':
        return torch.nn.functional.binary_cross_entropy(pred, t, reduction='sum')
    scores, reg = pred
    return (scores * t).sum() + 0.5 * (reg ** 2).sum()


class _Samples(dict):
    """The arrays tests/util.check_grad_samples reads from a golden file, made from an oracle run instead."""
    @property
    def files(self):
        return list(self)


def oracle_net64(c, search=None):
    """The CPU oracle on the case in float64 (the yardstick) and in float32 -> (pred64, loss64, grads64, the sample arrays of
    check_grad_samples).  The relation-path Linears (tests/util.is_rel_path) are watched as tests/golden/make_golden.py's
    capture_rel_linears watches the reference's: their input and the gradient of their output give the cancellation scale
    sum_e |g[e, o] x[e, i]| (weights) / sum_e |g[e, o]| (biases) of every gradient entry."""
    f64 = lambda a: T(a).double() if a.dtype.kind == 'f' else T(a)
    P = {k: f64(v).clone().requires_grad_(True) for k, v in c['P'].items()}
    name_of = {id(v): k for k, v in P.items() if is_rel_path(k) and k.endswith('.weight')}
    seen = {}
    plain = O._linear

    def watched(x, w, b=None):
        y = plain(x, w, b)
        k = name_of.get(id(w))
        if k is not None:
            rec = {'x': x.detach()}
            y.register_hook(lambda gr, rec=rec: rec.__setitem__('g', gr.detach().clone()))
            seen.setdefault(k, []).append(rec)
        return y

    O._linear = watched
    try:
        pred = O.net_forward(c['task'], P, c['cfg'], tuple(f64(a) for a in c['inputs']), genotype=c['genotype'], search=search)
        loss = R.net_loss(c['task'], pred, c['target'].astype(np.float64))
        loss.backward()
    finally:
        O._linear = plain
    g64 = {k: (p.grad.numpy() if p.grad is not None else None) for k, p in P.items()}
    _, _, g32 = R.run_oracle_net(c, search=search)
    keys = sorted(k for k in g64 if g64[k] is not None)
    e64 = lambda a: np.ascontiguousarray(a, dtype=np.float64).reshape(-1)[::max(1, a.size // 64)][:64]
    scales = []
    for k in keys:
        sc = np.zeros(g64[k].shape)
        wk = k.rsplit('.', 1)[0] + '.weight'
        for rec in seen.get(wk, []):
            ga = rec['g'].abs().reshape(-1, rec['g'].shape[-1])
            sc = sc + (ga.t() @ rec['x'].abs().reshape(-1, rec['x'].shape[-1]) if k.endswith('.weight') else ga.sum(0)).numpy()
        scales.append(e64(sc))
    off = np.cumsum([0] + [e64(g64[k]).size for k in keys]).astype(np.int64)
    s = _Samples()
    s['gs_keys'] = s['gs64_keys'] = np.array(keys)
    s['gs_off'] = s['gs64_off'] = off
    s['gs'] = np.concatenate([esample(g32[k] if g32[k] is not None else np.zeros_like(g64[k])) for k in keys])
    s['gs64'] = np.concatenate([e64(g64[k]) for k in keys])
    s['gs64_scale'] = np.concatenate(scales)
    return pred, float(loss.detach()), g64, s


NETS = [('vqa', 'mmnas_vqa'), ('vgd', 'mmnas_vgd'), ('itm', 'mmnas_itm')]


@functools.lru_cache(maxsize=None)
def _net_reference(task, arch):
    c = cases.net_case(task, arch, 20261019, B=3, Sx=6, Sy=300)
    return c, oracle_net64(c)


@pytest.mark.parametrize('chain', ['1', '0'])
@pytest.mark.parametrize('task,arch', NETS)
def test_net_full_300_regions(task, arch, chain, monkeypatch):
    """Predictions, loss and EVERY element of every parameter gradient against the oracle's float64 run, TOL by rel_err.  The
    denominator is floored at 1e-3 of the largest gradient entry of the network -- check_grad_samples' floor for round-off-sized
    gradients, on whole tensors here.  A floor is needed: the reference's own fp32 run is 1e-3 ... 1e-2 of the entry away from
    its float64 run on gradients that are mathematically zero (the bias in front of AttFlat's softmax: 2e-16).  It is the
    network-level one because the last decoder node's query / key projections have gradients of 4e-7 of the network's largest
    entry; an fp32 backward leaves 1e-7 ... 2e-7 of that largest entry on them, whatever forward ran (measured on an MI355X
    at 256 regions: one-shot forward 1.4e-7, streaming forward 1.1e-7; at 300 regions 2.4e-7).
    The relation-path keys are judged as check_grad_samples judges them: the entry's tolerance or KAPPA on its cancellation scale."""
    import importlib
    monkeypatch.setenv('MMNAS_CHAIN', chain)
    Net_Full = importlib.import_module('mmnas.model.full_%s' % task).Net_Full
    c, (rpred, rloss, g64, samples) = _net_reference(task, arch)
    net = Net_Full(c['cfg'], _init(c))
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    net = net.to(DEV).train()
    pred = net(tuple(T(a).to(DEV) for a in c['inputs']))
    if task == 'vgd':
        assert rel_err(pred[0].detach().cpu().numpy(), rpred[0].detach().numpy()) <= TOL
        assert rel_err(pred[1].detach().cpu().numpy(), rpred[1].detach().numpy()) <= TOL
    else:
        assert rel_err(pred.detach().cpu().numpy(), rpred.detach().numpy()) <= TOL
    loss = _loss(task, pred, c['target'])
    assert abs(float(loss.detach()) - rloss) <= TOL * abs(rloss)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in net.named_parameters()}
    gscale = max(float(np.abs(v).max()) for v in g64.values() if v is not None)
    for k, ref in g64.items():
        if ref is None or is_rel_path(k):
            continue
        e = float(np.abs(grads[k].astype(np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-3 * gscale))
        assert e <= TOL, (k, e)
    # the relation-path keys: the entry's tolerance OR KAPPA on its cancellation scale (tests/util.check_grad_samples)
    assert check_grad_samples(samples, '', grads, skip=lambda k: not is_rel_path(k)) >= 2


def test_supernet_step_300_regions():
    """Forward + backward of the VQA supernet under MixedOp.MODE = 'full' (every candidate of every node runs) at 300 regions,
    in the pattern -- and at the bounds -- of test_nets_gpu.py::test_net_search_steps."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas.model.mixed import MixedOp
    seed = 20261020
    c = cases.net_case('vqa', None, seed, search=True, B=2, Sx=5, Sy=300)
    plan = cases.search_plan(np.random.RandomState(seed + 50000), 'full')
    flat = plan['enc'] + plan['dec']
    for k, (act, _) in zip([k for k in c['P'] if k.endswith('alpha_gate')], flat):      # the binary gates of the sampled plan
        c['P'][k][:] = 0
        c['P'][k][act[0]] = 1.0
    rpred, rloss, g64, _ = oracle_net64(c, search=plan)
    net = Net_Search(c['cfg'], _init(c))
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    net = net.to(DEV).train()
    MixedOp.MODE = 'full'
    try:
        net.set_sampled(flat)
        net.unused_modules_off()
        pred = net(tuple(T(a).to(DEV) for a in c['inputs']))
        assert rel_err(pred.detach().cpu().numpy(), rpred.detach().numpy()) <= TOL
        loss = _loss('vqa', pred, c['target'])
        assert abs(float(loss.detach()) - rloss) <= TOL * abs(rloss)
        net.zero_grad()
        loss.backward()
        gate_keys = [k for k in c['P'] if k.endswith('alpha_gate')]
        gg = np.stack([np.pad(m.alpha_gate.grad.cpu().numpy(), (0, 4 - m.n_choices)) for m in net.redundant_modules])
        want = np.stack([np.pad(g64[k], (0, 4 - g64[k].size)) for k in gate_keys])
        assert rel_err(gg, want) <= 3e-3
        net.unused_modules_back()
    finally:
        MixedOp.MODE = None
