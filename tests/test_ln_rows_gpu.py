"""Every hand-written copy of the reference's LayerNorm (rowops / mixed / gemmln / small / vgdhead / retrieval .hip) against the
module's own statement in float64 autograd on the degenerate row classes of tests/ln_rows.py: constant rows (sd == 0), sd at
and far below eps, a large mean, rows of 1e15 and of 1e-12, one outlier per row.  Each fused kernel is steered so that its
pre-LayerNorm row IS the class row exactly (zero product operand, zero added row).  Errors are judged per output and per class;
a failure names the kernel, the class, the output and the row."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dropout_rng
from tests import ln_rows as LR
from tests.golden import cases
from tests.test_ops_gpu import run_hip_op
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T = torch.from_numpy
P_DROP, SEED, SITE = 0.2, 99, 1


def g(a):
    return T(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def _stats_file():
    yield
    LR.write_stats()


class Problems(list):
    """Every class is judged before the test fails, so one run shows all of them."""

    def judge(self, *args, **kw):
        try:
            LR.judge(*args, **kw)
        except AssertionError as e:
            self.append(str(e))

    def check(self, ok, msg):
        if not ok:
            self.append(msg)

    def done(self):
        assert not self, '\n' + '\n'.join(self)


def _ref32(cls, fn):
    return fn(torch.float32) if cls == 'offset' else None


# ---------------------------------------------------------------------------------------------- rowops.hip
def _ln_direct(x, a, b, gy, use_ws, drop):
    from mmnas_amd import _lib as L
    lib = L.lib()
    M, d = x.shape
    xd, ad, bd, gd = g(x), g(a), g(b), g(gy)
    y, dx = torch.empty(M, d, device=DEV), torch.empty(M, d, device=DEV)
    dd = torch.empty(M, d, device=DEV) if drop else None
    dab = torch.zeros(3, d, device=DEV)
    ws = torch.empty(lib.mmnas_layernorm_bwd_ws_floats(M, d), device=DEV) if use_ws else None
    L.check(lib.mmnas_layernorm_fwd(L.fptr(xd), L.fptr(ad), L.fptr(bd), L.fptr(y), M, d, LR.EPS, L.stream()))
    L.check(lib.mmnas_layernorm_bwd(L.fptr(xd), L.fptr(ad), L.fptr(gd), L.fptr(dx), L.fptr(dab[0]), L.fptr(dab[1]), L.fptr(dd),
                                    L.fptr(dab[2]) if drop else None, L.fptr(ws), P_DROP if drop else 0.0, SEED, SITE, M, d, LR.EPS,
                                    L.stream()))
    torch.cuda.synchronize()
    res = {'y': host(y), 'dx': host(dx), 'da': host(dab[0]), 'db': host(dab[1])}
    if drop:
        res['ddrop'], res['dcol'] = host(dd), host(dab[2])
    return res


def _without_drop(ref):
    return None if ref is None else {k: v for k, v in ref.items() if k not in ('ddrop', 'dcol')}


@pytest.mark.parametrize('d', [4, 36, 256, 260, 512, 516, 1024, 1028, 2048])       # the edges of NV = 1 / 2 / 4 / 8
def test_layernorm_kernels_on_every_row_class(d):
    """mmnas_layernorm_fwd / _bwd called directly (column sums by atomics and through the scratch buffer, with and without
    ddrop + dcol at p = 0.2) and through ops.layer_norm."""
    from mmnas_amd import ops
    M = 5
    a, b = LR.params(d)
    gy = LR.grad_out(M, d)
    mask = dropout_rng.scaled_mask(SEED, SITE, (M, d), P_DROP)
    pr = Problems()
    for cls in LR.CLASSES:
        x = LR.rows(cls, M, d)
        ref = LR.ln_reference(x, a, b, gy, mask)
        r32 = _ref32(cls, lambda dt: LR.ln_reference(x, a, b, gy, mask, dtype=dt))
        for use_ws in (False, True):
            for drop in (False, True):
                got = _ln_direct(x, a, b, gy, use_ws, drop)
                pr.judge('rowops.ln', cls, got, ref if drop else _without_drop(ref), r32 if drop else _without_drop(r32),
                         where=' (d=%d, %s, %s)' % (d, 'scratch' if use_ws else 'atomics', 'ddrop+dcol' if drop else 'dx only'))
        xd, ad, bd = (g(v).requires_grad_(True) for v in (x, a, b))
        y = ops.layer_norm(xd, ad, bd)
        y.backward(g(gy))
        got = {'y': host(y), 'dx': host(xd.grad), 'da': host(ad.grad), 'db': host(bd.grad)}
        pr.judge('ops.layer_norm', cls, got, _without_drop(ref), _without_drop(r32), where=' (d=%d)' % d)
    pr.done()


@pytest.mark.parametrize('use_ws', [False, True])
def test_layernorm_bwd_row_loop_with_all_classes_interleaved(use_ws):
    """M = 2053 rows at d = 36: 512 workgroups walk more than one row each (the loop and its clamped prefetch run), the
    classes interleaved row by row.  y / dx / ddrop are judged per class; da / db / dcol sum over every class."""
    M, d = 2053, 36
    x, which = LR.interleaved(M, d)
    a, b = LR.params(d)
    gy = LR.grad_out(M, d)
    mask = dropout_rng.scaled_mask(SEED, SITE, (M, d), P_DROP)
    ref = LR.ln_reference(x, a, b, gy, mask)
    got = _ln_direct(x, a, b, gy, use_ws, True)
    pr = Problems()
    per_row = ('y', 'dx', 'ddrop')
    for k, cls in enumerate(LR.CLASSES):
        sel = which == k
        r32 = _ref32(cls, lambda dt: LR.ln_reference(x[sel], a, b, gy[sel], mask[sel], dtype=dt))
        pr.judge('rowops.ln', cls, {n: got[n][sel] for n in per_row}, {n: ref[n][sel] for n in per_row},
                 None if r32 is None else {n: r32[n] for n in per_row}, where=' (M=2053, d=36, every 8th row)')
    pr.judge('rowops.ln', 'interleaved', got, {n: ref[n] for n in ('da', 'db', 'dcol')}, where=' (M=2053, d=36)')
    pr.done()


@pytest.mark.parametrize('d', [36, 256])
@pytest.mark.parametrize('use_ws', [False, True])
def test_constant_rows_among_ordinary_rows(d, use_ws):
    """Two constant rows among randn rows: their dx and ddrop, and the column sums dcol that a NaN row would poison, are finite
    and within the bar; da / db likewise; the randn rows' dx is what it is without constant neighbours, bit for bit."""
    M = 9
    crow = np.asarray([2, 6])
    x = LR.rows('randn', M, d)
    x[crow] = LR.rows('const', 6, d)[[1, 4]]                     # 2.5 and 1024
    a, b = LR.params(d)
    gy = LR.grad_out(M, d)
    mask = dropout_rng.scaled_mask(SEED, SITE, (M, d), P_DROP)
    ref = LR.ln_reference(x, a, b, gy, mask)
    got = _ln_direct(x, a, b, gy, use_ws, True)
    pr = Problems()
    pr.judge('rowops.ln', 'const', {n: got[n][crow] for n in ('y', 'dx', 'ddrop')}, {n: ref[n][crow] for n in ('y', 'dx', 'ddrop')},
             where=' (d=%d, constant rows 2 and 6 of 9)' % d)
    pr.judge('rowops.ln', 'const+randn', got, {n: ref[n] for n in ('dcol', 'da', 'db')}, where=' (d=%d, constant rows 2 and 6 of 9)' % d)
    other = np.setdiff1d(np.arange(M), crow)
    pr.judge('rowops.ln', 'randn', {n: got[n][other] for n in ('y', 'dx', 'ddrop')}, {n: ref[n][other] for n in ('y', 'dx', 'ddrop')},
             where=' (d=%d, beside constant rows)' % d)
    plain = _ln_direct(LR.rows('randn', M, d), a, b, gy, use_ws, True)
    pr.check(np.array_equal(got['dx'][other], plain['dx'][other]) and np.array_equal(got['ddrop'][other], plain['ddrop'][other]),
             'rowops.ln (d=%d): dx of the randn rows changed with constant rows beside them' % d)
    pr.done()


# ---------------------------------------------------------------------------------------------- mixed.hip
def _node_mix_fwd(zs, las, lbs, gate, M, d):
    """mmnas_node_mix_fwd on device tensors (None: a candidate that is not evaluated / has no LayerNorm)."""
    from mmnas_amd import _lib as L
    n = len(zs)
    arr = lambda ts: (C.c_void_p * n)(*[L.fptr(t) for t in ts])
    out = torch.empty(M, d, device=DEV)
    L.check(L.lib().mmnas_node_mix_fwd(arr(zs), arr(las), arr(lbs), n, L.fptr(gate), L.fptr(out), M, d, LR.EPS, L.stream()))
    return out


def _node_mix(x, z0, a, b, gate, dout):
    """mmnas_node_mix_fwd / _bwd: candidates (plain z0, not evaluated, active with LayerNorm on rows x)."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    M, d = x.shape
    n, active = 3, 2
    arr = lambda ts: (C.c_void_p * n)(*[L.fptr(t) for t in ts])
    zs, las, lbs = [g(z0), None, g(x)], [None, None, g(a)], [None, None, g(b)]
    gd, dd = g(gate), g(dout)
    dact = torch.empty(M, d, device=DEV)
    dgate = torch.full((n,), 0.25, device=DEV)
    ws = torch.empty(lib.mmnas_mixed_sum_ws_floats(), device=DEV)
    out = _node_mix_fwd(zs, las, lbs, gd, M, d)
    L.check(lib.mmnas_node_mix_bwd(arr(zs), arr(las), arr(lbs), n, L.fptr(gd), L.fptr(dd), L.fptr(dact), active, L.fptr(dgate),
                                   L.fptr(ws), M, d, LR.EPS, L.stream()))
    torch.cuda.synchronize()
    return {'out': host(out), 'dgate': host(dgate), 'd_active': host(dact)}


@pytest.mark.parametrize('d', [36, 256, 512, 1024])
def test_node_mix_on_every_row_class(d):
    """mmnas_node_mix_fwd / _bwd with three candidates: one without LayerNorm parameters, one not evaluated (NULL) and the
    active one, whose pre-LayerNorm rows are the class rows.  (This entry point returns d_active = gate[active] * dout; the
    sampled candidate's LayerNorm backward inside the kernel has its own tests below.)"""
    M, n, active = 6, 3, 2
    rs = np.random.RandomState(d)
    z0 = (1.5 * rs.standard_normal((M, d)) + 0.3).astype(np.float32)
    gate = rs.standard_normal(n).astype(np.float32)
    dout = LR.grad_out(M, d, 1)
    a, b = LR.params(d)

    def reference(x, dt):
        X, Z0, A, B, G, D = (T(v).to(dt) for v in (x, z0, a, b, gate, dout))
        o2 = LR.module_ln(X, A, B)
        dgate = torch.stack([(D * Z0).sum(), torch.zeros((), dtype=dt), (D * o2).sum()]) + 0.25
        return {k: v.double().numpy() for k, v in (('out', G[0] * Z0 + G[2] * o2), ('dgate', dgate), ('d_active', G[active] * D))}

    pr = Problems()
    for cls in LR.CLASSES:
        x = LR.rows(cls, M, d)
        got = _node_mix(x, z0, a, b, gate, dout)
        pr.judge('mixed.node_mix', cls, got, reference(x, torch.float64), _ref32(cls, lambda dt: reference(x, dt)), where=' (d=%d)' % d)
        pr.check(got['dgate'][1] == 0.25, 'mixed.node_mix (d=%d): the gate gradient of a candidate that was not evaluated moved' % d)
    pr.done()


def _node_mix_fused(x, z0, a, b, gate, dout, drop):
    """mmnas_node_mix_bwd_ln: candidates (plain z0, not evaluated, active with LayerNorm on rows x)."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    M, d = x.shape
    n, active = 3, 2
    arr = lambda ts: (C.c_void_p * n)(*[L.fptr(t) for t in ts])
    zs, las, lbs = [g(z0), None, g(x)], [None, None, g(a)], [None, None, g(b)]
    gd, dd = g(gate), g(dout)
    dz = torch.full((M, d), float('nan'), device=DEV)
    dt = torch.full((M, d), float('nan'), device=DEV) if drop else None
    dab = torch.zeros(3, d, device=DEV)
    dgate = torch.full((n,), 0.25, device=DEV)
    ws = torch.empty(lib.mmnas_mixed_sum_ws_floats(), device=DEV)
    lnws = torch.empty(lib.mmnas_layernorm_bwd_ws_floats(M, d), device=DEV)
    L.check(lib.mmnas_node_mix_bwd_ln(arr(zs), arr(las), arr(lbs), n, L.fptr(gd), L.fptr(dd), active, L.fptr(dgate), L.fptr(ws), L.fptr(dz),
                                      L.fptr(dt), L.fptr(dab[0]), L.fptr(dab[1]), L.fptr(dab[2]) if drop else None, L.fptr(lnws),
                                      P_DROP if drop else 0.0, SEED, SITE, M, d, LR.EPS, L.stream()))
    torch.cuda.synchronize()
    res = {'dgate': host(dgate), 'dx': host(dz), 'da': host(dab[0]), 'db': host(dab[1])}
    if drop:
        res['ddrop'], res['dcol'] = host(dt), host(dab[2])
    return res


def _node_mix_fused_reference(x, z0, a, b, gate, dout, mask, dt):
    """dz / dt / da / db / dcol: the module's backward under the gradient gate[active] * dout; dgate as in node_mix."""
    ref = LR.ln_reference(x, a, b, gate[2].astype(np.float64) * dout.astype(np.float64), mask, dtype=dt)
    del ref['y']
    D = T(dout).to(dt)
    o2 = LR.module_ln(T(x).to(dt), T(a).to(dt), T(b).to(dt))
    ref['dgate'] = (torch.stack([(D * T(z0).to(dt)).sum(), torch.zeros((), dtype=dt), (D * o2).sum()]) + 0.25).double().numpy()
    return ref


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('d', [36, 256])
def test_node_mix_fused_layernorm_backward_on_every_row_class(d, drop):
    """The sampled candidate's LayerNorm backward inside the node kernel (node_mix_bwd_kernel<1, true>, what the mixed chain
    runs), through mmnas_node_mix_bwd_ln: dz, dt behind the dropout replay, the LayerNorm parameter gradients and the column
    sums of dt, per class; dz starts as NaN, so a launch that skipped the fused path cannot pass."""
    M = 6
    rs = np.random.RandomState(d + 1)
    z0 = (1.5 * rs.standard_normal((M, d)) + 0.3).astype(np.float32)
    gate = rs.standard_normal(3).astype(np.float32)
    dout = LR.grad_out(M, d, 2)
    a, b = LR.params(d)
    mask = dropout_rng.scaled_mask(SEED, SITE, (M, d), P_DROP) if drop else None
    pr = Problems()
    for cls in LR.CLASSES:
        x = LR.rows(cls, M, d)
        got = _node_mix_fused(x, z0, a, b, gate, dout, drop)
        pr.judge('mixed.node_mix_ln', cls, got, _node_mix_fused_reference(x, z0, a, b, gate, dout, mask, torch.float64),
                 _ref32(cls, lambda dt: _node_mix_fused_reference(x, z0, a, b, gate, dout, mask, dt)),
                 where=' (d=%d, %s)' % (d, 'dt+dcol' if drop else 'dz only'))
    pr.done()


@pytest.mark.parametrize('d', [36, 256])
def test_node_mix_fused_constant_rows_among_ordinary_rows(d):
    """As test_constant_rows_among_ordinary_rows, for the LayerNorm backward inside the node kernel."""
    M = 9
    crow = np.asarray([2, 6])
    x = LR.rows('randn', M, d)
    x[crow] = LR.rows('const', 6, d)[[1, 4]]
    rs = np.random.RandomState(d + 2)
    z0 = (1.5 * rs.standard_normal((M, d)) + 0.3).astype(np.float32)
    gate = rs.standard_normal(3).astype(np.float32)
    dout = LR.grad_out(M, d, 3)
    a, b = LR.params(d)
    mask = dropout_rng.scaled_mask(SEED, SITE, (M, d), P_DROP)
    ref = _node_mix_fused_reference(x, z0, a, b, gate, dout, mask, torch.float64)
    got = _node_mix_fused(x, z0, a, b, gate, dout, True)
    where = ' (d=%d, constant rows 2 and 6 of 9)' % d
    pr = Problems()
    pr.judge('mixed.node_mix_ln', 'const', {n: got[n][crow] for n in ('dx', 'ddrop')}, {n: ref[n][crow] for n in ('dx', 'ddrop')}, where=where)
    pr.judge('mixed.node_mix_ln', 'const+randn', got, {n: ref[n] for n in ('dcol', 'da', 'db', 'dgate')}, where=where)
    other = np.setdiff1d(np.arange(M), crow)
    pr.judge('mixed.node_mix_ln', 'randn', {n: got[n][other] for n in ('dx', 'ddrop')}, {n: ref[n][other] for n in ('dx', 'ddrop')},
             where=' (d=%d, beside constant rows)' % d)
    plain = _node_mix_fused(LR.rows('randn', M, d), z0, a, b, gate, dout, True)
    pr.check(np.array_equal(got['dx'][other], plain['dx'][other]) and np.array_equal(got['ddrop'][other], plain['ddrop'][other]),
             'mixed.node_mix_ln (d=%d): dz of the randn rows changed with constant rows beside them' % d)
    pr.done()


# ---- two copies of the forward against each other
@pytest.mark.parametrize('d', [36, 256, 512, 1024])
def test_node_mix_forward_of_one_candidate_is_layernorm_forward_bit_for_bit(d):
    """mmnas_node_mix_fwd with one LayerNorm candidate under gate 1.0 (out = 0 + 1 * LN(x)) against mmnas_layernorm_fwd: the
    same bits on every class at M = 5.  (At d <= 256 the two kernels are compiled to round different products of
    x * x + y * y -- csrc/ln_rows.h -- which these rows do not show; 2053 interleaved rows at d = 36 do.  The backward twin of
    this test, mmnas_node_mix_bwd_ln under gate 1.0 against mmnas_layernorm_bwd, does not hold: dz differs from dx in the last
    bit on 12 to 27 % of the elements, profiles/r16_ln_rows_bits.txt.)"""
    M = 5
    a, b = LR.params(d)
    gy = LR.grad_out(M, d)
    pr = Problems()
    for cls in LR.CLASSES:
        x = LR.rows(cls, M, d)
        out = host(_node_mix_fwd([g(x)], [g(a)], [g(b)], g(np.ones(1)), M, d))
        y = _ln_direct(x, a, b, gy, True, False)['y']
        pr.check(np.array_equal(out, y), 'node_mix_fwd (d=%d) on class %s: %d of %d elements differ from layernorm_fwd'
                 % (d, cls, int((out != y).sum()), y.size))
    pr.done()


# ---------------------------------------------------------------------------------------------- gemmln.hip
def _gemm_ln(L, ops, A, W, R, la, lb, M, K, panel, want_z=True):
    N = 256
    z = torch.full((M, N), float('nan'), device=DEV)
    y = torch.full((M, N), float('nan'), device=DEV)
    d = ops.gemm_desc(L.GEMM_NT, [dict(M=M, A=[A], B=[W], C=z, residual=R)], N, K, K, K, N, ldres=N)
    if not want_z:
        d.g[0].C = None                      # (only the panel kernel runs without z: the two-launch form refuses)
    old = L.lib().mmnas_set_gemm_ln(1 if panel else 0)
    try:
        L.check(L.lib().mmnas_gemm_ln(C.byref(d), L.fptr(la), L.fptr(lb), L.fptr(y), LR.EPS, L.stream()))
        torch.cuda.synchronize()
    finally:
        L.lib().mmnas_set_gemm_ln(old)
    return z, y


@pytest.mark.parametrize('K', [32, 64])
def test_gemm_ln_on_every_row_class(K):
    """mmnas_gemm_ln at N = 256, M = 2048 (the default row threshold of the panel kernel).  The class rows are residual rows
    under a zero row of A and no bias, so z = residual exactly; the other rows carry a random product.  K = 64 is the smallest
    K the row-panel kernel takes (two K-tiles of 32 in flight) -- a call without z, which the two-launch form refuses, proves it
    ran; K = 32 goes through the same entry point in its two-launch form.  z is compared bit for bit on the class rows only
    (there it is the residual row in both forms); on the rows with a product the two forms accumulate in different orders and
    agree to 2e-5, as tests/test_gemm_ln_gpu.py holds them."""
    from mmnas_amd import _lib as L, ops
    M, N, R = 2048, 256, 6
    rs = np.random.RandomState(K)
    nc = R * len(LR.CLASSES)
    A = rs.standard_normal((M, K)).astype(np.float32)
    A[:nc] = 0
    res = rs.standard_normal((M, N)).astype(np.float32)
    for k, cls in enumerate(LR.CLASSES):
        res[k * R:(k + 1) * R] = LR.rows(cls, R, N)
    W = (rs.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    la, lb = LR.params(N)
    Ad, Wd, Rd, lad, lbd = g(A), g(W), g(res), g(la), g(lb)
    z, y = _gemm_ln(L, ops, Ad, Wd, Rd, lad, lbd, M, K, panel=True)
    z2, y2 = _gemm_ln(L, ops, Ad, Wd, Rd, lad, lbd, M, K, panel=False)
    if K >= 64:
        _, y3 = _gemm_ln(L, ops, Ad, Wd, Rd, lad, lbd, M, K, panel=True, want_z=False)
        assert torch.equal(y3, y)
    pr = Problems()
    # z of the class rows: the residual itself, in both forms, bit for bit
    pr.check(torch.equal(z[:nc], Rd[:nc]) and torch.equal(z2[:nc], Rd[:nc]), 'gemmln (K=%d): z of a zero product row is not its residual row' % K)
    gemm_ln_y, two_y = host(y), host(y2)
    dummy_g = np.zeros((R, N), np.float32)
    for k, cls in enumerate(LR.CLASSES):
        sl = slice(k * R, (k + 1) * R)
        ref = {'y': LR.ln_reference(res[sl], la, lb, dummy_g)['y']}
        r32 = _ref32(cls, lambda dt: {'y': LR.ln_reference(res[sl], la, lb, dummy_g, dtype=dt)['y']})
        pr.judge('gemmln.panel' if K >= 64 else 'gemmln.two_launch', cls, {'y': gemm_ln_y[sl]}, ref, r32, where=' (K=%d)' % K)
        pr.judge('gemmln.two_launch', cls, {'y': two_y[sl]}, ref, r32, where=' (K=%d, switch off)' % K)
    # the rows with a product: as tests/test_gemm_ln_gpu.py holds them
    t = T(A[nc:]).double() @ T(W).double().t() + T(res[nc:]).double()
    yr = LR.module_ln(t, T(la).double(), T(lb).double()).numpy()
    pr.check(rel_err(host(z[nc:]), t.numpy()) < 2e-5 and rel_err(gemm_ln_y[nc:], yr) < 2e-5 and rel_err(host(z[nc:]), host(z2[nc:])) < 2e-5,
             'gemmln (K=%d): rows with a product' % K)
    pr.done()


# ---------------------------------------------------------------------------------------------- small.hip
@pytest.fixture
def small_ops():
    from mmnas_amd import _lib as L
    lib = L.lib()
    prev = lib.mmnas_set_small_ops(1), lib.mmnas_set_small_bwd(1), lib.mmnas_set_small_ffn(1)
    yield lib
    lib.mmnas_set_small_ops(prev[0])
    lib.mmnas_set_small_bwd(prev[1])
    lib.mmnas_set_small_ffn(prev[2])


def _run_counted(lib, case):
    """run_hip_op and the number of launches of the one-launch kernel class (tests/test_small_gpu.py)."""
    from mmnas_amd import _lib as L
    arr = (L.ProfStat * len(L.K_NAMES))()
    L.check(lib.mmnas_prof_enable(1))
    try:
        got = run_hip_op(case)
        torch.cuda.synchronize()
        L.check(lib.mmnas_prof_collect(arr))
    finally:
        L.check(lib.mmnas_prof_enable(0))
    return got, arr[L.K_NAMES.index('small_ops')].launches


SMALL_DIMS = dict(B=3, Sx=14, Sy=3, HSIZE=256)


def _small_reference(case, dt, att_of):
    """out = LN(x + att W^T + bias) with W = 0 and bias = 0 given as parameters: z = x, and the gradient of W is fed by dt."""
    P = {k: T(v).to(dt).requires_grad_(True) for k, v in case['P'].items()}
    X = T(case['x']).to(dt).requires_grad_(True)
    att, W, bias = att_of(X, P)
    z = X + att @ W.t() + (bias if bias is not None else 0)
    out = LR.module_ln(z, P['ln.a_2'], P['ln.b_2'])
    out.backward(T(case['gout']).to(dt))
    res = {'out': out.detach(), 'dx': X.grad}
    for k, p in P.items():
        res['g:' + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return {k: v.double().numpy() for k, v in res.items()}


def _short_self_att_case(cls):
    case = cases.op_case('self_att_64', True, True, 11, SMALL_DIMS)
    case['x'] = LR.rows(cls, 42, 256).reshape(3, 14, 256)
    case['x_mask'][...] = False
    case['P']['mhatt.linear_merge.weight'][...] = 0
    case['P']['mhatt.linear_q.weight'][...] = 0
    return case


def test_short_self_attention_on_every_row_class(small_ops):
    """The one-launch SelfAtt forward and backward (Sx = 14, HSIZE = 256, B = 3, no dropout, no padding) with the merge weight
    zero: z = x, x carries the class.  The query weight is zero as well, so the attention is uniform and the merge-weight
    gradient dt^T att is well conditioned on every class (att = the sample's mean value row)."""
    pr = Problems()
    for cls in LR.CLASSES:
        case = _short_self_att_case(cls)
        got, launches = _run_counted(small_ops, case)
        pr.check(launches == 2, 'small.self_att: %d one-launch kernels ran, not forward + backward' % launches)

        def att_of(X, P):
            V = X @ P['mhatt.linear_v.weight'].t()
            return V.mean(1, keepdim=True).expand_as(V), P['mhatt.linear_merge.weight'], None
        ref = _small_reference(case, torch.float64, att_of)
        pr.judge('small.self_att', cls, got, ref, _ref32(cls, lambda dt: _small_reference(case, dt, att_of)))
    pr.done()


@pytest.mark.parametrize('mode', [1, 2])
def test_short_feed_forward_on_every_row_class(mode, small_ops):
    """The one-launch FeedForward forward (MMNAS_SMALL_FFN modes 1 and 2) with the last layer's weight and bias zero: z = x."""
    small_ops.mmnas_set_small_ffn(mode)
    pr = Problems()
    for cls in LR.CLASSES:
        case = cases.op_case('feed_forward', True, True, 12, SMALL_DIMS)
        case['x'] = LR.rows(cls, 42, 256).reshape(3, 14, 256)
        case['P']['mlp.linear.weight'][...] = 0
        case['P']['mlp.linear.bias'][...] = 0
        got, launches = _run_counted(small_ops, case)
        pr.check(launches == 1, 'small.ffn: %d one-launch kernels ran, not the forward' % launches)

        def att_of(X, P):
            h = torch.relu(X @ P['mlp.fc.linear.weight'].t() + P['mlp.fc.linear.bias'])
            return h, P['mlp.linear.weight'], P['mlp.linear.bias']
        ref = _small_reference(case, torch.float64, att_of)
        pr.judge('small.ffn', cls, got, ref, _ref32(cls, lambda dt: _small_reference(case, dt, att_of)), where=' (mode %d)' % mode)
    pr.done()


# ---------------------------------------------------------------------------------------------- vgdhead.hip
VGD_B, VGD_S = 2, 5


def _grounding_head_case(F):
    B, S = VGD_B, VGD_S
    rs = np.random.RandomState(F)
    a, b = LR.params(F)
    Ws, bs = (rs.standard_normal((1, F)) / np.sqrt(F)).astype(np.float32), rs.standard_normal(1).astype(np.float32)
    Wr, br = (rs.standard_normal((4, F)) / np.sqrt(F)).astype(np.float32), rs.standard_normal(4).astype(np.float32)
    dsc, dreg = rs.standard_normal((B, S)).astype(np.float32), rs.standard_normal((B, S, 4)).astype(np.float32)
    return a, b, Ws, bs, Wr, br, dsc, dreg


def _grounding_head_run(F, logsm, yf, to, head):
    """scores, reg and every gradient of `head` on yf (xp = 0) under the case's output gradients, as float64 arrays."""
    a, b, Ws, bs, Wr, br, dsc, dreg = _grounding_head_case(F)
    names = ('dyf', 'dxp', 'da', 'db', 'dWs', 'dbs', 'dWr', 'dbr')
    ts = [to(v).requires_grad_(True) for v in (yf, np.zeros((VGD_B, F), np.float32), a, b, Ws, bs, Wr, br)]
    scores, reg = head(ts[0], ts[1], ts[2], ts[3], LR.EPS, *ts[4:], logsm)
    ((scores * to(dsc)).sum() + (reg * to(dreg)).sum()).backward()
    res = {'scores': scores, 'reg': reg}
    res.update({n: t.grad for n, t in zip(names, ts)})
    return {k: v.detach().double().cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize('F,logsm', [(8, True), (256, False), (512, True), (1024, False), (2048, True)])   # the smallest F; NV = 1 / 2 / 4 / 8
def test_grounding_head_on_every_row_class(F, logsm, monkeypatch):
    """ops.grounding_head (one launch per direction) with xp = 0 and yf carrying the class rows, against the torch
    composition of the reference's statements in float64."""
    from mmnas_amd import ops
    B, S = VGD_B, VGD_S
    a, b, Ws, bs, Wr, br, dsc, dreg = _grounding_head_case(F)

    def run(yf, to, head):
        return _grounding_head_run(F, logsm, yf, to, head)

    native = []
    orig = ops.GroundingHeadFn.apply
    monkeypatch.setattr(ops.GroundingHeadFn, 'apply', lambda *args: (native.append(1), orig(*args))[1])
    prev = ops.set_vgd_head(True)
    pr = Problems()
    try:
        for cls in LR.CLASSES:
            yf = LR.rows(cls, B * S, F).reshape(B, S, F)
            got = run(yf, g, ops.grounding_head)
            ref = run(yf, lambda v: T(v).double(), ops._grounding_head_torch)
            r32 = _ref32(cls, lambda dt: run(yf, lambda v: T(v).to(dt), ops._grounding_head_torch))
            floors = None
            if logsm:
                # behind log_softmax the score gradients ds = dscores - softmax * sum(dscores) add up to 0 over a sample, so
                # dbs = sum ds is 0 on every class; dWs = sum ds * (normalised row) cancels the same way where the normalised rows
                # agree (constant rows, sd << eps).  A sum that cancels is judged against the sum of its terms' magnitudes.
                ds = np.abs(dsc - np.exp(ref['scores']) * dsc.sum(-1, keepdims=True))
                floors = {'dbs': float(ds.sum())}
                if cls in ('const', 'sd_tiny', 'small'):
                    n = np.abs(LR.module_ln(T(yf).double(), T(a).double(), T(b).double()).numpy()).max(-1)
                    floors['dWs'] = float((ds * n).sum())
            pr.judge('vgdhead', cls, got, ref, r32, where=' (F=%d, %s)' % (F, 'log_softmax' if logsm else 'raw scores'), floors=floors)
    finally:
        ops.set_vgd_head(prev)
    pr.check(len(native) == len(LR.CLASSES), 'vgdhead (F=%d): the native head ran %d times for %d classes' % (F, len(native), len(LR.CLASSES)))
    pr.done()


# ---------------------------------------------------------------------------------------------- retrieval.hip
@pytest.mark.parametrize('D', [36, 256, 2048])
def test_itm_pair_head_on_every_row_class(D):
    """mmnas_itm_pair_head (forward only): xflat rows are zero, yflat carries the class rows."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    P = 6
    rs = np.random.RandomState(D)
    a, b = LR.params(D)
    Wp, bp = (rs.standard_normal(D) / np.sqrt(D)).astype(np.float32), rs.standard_normal(1).astype(np.float32)
    xflat = torch.zeros(2, D, device=DEV)
    idx = T(np.asarray([0, 1, 1, 0, 1, 0], np.int32)).to(DEV)
    ad, bd, Wd, bpd = g(a), g(b), g(Wp), g(bp)

    def reference(x, dt):
        logit = LR.module_ln(T(x).to(dt), T(a).to(dt), T(b).to(dt)) @ T(Wp).to(dt) + T(bp).to(dt)
        return {'logits': logit.double().numpy(), 'scores': torch.sigmoid(logit).double().numpy()}

    pr = Problems()
    for cls in LR.CLASSES:
        x = LR.rows(cls, P, D)
        yd = g(x)
        logits, scores = torch.empty(P, device=DEV), torch.empty(P, device=DEV)
        L.check(lib.mmnas_itm_pair_head(L.fptr(xflat), L.ptr(idx), L.fptr(yd), L.fptr(ad), L.fptr(bd), L.fptr(Wd), L.fptr(bpd),
                                        L.fptr(logits), L.fptr(scores), None, None, 0, P, D, LR.EPS, L.stream()))
        torch.cuda.synchronize()
        pr.judge('retrieval.pair_head', cls, {'logits': host(logits), 'scores': host(scores)}, reference(x, torch.float64),
                 _ref32(cls, lambda dt: reference(x, dt)), where=' (D=%d)' % D)
    pr.done()
