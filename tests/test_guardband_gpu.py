"""Guard-band tests (GPU): every kernel of the direct ABI is handed pointers carved out of a tests/guardband.py `Arena` -- each
tensor between two 4 KiB bands of a NaN pattern (zeros around index tables and masks), strided operands with poisoned row gaps,
every `*_ws_floats()` scratch at exactly its advertised size -- and after the call `arena.check()` proves that every band, gap
and input is bitwise intact and every output element was written and is finite.  The float64 comparison of the kernel's
existing test follows, at that test's tolerance (references: tests/kernel_refs.py).

Shapes are the smallest that reach each edge: one element, ragged tails of the 32 / 64 / 128 tiles, odd K, more than one
block, the grid cap of the element-wise launches.  Where a `*_supported()` call or a documented limit refuses a shape of the
table the nearest accepted one is taken and the table says so."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.gemm_knobs import gemm_knobs
from tests.guardband import Arena, GuardBandError
from tests.kernel_refs import (attflat_pool_ref, eltwise_ref, gemm_epilogue_ref, gemm_ref, glu_ref, layer_norm_bwd_ref,
                               layer_norm_ref, mha_ref, rel_bias_ref, rel_fused_ref, rel_multi_pre, rel_multi_ref)
from tests.util import TOL, rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# The row-panel kernel of mmnas_gemm_ln takes products of >= MMNAS_GEMM_LN_MINM rows (default 2048) and K <= MMNAS_GEMM_LN_MAXK
# (256); the library reads both once.  As tests/test_gemm_ln_gpu.py does: every row count and K, set before the first read.
os.environ.setdefault('MMNAS_GEMM_LN_MINM', '0')
os.environ.setdefault('MMNAS_GEMM_LN_MAXK', '65536')
PAD = 4          # every leading dimension of a strided case is the row width + PAD floats


def _L():
    import mmnas_amd._lib as L
    return L


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def cpu(view):
    return view.cpu().numpy()


@pytest.fixture
def gemm_tuning():
    yield from gemm_knobs()


@pytest.fixture
def ar():
    yield Arena(DEV)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a fault on the device: nothing more is started on it
        pytest.exit('GPU error in a guard-band case, the session ends here: %s' % e, returncode=3)


def zeros(*shape):
    return np.zeros(shape, np.float32)


# ----------------------------------------------------------------------------- end-to-end detection
def test_a_kernel_told_one_row_too_many_is_caught(ar):
    """LayerNorm forward is told M + 1 rows while y was carved for M: the extra row stays inside the arena's allocation and
    lands in y's trailing band -- check() must name y and the first byte behind its payload."""
    L = _L()
    rs = np.random.RandomState(0)
    M, d = 5, 36
    (x, _), (a, _), (b, _) = ar.inp(rnd(rs, M + 1, d), name='x'), ar.inp(1 + 0.1 * rnd(rs, d), name='a'), ar.inp(rnd(rs, d), name='b')
    y, _ = ar.out((M, d), name='y')
    L.check(L.lib().mmnas_layernorm_fwd(L.fptr(x), L.fptr(a), L.fptr(b), L.fptr(y), M + 1, d, 1e-6, L.stream()))
    with pytest.raises(GuardBandError) as e:
        ar.check()
    assert str(e.value).startswith('y: trailing band overwritten at payload byte offset %d ' % (M * d * 4)), str(e.value)


# ----------------------------------------------------------------------------- GEMM
LAYOUTS = {'NT': 0, 'NN': 1, 'TN': 2}


def _operand_shapes(layout, M, N, K):
    return {'NT': ((M, K), (N, K)), 'NN': ((M, K), (K, N)), 'TN': ((K, M), (K, N))}[layout]


def _gemm(ar, rs, layout, Ms, N, K, nseg=1, bias=False, relu=False, drop=None, gate=False, residual=False, colsum=False,
          accumulate=False, planes=False, pad=PAD, ldb_pad=None, tol=1e-5):
    """One mmnas_gemm call with every operand strided (ld = width + pad), checked: bands, gaps, inputs, outputs, float64."""
    L = _L()
    from oracle import dropout_rng
    ldb_pad = pad if ldb_pad is None else ldb_pad
    d = L.GemmDesc()
    d.layout, d.ngroups, d.nseg, d.N, d.K = LAYOUTS[layout], len(Ms), nseg, N, K
    d.relu, d.split_k, d.alpha, d.gate_scale, d.accumulate, d.b_planes = int(relu), 1, 1.0, 1.25 if gate else 1.0, int(accumulate), int(planes)
    if drop is not None:
        d.drop_p, d.drop_seed, d.drop_site = drop
    d.ldc, d.ldres, d.ldgate = N + pad, (N + pad) if residual else 0, (N + pad) if gate else 0
    groups = []
    d.lda = max(_operand_shapes(layout, M, N, K)[0][1] for M in Ms) + pad      # (TN: A is [K, M] -- the widest group's M)
    d.ldb = _operand_shapes(layout, Ms[0], N, K)[1][1] + ldb_pad
    for gi, M in enumerate(Ms):
        sa, sb = _operand_shapes(layout, M, N, K)
        g = dict(M=M, A=[rnd(rs, *sa) for _ in range(nseg)], B=[rnd(rs, *sb) for _ in range(nseg)])
        g['Ad'] = [ar.inp(a, ld=d.lda, name='A%d.%d' % (gi, s))[0] for s, a in enumerate(g['A'])]
        if planes:
            # mmnas_split_planes over the strided matrix as one flat array of N * ldb floats (gap columns included: they hold
            # the pattern and split into NaN planes nobody may read)
            g['Bd'] = []
            for s, bm in enumerate(g['B']):
                full = np.full((sb[0], d.ldb), np.nan, np.float32)
                full[:, :sb[1]] = bm
                wf, _ = ar.inp(full, name='W%d.%d' % (gi, s))
                pl, _ = ar.inout(np.zeros(3 * full.size // 2, np.float32), name='planes%d.%d' % (gi, s))    # 3 n bf16 = 6 n bytes
                L.check(L.lib().mmnas_split_planes(L.fptr(wf), L.ptr(pl), full.size, L.stream()))
                g['Bd'].append(pl)
                p3 = pl.view(torch.bfloat16).view(3, sb[0], d.ldb)[:, :, :sb[1]].double().sum(0).cpu()
                assert torch.equal(p3, torch.from_numpy(bm).double()), 'the three planes do not sum back to the matrix'
        else:
            g['Bd'] = [ar.inp(b, ld=d.ldb, name='B%d.%d' % (gi, s))[0] for s, b in enumerate(g['B'])]
        if accumulate:
            g['C0'] = rnd(rs, M, N)
            g['Cd'], g['Cv'] = ar.inout(g['C0'], ld=d.ldc, name='C%d' % gi)
        else:
            g['Cd'], g['Cv'] = ar.out((M, N), ld=d.ldc, name='C%d' % gi)
        gg = d.g[gi]
        gg.M = M
        for s in range(nseg):
            gg.A[s], gg.B[s] = L.fptr(g['Ad'][s]), L.ptr(g['Bd'][s])
        gg.C = L.fptr(g['Cd'])
        if bias:
            g['bias'] = rnd(rs, N)
            g['biasd'] = ar.inp(g['bias'], name='bias%d' % gi)[0]
            gg.bias = L.fptr(g['biasd'])
        if residual:
            g['res'] = rnd(rs, M, N)
            g['resd'] = ar.inp(g['res'], ld=d.ldres, name='res%d' % gi)[0]
            gg.residual = L.fptr(g['resd'])
        if gate:
            g['gate'] = (rnd(rs, M, N) > 0).astype(np.float32)
            g['gated'] = ar.inp(g['gate'], ld=d.ldgate, name='gate%d' % gi)[0]
            gg.gate = L.fptr(g['gated'])
        if colsum:
            g['cs0'] = rnd(rs, N)
            g['csd'], g['csv'] = ar.inout(g['cs0'], name='colsum%d' % gi)
            gg.colsum = L.fptr(g['csd'])
        groups.append(g)
    L.check(L.lib().mmnas_gemm(C.byref(d), L.stream()))
    ar.check()
    for gi, g in enumerate(groups):
        M = g['M']
        acc = sum(gemm_ref(layout, a, b) for a, b in zip(g['A'], g['B']))
        dm = dropout_rng.scaled_mask(drop[1], drop[2], (M, N), drop[0]) if drop is not None else None
        ref = gemm_epilogue_ref(acc, g.get('bias'), relu, dm, g.get('gate'), 1.25, g.get('res'))
        if accumulate:
            ref = ref + torch.from_numpy(g['C0']).double()
        err = rel_err(cpu(g['Cv']), ref.numpy())
        assert err < tol, (gi, err)
        if colsum:
            want = torch.from_numpy(g['cs0']).double() + ref.sum(0)
            assert rel_err(cpu(g['csv']), want.numpy()) < 2e-5, gi       # (test_gemm_colsum_epilogue's bound)
    return groups


SHAPES = [(1, 4, 4), (63, 68, 36), (65, 132, 33), (129, 64, 64), (300, 192, 160)]      # (65, 132, 33): the odd-K generic path


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('M,N,K', SHAPES)
@pytest.mark.parametrize('tile', [0, 64, 128])
@pytest.mark.parametrize('mode', [6, 0])
def test_gemm_plain(ar, gemm_tuning, layout, M, N, K, tile, mode):
    """lda, ldb, ldc = width + 4.  (K = 33: the leading dimension K + 4 = 37 is odd too -- scalar guarded loads throughout.)"""
    gemm_tuning(tile=tile or None, split=mode)
    _gemm(ar, np.random.RandomState(M * 7 + N * 3 + K), layout, [M], N, K)


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('M,N,K', [(63, 68, 36), (65, 132, 33), (300, 192, 160)])
@pytest.mark.parametrize('tile', [0, 64, 128])
@pytest.mark.parametrize('mode', [6, 0])
def test_gemm_full_epilogue(ar, gemm_tuning, layout, M, N, K, tile, mode):
    """bias + relu + dropout + gate + residual; ldres = ldgate = N + 4."""
    gemm_tuning(tile=tile or None, split=mode)
    _gemm(ar, np.random.RandomState(M + N + K), layout, [M], N, K, bias=True, relu=True, drop=(0.25, 12345678901234, 1), gate=True,
          residual=True)


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('M,N,K', [(63, 68, 36), (65, 132, 33), (300, 192, 160)])
@pytest.mark.parametrize('tile', [0, 64, 128])
@pytest.mark.parametrize('mode', [6, 0])
def test_gemm_colsum(ar, gemm_tuning, layout, M, N, K, tile, mode):
    gemm_tuning(tile=tile or None, split=mode)
    _gemm(ar, np.random.RandomState(M + N), layout, [M], N, K, gate=True, colsum=True)


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('M,N,K', [(63, 68, 36), (65, 132, 33), (300, 192, 160)])
@pytest.mark.parametrize('tile', [0, 64, 128])
@pytest.mark.parametrize('mode', [6, 0])
def test_gemm_accumulate(ar, gemm_tuning, layout, M, N, K, tile, mode):
    gemm_tuning(tile=tile or None, split=mode)
    _gemm(ar, np.random.RandomState(M + 2 * N + K), layout, [M], N, K, accumulate=True)


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN'])
@pytest.mark.parametrize('tile', [0, 64, 128])
@pytest.mark.parametrize('mode', [6, 0])
@pytest.mark.parametrize('N,K,nseg', [(68, 36, 1), (192, 160, 1), (68, 64, 2)])
def test_gemm_two_groups_and_two_segments(ar, gemm_tuning, layout, tile, mode, N, K, nseg):
    """Two groups of 5 and 70 rows (both inside one 128-row tile, the second across two 64-row tiles); nseg = 2."""
    gemm_tuning(tile=tile or None, split=mode)
    _gemm(ar, np.random.RandomState(N + K + nseg), layout, [5, 70], N, K, nseg=nseg, bias=True)


@pytest.mark.parametrize('tile', [0, 64])
def test_gemm_weight_planes(ar, gemm_tuning, tile):
    """(129, 64, 64) with b_planes: the weight as three bf16 planes fetched by LDS-DMA.  The library accepts b_planes with
    ldb % 8 == 0, 64^2 tiles and MMNAS_GEMM_SPLIT=6 only (anything else is refused with MMNAS_E_ARG): this operand's leading
    dimension is K + 8 (the nearest accepted one), every other one width + 4; tile 128 and mode 0 are not in the table."""
    gemm_tuning(tile=tile or None, split=6)
    _gemm(ar, np.random.RandomState(129), 'NT', [129], 64, 64, planes=True, ldb_pad=8, bias=True, relu=True)


@pytest.mark.parametrize('mode', [6, 0])
@pytest.mark.parametrize('tile', [0, 64, 128])
def test_gemm_overlapping_rows_read_zero_past_the_extent(ar, gemm_tuning, tile, mode):
    """lda = d, K = 3 d: row m of A is the 3 d floats from m * d on (a 3-tap convolution window).  The operand holds M * d
    floats and not one more; the band behind it is NaN, and the product must equal the one on the zero-extended operand
    (include/mmnas_hip.h: "reads past the M * lda extent of such an operand return zero")."""
    L = _L()
    gemm_tuning(tile=tile or None, split=mode)
    rs = np.random.RandomState(3)
    M, d, N = 70, 32, 68
    K = 3 * d
    a, w = rnd(rs, M, d), rnd(rs, N, K)
    ad, _ = ar.inp(a, name='A')
    wd, _ = ar.inp(w, ld=K + PAD, name='W')
    cd, cv = ar.out((M, N), ld=N + PAD, name='C')
    g = L.GemmDesc()
    g.layout, g.ngroups, g.nseg, g.N, g.K, g.lda, g.ldb, g.ldc, g.alpha, g.gate_scale, g.split_k = 0, 1, 1, N, K, d, K + PAD, N + PAD, 1.0, 1.0, 1
    g.g[0].M, g.g[0].A[0], g.g[0].B[0], g.g[0].C = M, L.fptr(ad), L.fptr(wd), L.fptr(cd)
    L.check(L.lib().mmnas_gemm(C.byref(g), L.stream()))
    ar.check()
    ext = np.concatenate([a.reshape(-1), np.zeros(2 * d, np.float32)])
    win = np.stack([ext[m * d:m * d + K] for m in range(M)])
    assert rel_err(cpu(cv), gemm_ref('NT', win, w).numpy()) < 1e-5


@pytest.mark.parametrize('M,nin,nout', [(300, 132, 68), (64, 32, 32)])
@pytest.mark.parametrize('pair', [1, 0])
@pytest.mark.parametrize('mode', [6, 0])
def test_gemm_pair(ar, gemm_tuning, M, nin, nout, pair, mode):
    """Data gradient (NN, residual epilogue) + weight gradient (TN, accumulate) of one linear layer, every operand strided."""
    L = _L()
    gemm_tuning(pair=pair, split=mode)
    rs = np.random.RandomState(M + nin + nout)
    dy, x, W, res, dW0 = rnd(rs, M, nout), rnd(rs, M, nin), rnd(rs, nout, nin), rnd(rs, M, nin), rnd(rs, nout, nin)
    dyd, _ = ar.inp(dy, ld=nout + PAD, name='dy')
    xd, _ = ar.inp(x, ld=nin + PAD, name='x')
    Wd, _ = ar.inp(W, ld=nin + PAD, name='W')
    rd, _ = ar.inp(res, ld=nin + PAD, name='res')
    dxd, dxv = ar.out((M, nin), ld=nin + PAD, name='dx')
    dWd, dWv = ar.inout(dW0, ld=nin + PAD, name='dW')
    dg, wg = L.GemmDesc(), L.GemmDesc()
    for g in (dg, wg):
        g.ngroups, g.nseg, g.alpha, g.gate_scale, g.split_k = 1, 1, 1.0, 1.0, 1
    dg.layout, dg.N, dg.K, dg.lda, dg.ldb, dg.ldc, dg.ldres = 1, nin, nout, nout + PAD, nin + PAD, nin + PAD, nin + PAD
    dg.g[0].M, dg.g[0].A[0], dg.g[0].B[0], dg.g[0].C, dg.g[0].residual = M, L.fptr(dyd), L.fptr(Wd), L.fptr(dxd), L.fptr(rd)
    wg.layout, wg.N, wg.K, wg.lda, wg.ldb, wg.ldc, wg.accumulate = 2, nin, M, nout + PAD, nin + PAD, nin + PAD, 1
    wg.g[0].M, wg.g[0].A[0], wg.g[0].B[0], wg.g[0].C = nout, L.fptr(dyd), L.fptr(xd), L.fptr(dWd)
    L.check(L.lib().mmnas_gemm_pair(C.byref(dg), C.byref(wg), L.stream()))
    ar.check()
    td = lambda a: torch.from_numpy(a).double()
    assert rel_err(cpu(dxv), (td(dy) @ td(W) + td(res)).numpy()) < 1e-5
    assert rel_err(cpu(dWv), (td(dW0) + td(dy).t() @ td(x)).numpy()) < 1e-5


@pytest.mark.parametrize('M,K', [(33, 64), (129, 192)])       # (the panel kernel needs K % 64 == 0; 32-row panels: ragged last one)
@pytest.mark.parametrize('panel', [1, 0])
def test_gemm_ln(ar, M, K, panel):
    """N = 256 with the row-panel switch on and off (setter, restored).  lda = ldb = K + 4, ldres = N + 4.  Switch on: z has
    ldc = N + 4 too -- the two-launch form refuses that (MMNAS_E_ARG), so a quiet fall-back to it cannot pass as the panel kernel;
    switch off: the two-launch form, which needs ldc = N."""
    L = _L()
    from oracle import dropout_rng
    rs = np.random.RandomState(M + K)
    N = 256
    ldc = N + PAD if panel else N
    A, W, b, R = rnd(rs, M, K), rnd(rs, N, K) / np.float32(np.sqrt(K)), rnd(rs, N), rnd(rs, M, N)
    la, lb = 1 + 0.3 * rnd(rs, N), 0.3 * rnd(rs, N)
    drop = (0.1, 0x1234567887654321 + M, 1)
    Ad, _ = ar.inp(A, ld=K + PAD, name='A')
    Wd, _ = ar.inp(W, ld=K + PAD, name='W')
    bd, _ = ar.inp(b, name='bias')
    Rd, _ = ar.inp(R, ld=N + PAD, name='res')
    lad, _ = ar.inp(la, name='ln_a')
    lbd, _ = ar.inp(lb, name='ln_b')
    zd, zv = ar.out((M, N), ld=ldc, name='z')
    yd, yv = ar.out((M, N), name='y')
    d = L.GemmDesc()
    d.layout, d.ngroups, d.nseg, d.N, d.K, d.lda, d.ldb, d.ldc, d.ldres = 0, 1, 1, N, K, K + PAD, K + PAD, ldc, N + PAD
    d.alpha, d.gate_scale, d.split_k = 1.0, 1.0, 1
    d.drop_p, d.drop_seed, d.drop_site = drop
    g = d.g[0]
    g.M, g.A[0], g.B[0], g.C, g.bias, g.residual = M, L.fptr(Ad), L.fptr(Wd), L.fptr(zd), L.fptr(bd), L.fptr(Rd)
    old = L.lib().mmnas_set_gemm_ln(panel)
    try:
        L.check(L.lib().mmnas_gemm_ln(C.byref(d), L.fptr(lad), L.fptr(lbd), L.fptr(yd), 1e-6, L.stream()))
        ar.check()
    finally:
        L.lib().mmnas_set_gemm_ln(old)
    dm = dropout_rng.scaled_mask(drop[1], drop[2], (M, N), drop[0])
    zr = gemm_epilogue_ref(gemm_ref('NT', A, W), b, False, dm, None, 1.0, R)
    assert rel_err(cpu(zv), zr.numpy()) < TOL                          # (test_gemm_ln_gpu.py's bounds)
    assert rel_err(cpu(yv), layer_norm_ref(zr.numpy(), la, lb).numpy()) < 2e-5


# ----------------------------------------------------------------------------- row ops
LN_SHAPES = [(1, 4), (5, 36), (7, 260), (3, 2048), (2049, 36)]


@pytest.mark.parametrize('M,d', LN_SHAPES)
def test_layernorm_fwd(ar, M, d):
    L = _L()
    rs = np.random.RandomState(d + M)
    x, a, b = rnd(rs, M, d) * 2 + 0.3, 1 + 0.2 * rnd(rs, d), 0.1 * rnd(rs, d)
    (xd, _), (ad, _), (bd, _) = ar.inp(x, name='x'), ar.inp(a, name='a'), ar.inp(b, name='b')
    yd, yv = ar.out((M, d), name='y')
    L.check(L.lib().mmnas_layernorm_fwd(L.fptr(xd), L.fptr(ad), L.fptr(bd), L.fptr(yd), M, d, 1e-6, L.stream()))
    ar.check()
    assert rel_err(cpu(yv), layer_norm_ref(x, a, b).numpy()) < 1e-5


@pytest.mark.parametrize('M,d', LN_SHAPES)
@pytest.mark.parametrize('use_ws', [True, False])
@pytest.mark.parametrize('extra', ['none', 'ddrop', 'ddrop+dcol'])
def test_layernorm_bwd(ar, M, d, use_ws, extra):
    L = _L()
    from oracle import dropout_rng
    rs = np.random.RandomState(d + M)
    p, seed = 0.2, 99
    x, a, gy = rnd(rs, M, d) * 2 + 0.3, 1 + 0.2 * rnd(rs, d), rnd(rs, M, d)
    (xd, _), (ad, _), (gd, _) = ar.inp(x, name='x'), ar.inp(a, name='a'), ar.inp(gy, name='dy')
    dxd, dxv = ar.out((M, d), name='dx')
    (dad, dav), (dbd, dbv) = ar.inout(zeros(d), name='da'), ar.inout(zeros(d), name='db')
    ddd = ddv = dcd = dcv = None
    if extra != 'none':
        ddd, ddv = ar.out((M, d), name='ddrop')
    if extra == 'ddrop+dcol':
        dcd, dcv = ar.inout(zeros(d), name='dcol')
    ws = ar.scratch_floats(L.lib().mmnas_layernorm_bwd_ws_floats(M, d), name='ws')[0] if use_ws else None
    L.check(L.lib().mmnas_layernorm_bwd(L.fptr(xd), L.fptr(ad), L.fptr(gd), L.fptr(dxd), L.fptr(dad), L.fptr(dbd), L.fptr(ddd),
                                        L.fptr(dcd), L.fptr(ws), p, seed, 1, M, d, 1e-6, L.stream()))
    ar.check()
    rdx, rda, rdb = layer_norm_bwd_ref(x, a, gy)
    assert rel_err(cpu(dxv), rdx.numpy()) < 1e-4
    assert rel_err(cpu(dav), rda.numpy()) < 1e-4
    assert rel_err(cpu(dbv), rdb.numpy()) < 1e-4
    if ddv is not None:
        rdd = rdx * torch.from_numpy(dropout_rng.scaled_mask(seed, 1, (M, d), p)).double()
        assert rel_err(cpu(ddv), rdd.numpy()) < 1e-4
        if dcv is not None:
            assert rel_err(cpu(dcv), rdd.sum(0).numpy()) < 1e-4


@pytest.mark.parametrize('M,N,ldx', [(1, 1, 1), (65, 63, 67), (777, 65, 68)])
def test_colsum(ar, M, N, ldx):
    L = _L()
    rs = np.random.RandomState(M + N)
    x, o0 = rnd(rs, M, N), rnd(rs, N)
    xd, _ = ar.inp(x, ld=ldx, name='x')
    od, ov = ar.inout(o0, name='out')
    L.check(L.lib().mmnas_colsum(L.fptr(xd), L.fptr(od), M, N, ldx, L.stream()))
    ar.check()
    assert rel_err(cpu(ov), o0.astype(np.float64) + x.astype(np.float64).sum(0)) < 1e-5


ELT_N = [1, 255, 257, 2048 * 256 + 3]       # the last: beyond the 2048-block grid cap (grid-stride loop)


@pytest.mark.parametrize('n', ELT_N)
@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_eltwise(ar, n, kind):
    L = _L()
    rs = np.random.RandomState(n + kind)
    x, gy = rnd(rs, n), rnd(rs, n)
    (xd, _), (gd, _) = ar.inp(x, name='x'), ar.inp(gy, name='dy')
    yd, yv = ar.out(n, name='y')
    dxd, dxv = ar.out(n, name='dx')
    L.check(L.lib().mmnas_eltwise_fwd(kind, L.fptr(xd), L.fptr(yd), n, L.stream()))
    L.check(L.lib().mmnas_eltwise_bwd(kind, L.fptr(xd), L.fptr(gd), L.fptr(dxd), n, L.stream()))
    ar.check()
    r, rdx = eltwise_ref(kind, x, gy)
    assert rel_err(cpu(yv), r.numpy()) < 1e-5 and rel_err(cpu(dxv), rdx.numpy()) < 1e-5


@pytest.mark.parametrize('n', ELT_N)
@pytest.mark.parametrize('with_res', [True, False])
def test_drop_add(ar, n, with_res):
    L = _L()
    from oracle import dropout_rng
    rs = np.random.RandomState(n)
    x, r = rnd(rs, n), rnd(rs, n)
    xd, _ = ar.inp(x, name='x')
    rd = ar.inp(r, name='res')[0] if with_res else None
    yd, yv = ar.out(n, name='y')
    L.check(L.lib().mmnas_drop_add(L.fptr(xd), L.fptr(rd), L.fptr(yd), n, 0.5, 77, 1, L.stream()))
    ar.check()
    ref = (r if with_res else 0) + x * dropout_rng.scaled_mask(77, 1, (n,), 0.5)
    assert rel_err(cpu(yv), ref) < 1e-6


@pytest.mark.parametrize('M,C_', [(1, 1), (1, 255), (257, 1), (1, 2048 * 256 + 3)])       # M * C = 1, 255, 257, 2048 * 256 + 3
def test_glu(ar, M, C_):
    L = _L()
    from oracle import dropout_rng
    rs = np.random.RandomState(M + C_)
    seed, p = 4242, 0.3
    h, gy = rnd(rs, M, 2 * C_), rnd(rs, M, C_)
    (hd, _), (gd, _) = ar.inp(h, name='h'), ar.inp(gy, name='dy')
    yd, yv = ar.out((M, C_), name='y')
    dhd, dhv = ar.out((M, 2 * C_), name='dh')
    L.check(L.lib().mmnas_glu_fwd(L.fptr(hd), L.fptr(yd), M, C_, 1, p, seed, 0, L.stream()))
    L.check(L.lib().mmnas_glu_bwd(L.fptr(hd), L.fptr(gd), L.fptr(dhd), M, C_, 1, p, seed, 0, L.stream()))
    ar.check()
    r, rdh = glu_ref(h, gy, relu=True, dmask=dropout_rng.scaled_mask(seed, 0, (M, C_), p))
    assert rel_err(cpu(yv), r.numpy()) < 1e-5 and rel_err(cpu(dhv), rdh.numpy()) < 1e-5


# ----------------------------------------------------------------------------- attention core
def _mha_desc(L, B, H, Sq, Sk, dh, lds):
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, dh
    d.ldq, d.ldk, d.ldv, d.ldo = lds
    return d


MHA_SHAPES = [(1, 1, 64), (33, 31, 16), (65, 33, 32), (64, 64, 64), (65, 65, 64), (128, 128, 64), (129, 129, 64), (1, 256, 128),
              (40, 10, 256)]


@pytest.mark.parametrize('Sq,Sk,dh', MHA_SHAPES)
@pytest.mark.parametrize('use_mask,use_bias,p,lds', [(True, True, 0.1, (4, 4, 4, 4)), (False, False, 0.0, (4, 8, 12, 16))],
                         ids=['mask+bias+drop', 'plain-4-lds'])
def test_mha_core(ar, Sq, Sk, dh, use_mask, use_bias, p, lds):
    """ldq, ldk, ldv, ldo = H * dh + 4 (second variant: + 4, + 8, + 12, + 16, pairwise different); lse, delta, dbiasT, dK, dV
    all guarded.  The mask pads one sample completely, as in test_mha_core."""
    L = _L()
    from oracle import dropout_rng
    B, H = 2, 2
    rs = np.random.RandomState(H * 3 + Sq * 5 + Sk * 7 + dh)
    di = H * dh
    lds = tuple(di + x for x in lds)
    Q, K, V, dO = rnd(rs, B, Sq, di), rnd(rs, B, Sk, di), rnd(rs, B, Sk, di), rnd(rs, B, Sq, di)
    mask = np.zeros((B, Sk), np.bool_)
    if use_mask:
        mask[0, max(1, Sk // 2):] = Sk > 1
        mask[B - 1] = True                      # fully padded sample: uniform softmax
    biasT = (rnd(rs, B, H, Sk, Sq) * 2) if use_bias else None
    seed = 31337
    Qd, _ = ar.inp(Q.reshape(B * Sq, di), ld=lds[0], name='Q')
    Kd, _ = ar.inp(K.reshape(B * Sk, di), ld=lds[1], name='K')
    Vd, _ = ar.inp(V.reshape(B * Sk, di), ld=lds[2], name='V')
    m8 = ar.inp(mask.astype(np.uint8), name='mask')[0] if use_mask else None
    bd = ar.inp(biasT, name='biasT')[0] if use_bias else None
    Od, Ov = ar.out((B * Sq, di), ld=lds[3], name='O')
    sd, _ = ar.out((B, H, Sq, 2), name='lse')
    d = _mha_desc(L, B, H, Sq, Sk, dh, lds)
    d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = L.fptr(Qd), L.fptr(Kd), L.fptr(Vd), L.ptr(m8), L.fptr(bd), L.fptr(Od), L.fptr(sd)
    d.drop_p, d.drop_site, d.drop_seed = p, 0, seed
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    ar.check()
    Qt, Kt, Vt = (torch.from_numpy(v).double().requires_grad_(True) for v in (Q, K, V))
    bt = torch.from_numpy(biasT).double().requires_grad_(True) if use_bias else None
    dm = torch.from_numpy(dropout_rng.scaled_mask(seed, 0, (B, H, Sq, Sk), p)).double() if p > 0 else None
    ref = mha_ref(Qt, Kt, Vt, torch.from_numpy(mask) if use_mask else None, bt, H, dh, dm)
    assert rel_err(cpu(Ov).reshape(B, Sq, di), ref.detach().numpy()) < 1e-5
    ref.backward(torch.from_numpy(dO).double())
    dOd, _ = ar.inp(dO.reshape(B * Sq, di), ld=lds[3], name='dO')
    dQd, dQv = ar.out((B * Sq, di), ld=lds[0], name='dQ')
    dKd, dKv = ar.out((B * Sk, di), ld=lds[1], name='dK')
    dVd, dVv = ar.out((B * Sk, di), ld=lds[2], name='dV')
    dbd, dbv = ar.out((B, H, Sk, Sq), name='dbiasT') if use_bias else (None, None)
    dl, _ = ar.scratch_floats(B * H * Sq, name='delta')        # (scratch: the fused backward kernels do not use it)
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQd), L.fptr(dKd), L.fptr(dVd), L.fptr(dbd), L.fptr(dl)
    L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
    ar.check()
    assert rel_err(cpu(dQv).reshape(B, Sq, di), Qt.grad.numpy()) < 1e-4
    assert rel_err(cpu(dKv).reshape(B, Sk, di), Kt.grad.numpy()) < 1e-4
    assert rel_err(cpu(dVv).reshape(B, Sk, di), Vt.grad.numpy()) < 1e-4
    if use_bias:
        assert rel_err(cpu(dbv), bt.grad.numpy()) < 1e-4


@pytest.mark.parametrize('lens,use_bias,p', [([5, 0, 1, 33], False, 0.0), ([64, 1, 0, 17], True, 0.1)])
def test_mha_core_packed_rows(ar, lens, use_bias, p):
    """q_off / k_off (self-attention over packed rows, d_h = 64) with one empty and one single-row sequence.  lse, delta and
    dbiasT keep the padded layout: only a sequence's own corner of them is the kernels' to write (given as accumulators)."""
    L = _L()
    from oracle import dropout_rng
    B, H, dh = len(lens), 2, 64
    di, Sm = H * dh, max(lens)
    rs = np.random.RandomState(sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    Nr = int(off[-1])
    Q, K, V, dO = rnd(rs, Nr, di), rnd(rs, Nr, di), rnd(rs, Nr, di), rnd(rs, Nr, di)
    biasT = (rnd(rs, B, H, Sm, Sm) * 2) if use_bias else None
    seed, ld = 777, di + PAD
    (Qd, _), (Kd, _), (Vd, _) = ar.inp(Q, ld=ld, name='Q'), ar.inp(K, ld=ld, name='K'), ar.inp(V, ld=ld, name='V')
    offd, _ = ar.inp(off, name='off')
    bd = ar.inp(biasT, name='biasT')[0] if use_bias else None
    Od, Ov = ar.out((Nr, di), ld=ld, name='O')
    sd, _ = ar.inout(zeros(B, H, Sm, 2), name='lse')
    d = _mha_desc(L, B, H, Sm, Sm, dh, (ld,) * 4)
    d.Q, d.K, d.V, d.biasT, d.O, d.lse = L.fptr(Qd), L.fptr(Kd), L.fptr(Vd), L.fptr(bd), L.fptr(Od), L.fptr(sd)
    d.q_off = d.k_off = L.ptr(offd)
    d.drop_p, d.drop_site, d.drop_seed = p, 0, seed
    L.check(L.lib().mmnas_mha_core_fwd(C.byref(d), L.stream()))
    ar.check()
    dOd, _ = ar.inp(dO, ld=ld, name='dO')
    (dQd, dQv), (dKd, dKv), (dVd, dVv) = ar.out((Nr, di), ld=ld, name='dQ'), ar.out((Nr, di), ld=ld, name='dK'), ar.out((Nr, di), ld=ld, name='dV')
    dbd, dbv = ar.inout(zeros(B, H, Sm, Sm), name='dbiasT') if use_bias else (None, None)
    dl, _ = ar.inout(zeros(B, H, Sm), name='delta')
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = L.fptr(dOd), L.fptr(dQd), L.fptr(dKd), L.fptr(dVd), L.fptr(dbd), L.fptr(dl)
    L.check(L.lib().mmnas_mha_core_bwd(C.byref(d), L.stream()))
    ar.check()
    dm_all = dropout_rng.scaled_mask(seed, 0, (B, H, Sm, Sm), p) if p > 0 else None
    Oc, dQc, dKc, dVc = cpu(Ov), cpu(dQv), cpu(dKv), cpu(dVv)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        r0, r1 = int(off[b]), int(off[b + 1])
        Qt, Kt, Vt = (torch.from_numpy(a[r0:r1]).double().unsqueeze(0).requires_grad_(True) for a in (Q, K, V))
        bt = torch.from_numpy(biasT[b:b + 1, :, :n, :n].copy()).double().requires_grad_(True) if use_bias else None
        dm = torch.from_numpy(dm_all[b:b + 1, :, :n, :n].copy()).double() if p > 0 else None
        ref = mha_ref(Qt, Kt, Vt, None, bt, H, dh, dm)
        assert rel_err(Oc[r0:r1], ref[0].detach().numpy()) < 1e-5, b
        ref.backward(torch.from_numpy(dO[r0:r1]).double().unsqueeze(0))
        assert rel_err(dQc[r0:r1], Qt.grad[0].numpy()) < 1e-4, b
        assert rel_err(dKc[r0:r1], Kt.grad[0].numpy()) < 1e-4, b
        assert rel_err(dVc[r0:r1], Vt.grad[0].numpy()) < 1e-4, b
        if use_bias:
            assert rel_err(cpu(dbv)[b, :, :n, :n], bt.grad[0].numpy()) < 1e-4, b


@pytest.mark.parametrize('Sk', [1, 64])
def test_mha_core_fwd_indexed(ar, Sk):
    """Query batch b reads the K / V / mask rows of batch kv_idx[b]; ldk = ldv wider than H * dh (slices of a wider product)."""
    L = _L()
    B, Bkv, H, Sq, dh = 5, 3, 2, 9, 64
    di = H * dh
    rs = np.random.RandomState(Sk)
    Q, K, V = rnd(rs, B, Sq, di), rnd(rs, Bkv, Sk, di), rnd(rs, Bkv, Sk, di)
    mask = np.zeros((Bkv, Sk), np.bool_)
    mask[1, Sk // 2:] = True
    idx = np.array([2, 0, 1, 1, 2], np.int32)
    Qd, _ = ar.inp(Q.reshape(B * Sq, di), ld=di + PAD, name='Q')
    Kd, _ = ar.inp(K.reshape(Bkv * Sk, di), ld=2 * di + 8, name='K')
    Vd, _ = ar.inp(V.reshape(Bkv * Sk, di), ld=2 * di + 8, name='V')
    m8, _ = ar.inp(mask.astype(np.uint8), name='mask')
    ix, _ = ar.inp(idx, name='kv_idx')
    Od, Ov = ar.out((B * Sq, di), ld=di + PAD, name='O')
    sd, _ = ar.out((B, H, Sq, 2), name='lse')
    d = _mha_desc(L, B, H, Sq, Sk, dh, (di + PAD, 2 * di + 8, 2 * di + 8, di + PAD))
    d.Q, d.K, d.V, d.mask, d.O, d.lse = L.fptr(Qd), L.fptr(Kd), L.fptr(Vd), L.ptr(m8), L.fptr(Od), L.fptr(sd)
    L.check(L.lib().mmnas_mha_core_fwd_indexed(C.byref(d), L.ptr(ix), L.stream()))
    ar.check()
    T = lambda a: torch.from_numpy(a).double()
    ref = mha_ref(T(Q), T(K[idx]), T(V[idx]), torch.from_numpy(mask[idx]), None, H, dh)
    assert rel_err(cpu(Ov).reshape(B, Sq, di), ref.numpy()) < 1e-5


# ----------------------------------------------------------------------------- relation kernels
@pytest.mark.parametrize('B,Sq,Sk,R,H', [(1, 5, 5, 64, 32), (2, 6, 6, 32, 4)])      # (the two smallest of test_rel_bias)
def test_rel_bias(ar, B, Sq, Sk, R, H):
    L = _L()
    rs = np.random.RandomState(B * 100 + Sq + H)
    rel = np.maximum(rnd(rs, B, Sq, Sk, R), 0)
    Wr, br, gb = rnd(rs, H, R) / 8, 0.1 * rnd(rs, H), rnd(rs, B, H, Sk, Sq)
    (reld, _), (Wd, _), (bd, _), (gbd, _) = ar.inp(rel, name='rel'), ar.inp(Wr, name='Wr'), ar.inp(br, name='br'), ar.inp(gb, name='dbiasT')
    bTd, bTv = ar.out((B, H, Sk, Sq), name='biasT')
    L.check(L.lib().mmnas_rel_bias_fwd(L.fptr(reld), L.fptr(Wd), L.fptr(bd), L.fptr(bTd), B, Sq, Sk, R, H, L.stream()))
    ar.check()
    bias, rdrel, rdW, rdb = rel_bias_ref(rel, Wr, br, gb)
    assert rel_err(cpu(bTv), bias.numpy()) < TOL
    dreld, drelv = ar.out((B, Sq, Sk, R), name='drel')
    (dWd, dWv), (dbd, dbv) = ar.inout(zeros(H, R), name='dWr'), ar.inout(zeros(H), name='dbr')
    L.check(L.lib().mmnas_rel_bias_bwd(L.fptr(reld), L.fptr(Wd), L.fptr(bd), L.fptr(gbd), L.fptr(dreld), L.fptr(dWd), L.fptr(dbd), 0,
                                       B, Sq, Sk, R, H, L.stream()))
    ar.check()
    assert rel_err(cpu(drelv), rdrel.numpy()) < TOL
    assert rel_err(cpu(dWv), rdW.numpy()) < TOL and rel_err(cpu(dbv), rdb.numpy()) < TOL


def _rel_params(ar, rs, C_, H, R=64):
    Wy, by, Wr, br = rnd(rs, R, C_) / 2, 0.1 * rnd(rs, R), rnd(rs, H, R) / 8, 0.1 * rnd(rs, H)
    dev = [ar.inp(a, name=n)[0] for a, n in ((Wy, 'Wy'), (by, 'by'), (Wr, 'Wr'), (br, 'br'))]
    return (Wy, by, Wr, br), dev


def _rel_grads(ar, C_, H, R=64):
    return [ar.inout(zeros(*sh), name=n) for sh, n in (((R, C_), 'dWy'), ((R,), 'dby'), ((H, R), 'dWr'), ((H,), 'dbr'))]


@pytest.mark.parametrize('B,Sq,Sk,C_,H', [(2, 7, 7, 4, 2), (3, 5, 9, 3, 4)])       # (the two smallest of test_rel_fused_lazy_handle)
def test_rel_fused_dense(ar, B, Sq, Sk, C_, H):
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(B * 131 + Sq + H + C_)
    R = 64
    assert lib.mmnas_rel_fused_supported(C_, R, H) == 1
    raw = rnd(rs, B, Sq, Sk, C_)
    raw[:, Sq // 2:, :, :] *= (rs.uniform(size=(B, Sq - Sq // 2, Sk, 1)) < 0.7)
    (Wy, by, Wr, br), (Wyd, byd, Wrd, brd) = _rel_params(ar, rs, C_, H)
    gb = rnd(rs, B, H, Sk, Sq)
    (rawd, _), (gbd, _) = ar.inp(raw, name='raw'), ar.inp(gb, name='dbiasT')
    bTd, bTv = ar.out((B, H, Sk, Sq), name='biasT')
    L.check(lib.mmnas_rel_fused_fwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(bTd), B, Sq, Sk, C_, R, H,
                                    L.stream()))
    ar.check()
    bias, *rg = rel_fused_ref(raw, Wy, by, Wr, br, gb)
    assert rel_err(cpu(bTv), bias) < TOL
    grads = _rel_grads(ar, C_, H)
    ws, _ = ar.scratch_floats(lib.mmnas_rel_fused_bwd_ws_floats(B, Sq, Sk), name='ws')
    L.check(lib.mmnas_rel_fused_bwd(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(gbd),
                                    *[L.fptr(t[0]) for t in grads], L.fptr(ws), B, Sq, Sk, C_, R, H, L.stream()))
    ar.check()
    for (_, v), want in zip(grads, rg):
        assert rel_err(cpu(v), want) < TOL


@pytest.mark.parametrize('B,S,C_,H,lens', [(5, 14, 3, 4, [14, 3, 7, 1, 9]), (2, 36, 4, 16, [36, 20])])  # (smallest of test_rel_fused_ragged)
def test_rel_fused_ragged(ar, B, S, C_, H, lens):
    """Lengths include 1 and the maximum.  Forward writes the n_b x n_b corners only (the rest of biasT must keep the pattern);
    backward reads dbiasT there only (the rest is the pattern: NaN)."""
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(B * 17 + S + H + C_)
    R = 64
    raw = rnd(rs, B, S, S, C_)
    (Wy, by, Wr, br), (Wyd, byd, Wrd, brd) = _rel_params(ar, rs, C_, H)
    gb = rnd(rs, B, H, S, S)
    valid = np.zeros((B, H, S, S), bool)
    for b, n in enumerate(lens):
        valid[b, :, :n, :n] = True
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    toff = np.concatenate([[0], np.cumsum([(n * n + 31) // 32 for n in lens])]).astype(np.int32)
    (offd, _), (toffd, _), (rawd, _) = ar.inp(off, name='off'), ar.inp(toff, name='tile_off'), ar.inp(raw, name='raw')
    bTd, bTv = ar.out((B, H, S, S), name='biasT', written=valid)
    L.check(lib.mmnas_rel_fused_fwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(bTd), B, S, C_, R, H,
                                           L.ptr(offd), L.stream()))
    ar.check()
    gb_dense = np.where(valid, gb, 0).astype(np.float32)
    bias, *rg = rel_fused_ref(raw, Wy, by, Wr, br, gb_dense)
    assert rel_err(np.where(valid, cpu(bTv), 0), np.where(valid, bias, 0)) < TOL
    gbd, _ = ar.inp(np.where(valid, gb, np.nan).astype(np.float32), name='dbiasT')
    grads = _rel_grads(ar, C_, H)
    ws, _ = ar.scratch_floats(lib.mmnas_rel_fused_bwd_ws_floats(B, S, S), name='ws')
    L.check(lib.mmnas_rel_fused_bwd_ragged(L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(Wrd), L.fptr(brd), L.fptr(gbd),
                                           *[L.fptr(t[0]) for t in grads], L.fptr(ws), B, S, C_, R, H, L.ptr(offd), L.ptr(toffd),
                                           int(toff[-1]), L.stream()))
    ar.check()
    for (_, v), want in zip(grads, rg):
        got = cpu(v)
        assert np.isfinite(got).all() and rel_err(got, want) < TOL


@pytest.mark.parametrize('B,S,C_,H,n_ops,lens', [(2, 7, 4, 2, 3, None), (2, 9, 4, 32, 2, None), (4, 23, 4, 4, 9, (23, 1, 7, 16))])
def test_rel_multi(ar, B, S, C_, H, n_ops, lens):
    """The two smallest dense shapes of test_rel_multi_all_relation_operators_in_one_launch and its smallest ragged one (lengths
    1 and the maximum); that test's conditioning (no bias gradient next to the clamp) and bounds."""
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(B * 31 + S + 7 * H + C_ + n_ops)
    R = 64
    assert lib.mmnas_rel_multi_supported(C_, R, H) == 1
    raw = rnd(rs, B, S, S, C_)
    Wy, by = rnd(rs, R, C_) / 2, 0.1 * rnd(rs, R)
    Wrs, brs = [rnd(rs, H, R) / 8 for _ in range(n_ops)], [0.1 * rnd(rs, H) for _ in range(n_ops)]
    gbs = [rnd(rs, B, H, S, S) for _ in range(n_ops)]
    valid = np.ones((B, 1, S, S), np.float32)
    m = L.RelMulti()
    if lens is not None:
        valid[:] = 0
        for b, n in enumerate(lens):
            valid[b, :, :n, :n] = 1
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        toff = np.concatenate([[0], np.cumsum([(n * n + 31) // 32 for n in lens])]).astype(np.int32)
        (offd, _), (toffd, _) = ar.inp(off, name='off'), ar.inp(toff, name='tile_off')
        m.off, m.tile_off, m.ntiles = L.ptr(offd), L.ptr(toffd), int(toff[-1])
    vfull = np.broadcast_to(valid > 0, (B, H, S, S))
    for i in range(n_ops):
        gbs[i] = np.where(np.abs(rel_multi_pre(raw, Wy, by, Wrs[i], brs[i])) < 0.05, 0.0, gbs[i]).astype(np.float32)
    (rawd, _), (Wyd, _), (byd, _) = ar.inp(raw, name='raw'), ar.inp(Wy, name='Wy'), ar.inp(by, name='by')
    (dWyd, dWyv), (dbyd, dbyv) = ar.inout(zeros(R, C_), name='dWy'), ar.inout(zeros(R), name='dby')
    ws, _ = ar.scratch_floats(lib.mmnas_rel_multi_bwd_ws_floats(B, S), name='ws')
    m.B, m.S, m.C, m.R, m.H, m.n_ops = B, S, C_, R, H, n_ops
    m.raw, m.Wy, m.by, m.dWy, m.dby, m.ws = L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(dWyd), L.fptr(dbyd), L.fptr(ws)
    bias, dWr, dbr, keep = [], [], [], []
    for i in range(n_ops):
        keep.append((ar.inp(Wrs[i], name='Wr%d' % i)[0], ar.inp(brs[i], name='br%d' % i)[0],
                     ar.inp(np.where(valid > 0, gbs[i], np.nan).astype(np.float32), name='dbiasT%d' % i)[0]))
        bias.append(ar.out((B, H, S, S), name='biasT%d' % i, written=vfull))
        dWr.append(ar.inout(zeros(H, R), name='dWr%d' % i))
        dbr.append(ar.inout(zeros(H), name='dbr%d' % i))
        m.Wr[i], m.br[i], m.dbiasT[i] = (L.fptr(t) for t in keep[-1])
        m.biasT[i], m.dWr[i], m.dbr[i] = L.fptr(bias[i][0]), L.fptr(dWr[i][0]), L.fptr(dbr[i][0])
    L.check(lib.mmnas_rel_multi_fwd(C.byref(m), L.stream()))
    L.check(lib.mmnas_rel_multi_bwd(C.byref(m), L.stream()))
    ar.check()
    r_ref, rdWr, rdbr, rdWy, rdby = rel_multi_ref(raw, Wy, by, Wrs, brs, gbs, valid)
    for i in range(n_ops):
        rr = np.exp(np.where(vfull, cpu(bias[i][1]), 0).astype(np.float64))
        assert float((np.abs(rr - r_ref[i]) * valid).max()) <= 2e-5 * float(np.abs(r_ref[i]).max()), i
        assert rel_err(cpu(dWr[i][1]), rdWr[i]) < 1e-4 and rel_err(cpu(dbr[i][1]), rdbr[i]) < 1e-4, i
    assert rel_err(cpu(dWyv), rdWy) < 1e-4 and rel_err(cpu(dbyv), rdby) < 1e-4


# ----------------------------------------------------------------------------- smaller kernels
@pytest.mark.parametrize('B,S,d,G', [(3, 14, 512, 1), (2, 7, 36, 2)])
def test_attflat_pool(ar, B, S, d, G):
    L = _L()
    rs = np.random.RandomState(B * 7 + S)
    logits, x, gp = rnd(rs, B, S, G), rnd(rs, B, S, d), rnd(rs, B, G * d)
    mask = rs.uniform(size=(B, S)) < 0.3
    mask[0] = True                      # everything padded: uniform
    (ld, _), (xd, _), (md, _), (gd, _) = ar.inp(logits, name='logits'), ar.inp(x, name='x'), ar.inp(mask.astype(np.uint8), name='mask'), ar.inp(gp, name='dpooled')
    (pd, pv), (od, ov) = ar.out((B, S, G), name='probs'), ar.out((B, G * d), name='pooled')
    L.check(L.lib().mmnas_attflat_pool_fwd(L.fptr(ld), L.fptr(xd), L.ptr(md), L.fptr(pd), L.fptr(od), B, S, d, G, L.stream()))
    ar.check()
    ref, rdl, rdx, att = attflat_pool_ref(logits, x, mask, gp)
    assert rel_err(cpu(ov), ref.numpy()) < 1e-5 and rel_err(cpu(pv), att.numpy()) < 1e-5
    (dld, dlv), (dxd, dxv) = ar.out((B, S, G), name='dlogits'), ar.out((B, S, d), name='dx')
    L.check(L.lib().mmnas_attflat_pool_bwd(L.fptr(pd), L.fptr(xd), L.ptr(md), L.fptr(gd), L.fptr(dld), L.fptr(dxd), B, S, d, G, L.stream()))
    ar.check()
    assert rel_err(cpu(dxv), rdx.numpy()) < 1e-5 and rel_err(cpu(dlv), rdl.numpy()) < 2e-5


@pytest.mark.parametrize('rows', [5, 37])
@pytest.mark.parametrize('bias', [True, False])
def test_glimpse1(ar, rows, bias):
    """K = 4: the smallest K mmnas_glimpse1_supported accepts."""
    L = _L()
    lib = L.lib()
    K = 4
    assert lib.mmnas_glimpse1_supported(K) == 1
    rs = np.random.RandomState(rows)
    x, w, b, dy, dw0, db0 = rnd(rs, rows, K), rnd(rs, K), rnd(rs, 1), rnd(rs, rows), rnd(rs, K), rnd(rs, 1)
    (xd, _), (wd, _), (dyd, _) = ar.inp(x, name='x'), ar.inp(w, name='w'), ar.inp(dy, name='dy')
    bd = ar.inp(b, name='b')[0] if bias else None
    yd, yv = ar.out(rows, name='y')
    L.check(lib.mmnas_glimpse1_fwd(L.fptr(xd), L.fptr(wd), L.fptr(bd), L.fptr(yd), rows, K, L.stream()))
    ar.check()
    ref = x.astype(np.float64) @ w.astype(np.float64) + (float(b[0]) if bias else 0.0)
    assert rel_err(cpu(yv), ref) <= 2e-6
    dxd, dxv = ar.out((rows, K), name='dx')
    dwd, dwv = ar.inout(dw0, name='dw')
    dbd, dbv = ar.inout(db0, name='db') if bias else (None, None)
    ws, _ = ar.scratch_floats(lib.mmnas_glimpse1_bwd_ws_floats(rows, K), name='ws')
    L.check(lib.mmnas_glimpse1_bwd(L.fptr(dyd), L.fptr(xd), L.fptr(wd), L.fptr(dxd), L.fptr(dwd), L.fptr(dbd), L.fptr(ws), rows, K,
                                   L.stream()))
    ar.check()
    assert np.array_equal(cpu(dxv), dy[:, None] * w[None, :])
    assert rel_err(cpu(dwv), dw0.astype(np.float64) + dy.astype(np.float64) @ x.astype(np.float64)) <= 2e-6
    if bias:
        assert abs(float(cpu(dbv)[0]) - float(db0[0]) - float(dy.astype(np.float64).sum())) <= 2e-6 * float(np.abs(dy).sum())


@pytest.mark.parametrize('shape', [(3, 7, 5), (2, 9, 36), (1, 1, 4)])
def test_row_is_zero(ar, shape):
    L = _L()
    rs = np.random.RandomState(sum(shape))
    f = rnd(rs, *shape)
    f[rs.uniform(size=shape[:-1]) < 0.4] = 0.0
    if shape[0] > 1:
        f[0, 0] = -0.0
        f[1, 0] = 0.0
        f[1, 0, -1] = np.nan
    rows = int(np.prod(shape[:-1]))
    fd, _ = ar.inp(f, name='f')
    md, mv = ar.inout(np.full(shape[:-1], 7, np.uint8), name='mask')         # (7: neither answer -- every row must be written)
    L.check(L.lib().mmnas_row_is_zero(L.fptr(fd), L.ptr(md), rows, shape[-1], L.stream()))
    ar.check()
    assert np.array_equal(cpu(mv), (np.abs(f).sum(-1) == 0).astype(np.uint8))


def test_pack_and_unpack_rows(ar):
    """A sequence of length 0 and one of length S."""
    L = _L()
    rs = np.random.RandomState(4)
    B, S, d, lens = 3, 5, 8, [0, 5, 2]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = rnd(rs, B, S, d)
    (xd, _), (offd, _) = ar.inp(x, name='x'), ar.inp(off, name='off')
    pd, pv = ar.out((int(off[-1]), d), name='packed')
    L.check(L.lib().mmnas_pack_rows(L.fptr(xd), L.ptr(offd), L.fptr(pd), B, S, d, L.stream()))
    ar.check()
    want = np.concatenate([x[b, :n] for b, n in enumerate(lens)])
    assert np.array_equal(cpu(pv), want)
    ud, uv = ar.out((B, S, d), name='unpacked')
    L.check(L.lib().mmnas_unpack_rows(L.fptr(pd), L.ptr(offd), L.fptr(ud), B, S, d, L.stream()))
    ar.check()
    ref = np.zeros_like(x)
    for b, n in enumerate(lens):
        ref[b, :n] = x[b, :n]
    assert np.array_equal(cpu(uv), ref)


@pytest.mark.parametrize('V,E,n', [(7, 24, 3), (50, 300, 200)])
@pytest.mark.parametrize('det', [False, True])
def test_embedding_bwd(ar, V, E, n, det):
    """Token indices outside [0, V) are ignored (both kernels); the fixed-order kernel's workspace at its advertised size."""
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(V + n)
    idx = rs.randint(-2, V + 2, size=n).astype(np.int64)
    idx[::2] = 1
    idx[-1] = V + 1
    dy, base = rnd(rs, n, E), rnd(rs, V, E)
    scale = 0.25 if det else 1.0
    want = base.astype(np.float64)
    ok = (idx >= 0) & (idx < V)
    np.add.at(want, idx[ok], scale * dy[ok].astype(np.float64))
    (ixd, _), (dyd, _) = ar.inp(idx, name='idx'), ar.inp(dy, name='dy')
    dWd, dWv = ar.inout(base, name='dW')
    if det:
        ws, _ = ar.scratch_floats(lib.mmnas_embedding_bwd_det_ws_floats(n, E), name='ws')
        L.check(lib.mmnas_embedding_bwd_det(L.ptr(ixd), L.fptr(dyd), L.fptr(dWd), L.fptr(ws), n, E, V, scale, L.stream()))
    else:
        L.check(lib.mmnas_embedding_bwd(L.ptr(ixd), L.fptr(dyd), L.fptr(dWd), n, E, V, L.stream()))
    ar.check()
    assert rel_err(cpu(dWv), want) < (2e-6 if det else 1e-6)      # (each kernel's own existing bound)


@pytest.mark.parametrize('M,d', [(1, 4), (257, 4)])         # count = M * d = 4 and 4 * 257
def test_node_mix_and_mixed_sum(ar, M, d):
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(M)
    n, active, eps = 3, 1, 1e-6
    z = [rnd(rs, M, d) * 1.5 + 0.3 for _ in range(n)]
    la = [None, rs.uniform(0.5, 1.5, d).astype(np.float32), rs.uniform(0.5, 1.5, d).astype(np.float32)]
    lb = [None, rnd(rs, d), rnd(rs, d)]
    gate, dout = rnd(rs, n), rnd(rs, M, d)
    zd = [ar.inp(a, name='z%d' % j)[0] for j, a in enumerate(z)]
    lad = [None if a is None else ar.inp(a, name='ln_a%d' % j)[0] for j, a in enumerate(la)]
    lbd = [None if a is None else ar.inp(a, name='ln_b%d' % j)[0] for j, a in enumerate(lb)]
    (gd, _), (dod, _) = ar.inp(gate, name='gate'), ar.inp(dout, name='dout')
    arr = lambda ts: (C.c_void_p * len(ts))(*[L.fptr(t) for t in ts])
    T = lambda a: torch.from_numpy(a).double()
    outs = [T(zj) if a is None else layer_norm_ref(zj, a, b, eps) for zj, a, b in zip(z, la, lb)]
    # node_mix
    od, ov = ar.out((M, d), name='out')
    L.check(lib.mmnas_node_mix_fwd(arr(zd), arr(lad), arr(lbd), n, L.fptr(gd), L.fptr(od), M, d, eps, L.stream()))
    ar.check()
    assert rel_err(cpu(ov), sum(float(gate[j]) * outs[j] for j in range(n)).numpy()) < 2e-6
    dgd, dgv = ar.inout(np.full(n, 0.25, np.float32), name='dgate')
    dad, dav = ar.out((M, d), name='d_active')
    ws, _ = ar.scratch_floats(lib.mmnas_mixed_sum_ws_floats(), name='ws')
    L.check(lib.mmnas_node_mix_bwd(arr(zd), arr(lad), arr(lbd), n, L.fptr(gd), L.fptr(dod), L.fptr(dad), active, L.fptr(dgd), L.fptr(ws),
                                   M, d, eps, L.stream()))
    ar.check()
    assert rel_err(cpu(dgv), np.array([float((T(dout) * o).sum()) for o in outs]) + 0.25) < 1e-5
    assert rel_err(cpu(dav), (float(gate[active]) * T(dout)).numpy()) < 1e-6
    # mixed_sum over the same tensors; candidate 2 takes no part (NULL)
    cand = [zd[0], zd[1], None]
    sd, sv = ar.out((M, d), name='sum')
    L.check(lib.mmnas_mixed_sum_fwd(arr(cand), n, L.fptr(gd), L.fptr(sd), M * d, L.stream()))
    ar.check()
    assert rel_err(cpu(sv), (float(gate[0]) * T(z[0]) + float(gate[1]) * T(z[1])).numpy()) < 1e-6
    dg2d, dg2v = ar.inout(zeros(n), name='dgate2')
    da2d, da2v = ar.out((M, d), name='d_active2')
    ws2, _ = ar.scratch_floats(lib.mmnas_mixed_sum_ws_floats(), name='ws2')
    L.check(lib.mmnas_mixed_sum_bwd(arr(cand), n, L.fptr(gd), L.fptr(dod), L.fptr(da2d), active, L.fptr(dg2d), L.fptr(ws2), M * d, L.stream()))
    ar.check()
    assert rel_err(cpu(dg2v), np.array([float((T(dout) * T(z[0])).sum()), float((T(dout) * T(z[1])).sum()), 0.0])) < 1e-5
    assert rel_err(cpu(da2v), (float(gate[active]) * T(dout)).numpy()) < 1e-6


@pytest.mark.parametrize('B,S,F', [(1, 1, 8), (3, 5, 24)])        # (S = 1, F = 8: the smallest mmnas_vgd_head_supported accepts)
def test_vgd_head(ar, B, S, F):
    """Raw scores (log_softmax = 0).  Bound: test_vgd_head_gpu.py's 1e-3 on every output and gradient."""
    L = _L()
    lib = L.lib()
    from oracle.mmnas_oracle import _linear, layer_norm
    assert lib.mmnas_vgd_head_supported(S, F) == 1
    rs = np.random.RandomState(10 * S + F)
    t = dict(yf=rnd(rs, B, S, F), xp=rnd(rs, B, F), ln_a=1 + 0.1 * rnd(rs, F), ln_b=0.1 * rnd(rs, F), Ws=rnd(rs, 1, F) * F ** -0.5,
             bs=0.1 * rnd(rs, 1), Wr=rnd(rs, 4, F) * F ** -0.5, br=0.1 * rnd(rs, 4))
    t = {k: v.astype(np.float32) for k, v in t.items()}
    gs, gr = rnd(rs, B, S), rnd(rs, B, S, 4)
    dv = {k: ar.inp(v, name=k)[0] for k, v in t.items()}
    (scd, scv), (rgd, rgv) = ar.out((B, S), name='scores'), ar.out((B, S, 4), name='reg')
    (mnd, _), (rsd, _) = ar.out((B, S), name='mean'), ar.out((B, S), name='rstd')
    L.check(lib.mmnas_vgd_head_fwd(*[L.fptr(dv[k]) for k in ('yf', 'xp', 'ln_a', 'ln_b', 'Ws', 'bs', 'Wr', 'br')], L.fptr(scd), L.fptr(rgd),
                                   L.fptr(mnd), L.fptr(rsd), B, S, F, 1e-6, 0, L.stream()))
    ar.check()
    p = {k: torch.from_numpy(v).double().requires_grad_() for k, v in t.items()}
    xy = layer_norm(p['xp'].unsqueeze(1) + p['yf'], p['ln_a'], p['ln_b'], 1e-6)
    scores, reg = _linear(xy, p['Ws'], p['bs']).squeeze(-1), _linear(xy, p['Wr'], p['br'])
    ((scores * torch.from_numpy(gs).double()).sum() + (reg * torch.from_numpy(gr).double()).sum()).backward()
    assert rel_err(cpu(scv), scores.detach().numpy()) < TOL and rel_err(cpu(rgv), reg.detach().numpy()) < TOL
    (gsd, _), (grd, _) = ar.inp(gs, name='dscores'), ar.inp(gr, name='dreg')
    outs = {k: ar.out(sh, name='d' + k) for k, sh in (('yf', (B, S, F)), ('xp', (B, F)), ('ln_a', (F,)), ('ln_b', (F,)), ('Ws', (1, F)),
                                                      ('bs', (1,)), ('Wr', (4, F)), ('br', (4,)))}
    ws, _ = ar.scratch_floats(lib.mmnas_vgd_head_bwd_ws_floats(B, S, F), name='ws')
    L.check(lib.mmnas_vgd_head_bwd(L.fptr(gsd), L.fptr(grd), *[L.fptr(dv[k]) for k in ('yf', 'xp', 'ln_a', 'ln_b', 'Ws', 'Wr')], None,
                                   L.fptr(mnd), L.fptr(rsd), *[L.fptr(outs[k][0]) for k in ('yf', 'xp', 'ln_a', 'ln_b', 'Ws', 'bs', 'Wr', 'br')],
                                   L.fptr(ws), B, S, F, 1e-6, 0, L.stream()))
    ar.check()
    for k, (_, v) in outs.items():
        assert rel_err(cpu(v), p[k].grad.numpy()) < TOL, k


@pytest.mark.parametrize('S', [1, 2, 9])
@pytest.mark.parametrize('k', [3, 11])
@pytest.mark.parametrize('d', [4, 260])
def test_conv_building_blocks(ar, S, k, d):
    """im2col / col2im / pad_seq / depthwise stencil.  pad_seq's rows from B * Sp on are slack the overlapping rows of the last
    sequence read (include/mmnas_hip.h): they are payload here -- written, with zeros."""
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(S + k + d)
    B, h = 2, k // 2
    x, dcol = rnd(rs, B, S, d), rnd(rs, B, S, k * d)
    w, bias, dy = rnd(rs, d, k), 0.1 * rnd(rs, d), rnd(rs, B, S, d)
    dw0, db0 = rnd(rs, d, k), rnd(rs, d)
    (xd, _), (dcd, _), (wd, _), (bd, _), (dyd, _) = (ar.inp(a, name=n) for a, n in ((x, 'x'), (dcol, 'dcol'), (w, 'w'), (bias, 'bias'), (dy, 'dy')))
    (cd, cv), (d2d, d2v) = ar.out((B, S, k * d), name='col'), ar.out((B, S, d), name='dx_col2im')
    Sp, rows = S + 2 * h, B * (S + 2 * h) + k
    ppd, ppv = ar.out((rows, d), name='xp')
    (yd, yv), (dxd, dxv) = ar.out((B, S, d), name='y'), ar.out((B, S, d), name='dx')
    (dwd, dwv), (dbd, dbv) = ar.inout(dw0, name='dw'), ar.inout(db0, name='db')
    L.check(lib.mmnas_im2col_seq(L.fptr(xd), L.fptr(cd), B, S, d, k, L.stream()))
    L.check(lib.mmnas_col2im_seq(L.fptr(dcd), L.fptr(d2d), B, S, d, k, L.stream()))
    L.check(lib.mmnas_pad_seq(L.fptr(xd), L.fptr(ppd), B, S, d, h, Sp, rows, L.stream()))
    L.check(lib.mmnas_dwconv_seq_fwd(L.fptr(xd), L.fptr(wd), L.fptr(bd), L.fptr(yd), B, S, d, k, L.stream()))
    L.check(lib.mmnas_dwconv_seq_bwd(L.fptr(xd), L.fptr(wd), L.fptr(dyd), L.fptr(dxd), L.fptr(dwd), L.fptr(dbd), B, S, d, k, L.stream()))
    ar.check()
    xpad = np.pad(x, ((0, 0), (h, h), (0, 0)))
    col = np.concatenate([xpad[:, t:t + S] for t in range(k)], -1)            # col[b, s, t * d + c] = x[b, s + t - k / 2, c]
    assert np.array_equal(cpu(cv), col)
    adj = np.zeros((B, S + 2 * h, d))
    for t in range(k):
        adj[:, t:t + S] += dcol[:, :, t * d:(t + 1) * d].astype(np.float64)
    assert rel_err(cpu(d2v), adj[:, h:h + S]) < 1e-6
    want = np.zeros((rows, d), np.float32)
    want[:B * Sp] = xpad.reshape(B * Sp, d)
    assert np.array_equal(cpu(ppv), want)
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, bias))
    r = torch.nn.functional.conv1d(xt.transpose(1, 2), wt.unsqueeze(1), bt, padding=h, groups=d).transpose(1, 2)
    r.backward(torch.from_numpy(dy).double())
    assert rel_err(cpu(yv), r.detach().numpy()) < 1e-5                     # (test_conv_building_blocks' bounds)
    assert rel_err(cpu(dxv), xt.grad.numpy()) < 1e-4
    assert rel_err(cpu(dwv), dw0 + wt.grad.numpy()) < 1e-4 and rel_err(cpu(dbv), db0 + bt.grad.numpy()) < 1e-4


@pytest.mark.parametrize('B,T,H', [(2, 1, 64), (70, 3, 64)])
def test_lstm_seq(ar, B, T, H):
    """The persistent LSTM on the direct ABI: xp = x W_ih^T + b_ih is the input; float64 recurrence in nn.LSTM's gate order
    (i, f, g, o); DG = the gradient of the pre-activations.  Bounds of test_lstm_vs_torch_fp64 (2e-5 / 1e-4)."""
    L = _L()
    lib = L.lib()
    assert lib.mmnas_lstm_seq_supported(H, B) == 1
    rs = np.random.RandomState(B + T + H)
    xp, bhh, Whh, dout = rnd(rs, B, T, 4 * H), 0.1 * rnd(rs, 4 * H), rnd(rs, 4 * H, H) / np.float32(np.sqrt(H)), rnd(rs, B, T, H)
    (xpd, _), (bd, _), (Wd, _), (dod, _) = ar.inp(xp, name='xp'), ar.inp(bhh, name='bhh'), ar.inp(Whh, name='Whh'), ar.inp(dout, name='dout')
    (hpd, hpv), (csd, csv), (gad, _), (od, ov) = (ar.out(sh, name=n) for sh, n in (((B, T, H), 'Hprev'), ((B, T, H), 'Cs'),
                                                                                 ((B, T, 4 * H), 'Gall'), ((B, T, H), 'out')))
    L.check(lib.mmnas_lstm_seq_fwd(L.fptr(xpd), L.fptr(bd), L.fptr(Wd), L.fptr(hpd), L.fptr(csd), L.fptr(gad), L.fptr(od), T, B, H, L.stream()))
    assert lib.mmnas_lstm_seq_timed_out(L.stream()) == 0
    ar.check()
    xt = torch.from_numpy(xp).double().requires_grad_(True)
    Wt, bt = torch.from_numpy(Whh).double(), torch.from_numpy(bhh).double()
    h, c, hs, cs = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64), [], []
    for t_ in range(T):
        i, f, g, o = (xt[:, t_] + h @ Wt.t() + bt).chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h); cs.append(c)
    y = torch.stack(hs, 1)
    y.backward(torch.from_numpy(dout).double())
    assert rel_err(cpu(ov), y.detach().numpy()) < 2e-5 and rel_err(cpu(csv), torch.stack(cs, 1).detach().numpy()) < 2e-5
    hprev = torch.cat([torch.zeros(B, 1, H, dtype=torch.float64), y.detach()[:, :-1]], 1)
    assert rel_err(cpu(hpv), hprev.numpy()) < 2e-5
    dgd, dgv = ar.out((B, T, 4 * H), name='DG')
    L.check(lib.mmnas_lstm_seq_bwd(L.fptr(dod), L.fptr(Wd), L.fptr(csd), L.fptr(gad), L.fptr(dgd), T, B, H, L.stream()))
    assert lib.mmnas_lstm_seq_timed_out(L.stream()) == 0
    ar.check()
    assert rel_err(cpu(dgv), xt.grad.numpy()) < 1e-4


@pytest.mark.parametrize('n', [1, 255, 10007])
def test_adam_sgd_sumsq(ar, n):
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(n)
    p0, g0, m0, v0, b0 = rnd(rs, n), rnd(rs, n) * 3, 0.1 * rnd(rs, n), np.abs(rnd(rs, n)), rnd(rs, n)
    gd, _ = ar.inp(g0, name='g')
    ssd, ssv = ar.inout(zeros(1), name='sumsq')
    L.check(lib.mmnas_sumsq(L.fptr(gd), n, L.fptr(ssd), L.stream()))
    ar.check()
    ss = float((g0.astype(np.float64) ** 2).sum())
    assert abs(float(cpu(ssv)[0]) - ss) < 1e-3 * ss                   # (test_pack_adam_sumsq's bound)
    # Adam, step 2, clipped through the device scalar
    (pd, pv), (md, mv), (vd, vv) = ar.inout(p0, name='p'), ar.inout(m0, name='m'), ar.inout(v0, name='v')
    lr, b1, b2, eps, step = 1e-3, 0.9, 0.98, 1e-9, 2
    L.check(lib.mmnas_adam_step(L.fptr(pd), L.fptr(gd), L.fptr(md), L.fptr(vd), n, lr, b1, b2, eps, 0.0, L.fptr(ssd), 1.0, step, L.stream()))
    ar.check()
    g = g0.astype(np.float64) * min(1.0, 1.0 / (np.sqrt(float(np.float32(ss))) + 1e-6))
    m = b1 * m0.astype(np.float64) + (1 - b1) * g
    v = b2 * v0.astype(np.float64) + (1 - b2) * g * g
    want = p0 - lr / (1 - b1 ** step) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)
    assert rel_err(cpu(pv), want) < 1e-5 and rel_err(cpu(mv), m) < 1e-5 and rel_err(cpu(vv), v) < 1e-5
    # SGD with momentum, weight decay, nesterov
    (qd, qv), (bfd, bfv) = ar.inout(p0, name='p_sgd'), ar.inout(b0, name='buf')
    mom, wd = 0.9, 1e-2
    L.check(lib.mmnas_sgd_step(L.fptr(qd), L.fptr(gd), L.fptr(bfd), n, 0.1, mom, 0.0, wd, 1, 0, None, 0.0, L.stream()))
    ar.check()
    gp = g0.astype(np.float64) + wd * p0
    buf = mom * b0 + gp
    assert rel_err(cpu(bfv), buf) < TOL and rel_err(cpu(qv), p0 - 0.1 * (gp + mom * buf)) < TOL      # (test_sgd_gpu.py's bound)


# ----------------------------------------------------------------------------- planned arenas (operator / chain / head level)
@pytest.fixture
def planned(monkeypatch):
    """ops._bytes (saved blocks, scratch and arenas sized by the *_plan() functions) and ops._ws_floats (the *_ws_floats()
    scratch) hand out Arena.scratch blocks of EXACTLY the requested size -- no 256-byte floor, no rounding -- while
    state['on'] is set."""
    from mmnas_amd import ops
    import sys
    arena = Arena(DEV, capacity=256 << 20)
    state = {'on': False, 'sites': []}       # sites: (helper, the autograd node that asked, forward / backward) per block
    real_bytes, real_ws = ops._bytes, ops._ws_floats

    def site(helper):
        f = sys._getframe(2)
        state['sites'].append((helper, type(f.f_locals.get('ctx')).__name__, f.f_code.co_name))
        return '%s#%d %s.%s' % ((helper, len(state['sites'])) + state['sites'][-1][1:])

    def _bytes(n, dev):
        if not state['on']:
            return real_bytes(n, dev)
        return arena.scratch(int(n), name='%s[%d]' % (site('_bytes'), n))[0]

    def _ws_floats(n, dev):
        if not state['on']:
            return real_ws(n, dev)
        return arena.scratch_floats(int(n), name='%s[%d]' % (site('_ws_floats'), n))[0]

    monkeypatch.setattr(ops, '_bytes', _bytes)
    monkeypatch.setattr(ops, '_ws_floats', _ws_floats)
    yield arena, state
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('GPU error in a guard-band case, the session ends here: %s' % e, returncode=3)


def _planned_equals_plain(planned, run, sites):
    """run() -> dict of arrays, once with the allocator's blocks and once with exact-size guarded ones: after the side
    stream's work has been joined every band is intact, and the results are the same bit for bit.  `sites`: the (helper,
    autograd node, direction) triples that must each have been handed a block -- the case really goes through them."""
    from mmnas_amd import ops
    arena, state = planned
    plain = run()
    state['on'] = True
    try:
        got = run()
        ops.join_side_stream()
        arena.check()
    finally:
        state['on'] = False
    missing = set(sites) - set(state['sites'])
    assert not missing, ('no block was handed out at', sorted(missing), 'handed out:', state['sites'])
    assert set(got) == set(plain)
    for k in plain:
        if plain[k] is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(got[k], plain[k]), (k, float(np.abs(got[k] - plain[k]).max()))


@pytest.mark.parametrize('name', ['self_att_64', 'guided_att_64', 'feed_forward'])
def test_planned_blocks_operator(planned, name):
    """One SelfAtt, GuidedAtt and feed-forward operator, forward + backward, at tests/test_ops_gpu.py's default dims."""
    from tests.golden import cases
    from tests.test_ops_gpu import run_hip_op
    case = cases.op_case(name, True, True, 11)
    node = 'MlpOpBackward' if name == 'feed_forward' else 'AttentionOpBackward'
    _planned_equals_plain(planned, lambda: run_hip_op(case), [('_bytes', node, 'forward'), ('_bytes', node, 'backward')])


def test_planned_blocks_rel_self_att_lazy_handle(planned):
    """RelSelfAtt fed a RelHandle (the scratch size depends on MMNAS_F_RELRAW), test_rel_self_att_with_lazy_handle's small dims."""
    from mmnas_amd.model.modules import RelHandle
    from mmnas_amd.utils.ops_adapter import OpsAdapter
    from tests.golden import cases
    dims = dict(B=3, Sx=7, Sy=5, HSIZE=128)
    case = cases.op_case('rel_self_att_64', True, True, 2024, dims)
    rs = np.random.RandomState(7)
    B, S = dims['B'], dims['Sx']
    raw = rnd(rs, B, S, S, 4)
    raw[:, S - 2:] = 0
    raw[:, :, S - 2:] = 0
    Wy, by = rnd(rs, 64, 4) / 2, 0.1 * rnd(rs, 64)

    def run():
        op = OpsAdapter().OPS['rel_self_att_64'](case['cfg'], norm=True, residual=True)
        op.load_state_dict({k: torch.from_numpy(v) for k, v in case['P'].items()})
        op = op.to(DEV).train()
        x = torch.from_numpy(case['x']).to(DEV).requires_grad_(True)
        Wyd, byd = torch.from_numpy(Wy).to(DEV).requires_grad_(True), torch.from_numpy(by).to(DEV).requires_grad_(True)
        h = RelHandle(torch.from_numpy(raw).to(DEV), Wyd, byd)
        out = op(x, None, torch.from_numpy(case['x_mask']).to(DEV), None, h)
        out.backward(torch.from_numpy(case['gout']).to(DEV))
        assert h._dense is None
        res = {'out': out.detach().cpu().numpy(), 'dx': x.grad.cpu().numpy(), 'dWy': Wyd.grad.cpu().numpy(), 'dby': byd.grad.cpu().numpy()}
        res.update({'g:' + k: p.grad.cpu().numpy() for k, p in op.named_parameters()})
        return res
    _planned_equals_plain(planned, run, [('_bytes', 'AttentionOpBackward', 'forward'), ('_bytes', 'AttentionOpBackward', 'backward')])


@pytest.mark.parametrize('unpad', [False, True], ids=['padded', 'ragged'])
def test_planned_blocks_backbone_chain_and_head(planned, unpad, monkeypatch):
    """One BackboneFn chain (padded and ragged decoder stream) and one HeadFn: the fixed-architecture VQA net through the flat
    gradient buffer, the smallest configuration tests/test_chain_gpu.py builds (B = 3, Sx = 6, Sy = 9, HSIZE = 128)."""
    from mmnas_amd import ops
    from tests.test_chain_gpu import _run_unpad
    heads, o_head = [], ops.HeadFn.apply
    monkeypatch.setattr(ops.HeadFn, 'apply', lambda *a: (heads.append(1), o_head(*a))[1])

    def run():
        del heads[:]
        out, grads, seen = _run_unpad('vqa', 'mmnas_vqa', False, unpad, B=3, Sy=9)
        assert seen == [unpad] and heads == [1], (seen, heads)        # one chain call (ragged or not) and one head call
        return dict(grads, out=out)
    _planned_equals_plain(planned, run, [('_bytes', 'BackboneFnBackward', 'forward'), ('_bytes', 'HeadFnBackward', 'forward')])


@pytest.mark.parametrize('which', ['glimpse1', 'layer_norm', 'grounding_head', 'mixed_sum'])
def test_planned_blocks_ws_floats_sites(planned, which):
    """The four *_ws_floats() scratch sites of ops.py behind their autograd functions, forward + backward."""
    from mmnas_amd import ops
    rs = np.random.RandomState(5)
    G = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).requires_grad_(True)

    def finish(outs, gouts, leaves):
        torch.autograd.backward(outs, [torch.from_numpy(g).to(DEV) for g in gouts])
        res = {'out%d' % i: o.detach().cpu().numpy() for i, o in enumerate(outs)}
        res.update({'g%d' % i: t.grad.cpu().numpy() for i, t in enumerate(leaves)})
        return res

    if which == 'glimpse1':         # nn.Linear with one output unit
        x, W, b, gy = rnd(rs, 37, 36), rnd(rs, 1, 36), rnd(rs, 1), rnd(rs, 37, 1)
        node = 'LinearFnBackward'

        def run():
            t = [G(x), G(W), G(b)]
            return finish([ops.linear(*t)], [gy], t)
    elif which == 'layer_norm':
        x, a, b, gy = rnd(rs, 37, 36), 1 + 0.1 * rnd(rs, 36), rnd(rs, 36), rnd(rs, 37, 36)
        node = 'LayerNormFnBackward'

        def run():
            t = [G(x), G(a), G(b)]
            return finish([ops.layer_norm(*t)], [gy], t)
    elif which == 'grounding_head':
        B, S, F = 3, 5, 24
        arrs = [rnd(rs, B, S, F), rnd(rs, B, F), 1 + 0.1 * rnd(rs, F), 0.1 * rnd(rs, F), rnd(rs, 1, F), rnd(rs, 1), rnd(rs, 4, F), rnd(rs, 4)]
        gs, gr = rnd(rs, B, S), rnd(rs, B, S, 4)
        node = 'GroundingHeadFnBackward'

        def run():
            t = [G(a) for a in arrs]
            return finish(list(ops.grounding_head(t[0], t[1], t[2], t[3], 1e-6, *t[4:])), [gs, gr], t)
    else:
        outs, gate, gy = [rnd(rs, 5, 7, 36) for _ in range(3)], rnd(rs, 3), rnd(rs, 5, 7, 36)
        node = 'MixedSumFnBackward'

        def run():
            t = [G(gate), G(outs[1])]
            lst = [torch.from_numpy(outs[0]).to(DEV), t[1], torch.from_numpy(outs[2]).to(DEV)]
            return finish([ops.mixed_sum(t[0], lst, 1)], [gy], t)
    _planned_equals_plain(planned, run, [('_ws_floats', node, 'backward')])
