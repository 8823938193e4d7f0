"""The grid-stride kernels of rowops.hip and util.hip behind their first pass: eltwise forward / backward (kinds 0..3), glu
forward / backward and drop_add at lengths on both sides of one workgroup and past the 2048 x 256 = 524 288 threads of the
capped grid, where the second pass -- and with it the dropout index (uint32_t)i of glu and drop_add -- is first used; sumsq past
its 1024 x 256 threads with the float4 body and the scalar tail; colsum at every split its launcher chooses, with ldx > N.

Outputs start as NaN, so an element that no pass wrote shows up, and carry three guard elements behind them.

  * kind 0 of a finite input is exactly 0 (or -0), forward and backward; kinds 1 and 2 are exact against their numpy float32
    statement (one comparison, at most one product: nothing to round differently);
  * GELU (kind 3) is judged as |err| <= bar max(1, |x|) against the float64 reference of tests/kernel_refs.py, the backward as
    |err| <= bar max(1, |x|) |dy|; bar = 4 x what the numpy float32 restatement of the same tanh formula reaches against
    float64 on the largest case's inputs (measured on the host that wrote this: 1.1e-7 forward, 2.3e-7 backward).  Above
    |x| ~ 5e19 the backward's x * x overflows and the formula yields NaN, as torch's own float32 kernel does; activations never
    get there, the inputs here stop at 1e4, and nothing is asserted about it;
  * drop_add is exact against oracle.dropout_rng.scaled_mask at p = 0 and p = 0.5 (the multiplier 2 rounds nothing, so a
    contracted multiply-add gives the same bits), with and without the residual;
  * glu follows GELU's rule against glu_ref: |err| <= bar max(1, |a|) forward, bar max(1, |a|) |dy| backward (both halves of
    dh), a the value half of h; bar = 4 x the numpy float32 restatement's worst on the largest shape at the same relu and p.
    Gate inputs include +-30 and +-100, where expf(-b) overflows to inf.  Forward and backward are each held to the reference
    under the one mask of oracle.dropout_rng.scaled_mask, and must be exactly 0 on the same elements;
  * colsum per column against the float64 sum, |err| <= bar (|out0| + sum |x|): out starts as a nonzero vector (the contract
    is +=), the slack columns of ldx > N hold NaN;
  * sumsq relative against float64, the output word pre-set (+=), aligned and one float off, each case run twice (the kernels
    add with atomics: no two runs need agree in bits).
  colsum's and sumsq's bar: 4 x max(what a float32 pairwise sum (numpy's) reaches on the same data, 2^-24).  The floor is the
  unit roundoff of the format: any float32 evaluation may commit it in its last addition alone, while the pairwise sum of a
  few elements often commits nothing, which measures luck and not the format.

Found with this test: mmnas_sumsq stood 5.9e-7 from float64 (bar 2.4e-7) at 1 048 576 + 1203 elements one float off alignment --
up to 1024 workgroups each added their partial to the word with a float atomic.  It now adds the partials in double, once.

When MMNAS_STREAM_KERNEL_STATS names a file, the worst figures met are written there at the end of the module
(profiles/r15_stream_kernel_error_stats.json is one such run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.kernel_refs import eltwise_ref, glu_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 3
SENTINEL = 7777.0
F32 = np.float32
WRAP = 524288 + 259
FIXED = np.array([0.0, -0.0, 1e-30, -1e-30, 5, -5, 12, -12, 50, -50, 1e4, -1e4], F32)
K0, K1 = F32(0.7978845608028654), F32(0.044715)
U32 = 2.0 ** -24

ERR = {}     # label -> worst value met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_STREAM_KERNEL_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)
            f.write('\n')


def _inputs(n, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(n).astype(F32)
    k = min(n, FIXED.size)
    x[rs.permutation(n)[:k]] = FIXED[:k]
    return x, rs.standard_normal(n).astype(F32)


def _out(n):
    t = torch.full((n + GUARD,), float('nan'), device=DEV)
    t[n:] = SENTINEL
    return t


def _read(t, n, what):
    a = t.cpu().numpy()
    assert np.all(a[n:] == SENTINEL), (what, 'guard elements written')
    assert not np.isnan(a[:n]).any(), (what, 'elements left unwritten', int(np.isnan(a[:n]).sum()))
    return a[:n]


def _gelu32(x, dy):
    """act_fwd / act_bwd of rowops.hip, kind 3, in numpy float32."""
    u = K0 * (x + K1 * x * x * x)
    t = np.tanh(u)
    y = F32(0.5) * x * (F32(1) + t)
    d = F32(0.5) * (F32(1) + t) + F32(0.5) * x * (F32(1) - t * t) * K0 * (F32(1) + F32(3) * K1 * x * x)
    assert y.dtype == F32 and d.dtype == F32
    return y, dy * d


def _gelu_measures(y, dx, x, dy, ry, rdx):
    sx = np.maximum(1.0, np.abs(x.astype(np.float64)))
    return (float(np.max(np.abs(y.astype(np.float64) - ry) / sx)),
            float(np.max(np.abs(dx.astype(np.float64) - rdx) / (sx * np.maximum(np.abs(dy.astype(np.float64)), 1e-30)))))


_BARS = {}


def _gelu_bars():
    if not _BARS:
        x, dy = _inputs(WRAP, WRAP)
        ry, rdx = eltwise_ref(3, x, dy)
        e = _gelu_measures(*_gelu32(x, dy), x, dy, ry.numpy(), rdx.numpy())
        _BARS['fwd'], _BARS['bwd'] = 4 * e[0], 4 * e[1]
        assert 0 < _BARS['fwd'] < 2e-6 and 0 < _BARS['bwd'] < 4e-6, _BARS
    return _BARS


@pytest.mark.parametrize('n', [1, 255, 256, 257, WRAP])
def test_eltwise_forward_and_backward(n):
    import mmnas_amd._lib as L
    x, dy = _inputs(n, n)
    xd, dyd = torch.from_numpy(x).to(DEV), torch.from_numpy(dy).to(DEV)
    for kind in range(4):
        y, dx = _out(n), _out(n)
        L.check(L.lib().mmnas_eltwise_fwd(kind, L.fptr(xd), L.fptr(y), n, L.stream()))
        L.check(L.lib().mmnas_eltwise_bwd(kind, L.fptr(xd), L.fptr(dyd), L.fptr(dx), n, L.stream()))
        y, dx = _read(y, n, ('fwd', kind)), _read(dx, n, ('bwd', kind))
        if kind == 0:
            assert np.all(y == 0) and np.all(dx == 0)
        elif kind == 1:
            assert np.array_equal(y, np.maximum(x, F32(0)))
            assert np.array_equal(dx, dy * (x > 0).astype(F32))
        elif kind == 2:
            assert np.array_equal(y, np.where(x > 0, x, F32(0.01) * x))
            assert np.array_equal(dx, dy * np.where(x > 0, F32(1), F32(0.01)))
        else:
            bar = _gelu_bars()
            ry, rdx = eltwise_ref(3, x, dy)
            ef, eb = _gelu_measures(y, dx, x, dy, ry.numpy(), rdx.numpy())
            _note('gelu|fwd', ef); _note('gelu|bwd', eb)
            print('gelu n=%d: forward %.3g (bar %.3g), backward %.3g (bar %.3g)' % (n, ef, bar['fwd'], eb, bar['bwd']))
            assert ef <= bar['fwd'] and eb <= bar['bwd'], (ef, eb, bar)


@pytest.mark.parametrize('n', [1, 2560, WRAP])
@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_drop_add_is_exact(n, with_res, p):
    import mmnas_amd._lib as L
    from oracle import dropout_rng
    x, res = _inputs(n, n + 1)
    seed, site = 0x1234567, 3
    xd = torch.from_numpy(x).to(DEV)
    rd = torch.from_numpy(res).to(DEV) if with_res else None
    y = _out(n)
    L.check(L.lib().mmnas_drop_add(L.fptr(xd), L.fptr(rd), L.fptr(y), n, p, seed, site, L.stream()))
    want = x * dropout_rng.scaled_mask(seed, site, (n,), p)
    if with_res:
        want = res + want
    assert want.dtype == F32
    assert np.array_equal(_read(y, n, 'drop_add'), want)


# ---------------------------------------------------------------------------------------------------------------- glu
GLU_SHAPES = [(1, 1), (3, 5), (60, 128), (1031, 509)]       # the last: 524 779 elements, an odd C under i / C
GLU_SEED, GLU_SITE = 4242, 2


def _glu_inputs(M, C):
    rs = np.random.RandomState(M * 1000 + C)
    h = rs.standard_normal((M, 2 * C)).astype(F32)
    fixed = np.array([30, -30, 100, -100], F32)
    k = min(M * C, fixed.size)
    where = rs.permutation(M * C)[:k]
    h[where // C, C + where % C] = fixed[:k]
    return h, rs.standard_normal((M, C)).astype(F32)


def _glu32(h, dy, relu, mult):
    """glu_fwd_kernel / glu_bwd_kernel of rowops.hip in numpy float32; mult: the dropout multiplier per element or None."""
    C = h.shape[1] // 2
    a, b = h[:, :C], h[:, C:]
    with np.errstate(over='ignore', under='ignore'):
        en = np.exp(-b)
        y = a / (F32(1) + en)
        sg = F32(1) / (F32(1) + en)
        if relu:
            y = np.maximum(y, F32(0))
        g = dy
        if mult is not None:
            y, g = y * mult, g * mult
        if relu:
            g = np.where(a * sg > 0, g, F32(0))
        dh = np.concatenate([g * sg, g * a * sg * (F32(1) - sg)], 1)
    assert y.dtype == F32 and dh.dtype == F32
    return y, dh


def _glu_measures(y, dh, h, dy, ry, rdh):
    C = h.shape[1] // 2
    sa = np.maximum(1.0, np.abs(h[:, :C].astype(np.float64)))
    sd = sa * np.maximum(np.abs(dy.astype(np.float64)), 1e-30)
    return (float(np.max(np.abs(y.astype(np.float64) - ry) / sa)),
            float(np.max(np.abs(dh.astype(np.float64) - rdh) / np.concatenate([sd, sd], 1))))


def _glu_case(M, C, relu, p):
    from oracle import dropout_rng
    h, dy = _glu_inputs(M, C)
    mult = dropout_rng.scaled_mask(GLU_SEED, GLU_SITE, (M, C), p) if p > 0 else None
    ry, rdh = glu_ref(h, dy, relu=bool(relu), dmask=mult)
    return h, dy, mult, ry.numpy(), rdh.numpy()


_GLU_BARS = {}


def _glu_bars(relu, p):
    if (relu, p) not in _GLU_BARS:
        h, dy, mult, ry, rdh = _glu_case(*GLU_SHAPES[-1], relu, p)
        e = _glu_measures(*_glu32(h, dy, relu, mult), h, dy, ry, rdh)
        assert 0 < e[0] < 1e-6 and 0 < e[1] < 1e-6, e
        _GLU_BARS[(relu, p)] = (4 * e[0], 4 * e[1])
    return _GLU_BARS[(relu, p)]


@pytest.mark.parametrize('p', [0.0, 0.3])
@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('M,C', GLU_SHAPES)
def test_glu_forward_and_backward(M, C, relu, p):
    import mmnas_amd._lib as L
    h, dy, mult, ry, rdh = _glu_case(M, C, relu, p)
    bar = _glu_bars(relu, p)
    hd, dyd = torch.from_numpy(h).to(DEV), torch.from_numpy(dy).to(DEV)
    y, dh = _out(M * C), _out(2 * M * C)
    L.check(L.lib().mmnas_glu_fwd(L.fptr(hd), L.fptr(y), M, C, relu, p, GLU_SEED, GLU_SITE, L.stream()))
    L.check(L.lib().mmnas_glu_bwd(L.fptr(hd), L.fptr(dyd), L.fptr(dh), M, C, relu, p, GLU_SEED, GLU_SITE, L.stream()))
    y, dh = _read(y, M * C, 'glu fwd').reshape(M, C), _read(dh, 2 * M * C, 'glu bwd').reshape(M, 2 * C)
    ef, eb = _glu_measures(y, dh, h, dy, ry, rdh)
    _note('glu|fwd', ef); _note('glu|bwd', eb)
    print('glu %dx%d relu %d p %g: forward %.3g (bar %.3g), backward %.3g (bar %.3g)' % (M, C, relu, p, ef, bar[0], eb, bar[1]))
    assert ef <= bar[0] and eb <= bar[1], (ef, eb, bar)
    if mult is not None:      # one mask on both sides, behind the wrap too
        dropped = mult == 0
        assert not y[dropped].any() and not dh[:, :C][dropped].any() and not dh[:, C:][dropped].any()


# ---------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize('M,N,ldx', [(1, 1, 1), (3, 65, 65), (65, 300, 300), (777, 300, 333), (4097, 64, 64), (130, 70000, 70000)])
def test_colsum_adds_the_column_sums(M, N, ldx):
    import mmnas_amd._lib as L
    rs = np.random.RandomState(M + N)
    x = np.full((M, ldx), np.nan, F32)
    x[:, :N] = rs.standard_normal((M, N)).astype(F32)
    out0 = (3.0 + rs.standard_normal(N)).astype(F32)
    xs = x[:, :N]
    ref = out0.astype(np.float64) + xs.astype(np.float64).sum(0)
    scale = np.abs(out0).astype(np.float64) + np.abs(xs).astype(np.float64).sum(0)
    pair = out0 + np.ascontiguousarray(xs.T).sum(1, dtype=F32)       # (a contiguous axis: numpy adds it pairwise)
    assert pair.dtype == F32
    bar = 4 * max(float(np.max(np.abs(pair.astype(np.float64) - ref) / scale)), U32)
    out = torch.full((N + GUARD,), SENTINEL, device=DEV)
    out[:N] = torch.from_numpy(out0).to(DEV)
    xd = torch.from_numpy(x).to(DEV)
    L.check(L.lib().mmnas_colsum(L.fptr(xd), L.fptr(out), M, N, ldx, L.stream()))
    got = out.cpu().numpy()
    assert np.all(got[N:] == SENTINEL), 'guard elements written'
    e = float(np.max(np.abs(got[:N].astype(np.float64) - ref) / scale))
    _note('colsum', e); _note('colsum|share_of_bar', e / bar)
    print('colsum %dx%d ldx %d: %.3g (bar %.3g)' % (M, N, ldx, e, bar))
    assert e <= bar, (e, bar)


# ---------------------------------------------------------------------------------------------------------------- sumsq
@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 4, 5, 1027, 1048576 + 1203])
def test_sumsq_adds_the_sum_of_squares(n, off):
    import mmnas_amd._lib as L
    rs = np.random.RandomState(n + off)
    g = (3.0 * rs.standard_normal(n)).astype(F32)
    out0 = F32(2.5)
    ref = float(out0) + float((g.astype(np.float64) ** 2).sum())
    pair = out0 + (g * g).sum(dtype=F32)
    assert pair.dtype == F32
    bar = 4 * max(abs(float(pair) - ref) / ref, U32)
    buf = torch.full((off + n + GUARD,), float('nan'), device=DEV)
    buf[off:off + n] = torch.from_numpy(g).to(DEV)
    gd = buf[off:off + n]
    assert gd.data_ptr() % 16 == 4 * off
    for run in range(2):
        word = torch.full((1 + GUARD,), SENTINEL, device=DEV)
        word[0] = float(out0)
        L.check(L.lib().mmnas_sumsq(L.fptr(gd), n, L.fptr(word), L.stream()))
        got = word.cpu().numpy()
        assert np.all(got[1:] == SENTINEL), 'guard elements written'
        e = abs(float(got[0]) - ref) / ref
        _note('sumsq', e); _note('sumsq|share_of_bar', e / bar)
        print('sumsq n=%d offset=%d run %d: %.3g (bar %.3g)' % (n, off, run, e, bar))
        assert e <= bar, (n, off, run, e, bar)
