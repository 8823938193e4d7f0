"""The degenerate-row LayerNorm cases (tests/ln_rows.py) without a GPU: the inputs are what they claim to be, the float32
module stays inside the bars the kernels are held to, and the closed form of oracle.layer_norm_backward -- which
test_layernorm pins the kernel to -- equals float64 autograd on every class, constant rows included."""
import numpy as np
import pytest
import torch

from oracle import mmnas_oracle as O
from tests import ln_rows as LR

WIDTHS = (4, 8, 36, 256, 260, 512, 516, 1024, 1028, 2048)     # every width the GPU module uses


@pytest.mark.parametrize('d', WIDTHS)
def test_const_rows_have_sd_exactly_zero_in_any_summation_order(d):
    """c * k is representable in float32 for every k <= d, so every partial sum of a constant row is exact whatever the
    order, and (c * d) / d == c: mean == c, every centred value and the sum of squares are exactly 0."""
    k = np.arange(1, d + 1, dtype=np.float64)
    for c in LR.CONSTS:
        assert np.array_equal((np.float32(c) * k.astype(np.float32)).astype(np.float64), c * k), c
        assert np.float32(c * d) / np.float32(d) == np.float32(c)
    x = LR.rows('const', 12, d)
    assert sorted(set(x[:, 0].tolist())) == sorted(LR.CONSTS) and bool((x == x[:, :1]).all())
    assert float(T32(x).std(-1).abs().max()) == 0.0


def T32(a):
    return torch.from_numpy(np.asarray(a, np.float32))


def test_classes_are_what_they_claim():
    d = 256
    sd = {c: LR.rows(c, 16, d).astype(np.float64).std(-1, ddof=1) for c in LR.CLASSES}
    assert (sd['const'] == 0).all()
    assert 0.5 * LR.EPS < sd['sd_eps'].min() and sd['sd_eps'].max() < 2 * LR.EPS
    assert sd['sd_tiny'].max() < LR.EPS / 64
    assert abs(LR.rows('offset', 16, d).mean() - 64) < 0.1
    big = LR.rows('big', 16, 2048).astype(np.float64)
    assert np.isfinite(np.float32(((big - big.mean(-1, keepdims=True)) ** 2).sum(-1).max()))       # d * 1e30 stays in range
    assert float((LR.rows('small', 16, d).astype(np.float64) ** 2).min()) > 0 and sd['small'].max() < 2e-12
    assert bool(((LR.rows('outlier', 16, d) == 1e4).sum(-1) == 1).all())
    x, which = LR.interleaved(2053, 36)
    assert x.shape == (2053, 36) and np.array_equal(x[which == 1], LR.rows('const', 257, 36)[:int((which == 1).sum())])
    assert np.array_equal(LR.rows('randn', 5, 36, 3), LR.rows('randn', 5, 36, 3))


@pytest.mark.parametrize('d', WIDTHS)
def test_float32_module_is_finite_and_inside_the_bars(d):
    """The reference module in float32 torch against its float64 run: finite everywhere (constant rows too), inside the
    project's bars on every class but `offset`, and on `offset` within the 1e-5 measured for d = 4 .. 2048 (x 2)."""
    R, p = 6, 0.2
    a, b = LR.params(d)
    gy = LR.grad_out(R, d)
    mask = (np.random.RandomState(d).random_sample((R, d)) >= p) / (1 - p)
    for cls in LR.CLASSES:
        x = LR.rows(cls, R, d)
        r64 = LR.ln_reference(x, a, b, gy, mask)
        r32 = LR.ln_reference(x, a, b, gy, mask, dtype=torch.float32)
        for name in r64:
            assert np.isfinite(r32[name]).all() and np.isfinite(r64[name]).all(), (cls, name)
            e = LR.err(r32[name], r64[name])
            if cls == 'offset':
                assert e <= 2e-5, (cls, name, e)
                assert LR.bars(cls, r64, r32)[name] == (max(LR.project_bar(name), 4 * e), e)
            else:
                assert e <= LR.project_bar(name), (cls, name, e)
        if cls == 'const':       # dx = (g - mean(g)) / eps: std's backward is masked where std == 0
            g = gy.astype(np.float64) * a.astype(np.float64)
            assert LR.err(r64['dx'], (g - g.mean(-1, keepdims=True)) / LR.EPS) < 1e-12


@pytest.mark.parametrize('d', WIDTHS)
def test_oracle_closed_form_equals_float64_autograd_on_every_class(d):
    R = 6
    a, b = LR.params(d)
    gy = LR.grad_out(R, d)
    for cls in LR.CLASSES:
        x = LR.rows(cls, R, d)
        ref = LR.ln_reference(x, a, b, gy)
        X, A, G = (torch.from_numpy(v).double() for v in (x, a, gy))
        y = O.layer_norm(X, A, torch.from_numpy(b).double())
        dx, da, db = O.layer_norm_backward(X, A, G)
        for name, got in (('y', y), ('dx', dx), ('da', da), ('db', db)):
            assert bool(torch.isfinite(got).all()), (cls, name)
            assert LR.err(got.numpy(), ref[name]) <= 1e-12, (cls, name, LR.err(got.numpy(), ref[name]))


def test_judge_names_the_kernel_the_class_and_the_row(monkeypatch):
    monkeypatch.setattr(LR, 'STATS', {})
    ref = {'dx': np.ones((4, 8)), 'y': np.ones((4, 8))}
    got = {'dx': np.ones((4, 8)), 'y': np.ones((4, 8))}
    got['dx'][2, 3] = np.nan
    with pytest.raises(AssertionError, match=r'some_kernel: dx is not finite on class const: 1 of 32 elements, first in row 2'):
        LR.judge('some_kernel', 'const', got, ref)
    got['dx'][2, 3] = 1.0
    got['y'][3, 0] = 1.0 + 1e-4
    with pytest.raises(AssertionError, match=r'some_kernel: y on class randn: error 1.000e-04 above the bar 1.000e-05 \(worst in row 3\)'):
        LR.judge('some_kernel', 'randn', got, ref)
    with pytest.raises(AssertionError, match='float32 module'):
        LR.judge('some_kernel', 'offset', got, ref)
