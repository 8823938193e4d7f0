"""The bars of tests/adam_cases.py, shown on the CPU to do their work before a GPU is involved: for every betas setting, weight
decay and clip the float32 restatement of mmnas_adam_step's arithmetic -- coefficients formed in double from the decimals,
rounded once -- meets them against torch.optim.Adam in float64 at every length the GPU test runs, and the same restatement
with float-formed coefficients (1.f - beta, powf) exceeds the v bar wherever beta2 = 0.999: 1 - 0.999f is 1.29e-5 from 0.001."""
import numpy as np
import pytest

from tests import adam_cases as A

SETTINGS = [(b, wd, clip) for b in A.BETAS for wd in A.WDS for clip in A.CLIPS]


@pytest.mark.parametrize('betas,wd,clip', SETTINGS, ids=lambda x: str(x))
def test_the_bars_separate_the_two_ways_of_forming_the_coefficients(betas, wd, clip):
    bar = A.bars(A.BAR_N, betas, wd, clip)
    print(betas, wd, clip, 'bars', bar)
    assert 0 < bar['v'] < 1.29e-5 / 4, 'the v bar stays well below what float-formed coefficients cost'
    c = A.case(A.BAR_N, betas, wd, clip)
    ff = A.restate_distance(c, float_formed=True)
    print('float-formed', ff)
    if betas[1] == 0.999:
        assert ff['v'] > 4 * bar['v'], (ff, bar)
    for n in A.SMALL_N:
        d = A.restate_distance(A.case(n, betas, wd, clip))
        for k in A.NAMES:
            assert d[k] <= bar[k], (n, k, d[k], bar[k])


@pytest.mark.parametrize('clip', ['below', 'above'])
def test_the_clip_takes_both_branches(clip):
    for n in A.SMALL_N + (A.BAR_N,):
        c = A.case(n, A.BETAS[0], 0.0, clip)
        scales = [A.clip_scale(ss, c['max_norm']) for ss in c['ss']]
        assert all(s < 1 for s in scales) if clip == 'below' else all(s == 1 for s in scales), (n, scales)


def test_coefficients_are_torchs_rounded_once():
    for betas in A.BETAS:
        for step in A.STEPS:
            c1, c2, o1, o2 = A.coefficients(betas, step)
            assert (c1, o1, o2) == (np.float32(1 - betas[0] ** step), np.float32(1 - betas[0]), np.float32(1 - betas[1]))
            assert c2 == np.float32((1 - betas[1] ** step) ** 0.5)
    assert A.coefficients((0.9, 0.999), 1, float_formed=True)[3] != np.float32(0.001)


ALPHA_SETTINGS = [(r, w, b, wd) for r, w in A.ALPHA_SHAPES for b in A.ALPHA_BETAS for wd in A.ALPHA_WDS]


@pytest.mark.parametrize('rows,width,betas,wd', ALPHA_SETTINGS, ids=lambda x: str(x))
def test_the_alpha_bars_separate_the_two_ways_too(rows, width, betas, wd):
    bar = A.alpha_bars(rows, width, betas, wd)
    print(rows, width, betas, wd, 'bars', bar)
    assert 0 < bar['v'] < 1.29e-5 / 4
    c = A.alpha_case(max(rows, A.ALPHA_BAR_ROWS), width, betas, wd)
    assert A.alpha_restate_distance(c, float_formed=True)['v'] > 4 * bar['v']
    small = A.alpha_case(rows, width, betas, wd)
    assert (~small['live']).any() or width == 2, 'padding columns are part of the case'
    d = A.alpha_restate_distance(small)
    for k in A.ALPHA_NAMES:
        assert d[k] <= bar[k], (k, d[k], bar[k])
