"""mmnas_adam_step on the GPU against torch.optim.Adam in float64, per element, after every step, for p, m and v
(tests/adam_cases.py: the cases, the reference, the error measures and the bars; tests/test_adam_kernels_host.py shows on the
CPU that the v bar rejects coefficients formed in float).

  * every betas setting x weight decay x clip (off, below and above the norm) at n = 1, 3, 4, 5, 1023, 1024, 1027: steps
    1..5 and one call with step = 1000 on the carried moments;
  * 4 194 304 + 1203 elements: the float4 body with a second grid-stride pass and a 3-element tail;
  * 1 048 576 + 300 elements with all four pointers one float off 16 bytes: the scalar kernel alone, with its own wrap.
p, m and v carry three guard elements behind them (and the offset case one in front): the kernels write their n elements only.
Every step is judged from the state before it; the end of each chain once more against the float64 chain that runs on its own.

mmnas_alpha_full_step[_wd] through ops.alpha_full_step: 1 x 2, 65 x 4, 300 x 3 with -inf padding columns, betas (0, 0.999) and
(0.5, 0.999), wd 0 and 1e-3, five steps: alphas, m, v and prob_grad per element, the padding, prob_grad against the weight decay.

When MMNAS_ADAM_KERNEL_STATS names a file, the worst measures met, and their largest share of a bar, are written there at the
end of the module (profiles/r15_adam_kernel_error_stats.json is one such run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import adam_cases as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 3
SENTINEL = 7777.0

ERR = {}     # label -> worst value met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_ADAM_KERNEL_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)
            f.write('\n')


def _buffer(a, off):
    """n host floats -> a device buffer of off + n + GUARD floats (SENTINEL around the n) and the view of the n."""
    buf = torch.full((off + a.size + GUARD,), SENTINEL, device=DEV)
    buf[off:off + a.size] = torch.from_numpy(np.array(a, np.float32)).to(DEV)
    return buf, buf[off:off + a.size]


def _chain(c, off, kind):
    """The case's chain of updates through mmnas_adam_step; every step measured against the float64 step from the state before
    it and held to the setting's bars, the end of the chain against the float64 chain that runs on its own."""
    import mmnas_amd._lib as L
    n = c['n']
    key = (n, c['betas'], c['wd'], c['clip'], c['steps'])
    bar = A.bars(*key)
    zero = np.zeros(n, np.float32)
    bufs = [_buffer(a, off) for a in (c['p0'], zero, zero)]
    p, m, v = (view for _, view in bufs)
    assert all(x.data_ptr() % 16 == 4 * off for x in (p, m, v))
    state = (c['p0'].copy(), zero, zero)
    failures = []

    def judge(label, got, bars):
        for k, e in got.items():
            _note('adam_step|%s|%s' % (label, k), e)
            _note('adam_step|%s|%s|share_of_bar' % (label, k), e / bars[k] if e else 0.0)
            print('n=%d offset=%d %s: %s %.3g (bar %.3g)' % (n, off, label, k, e, bars[k]))
            if not e <= bars[k]:
                failures.append((label, k, e, bars[k]))

    for t, step in enumerate(c['steps']):
        _, g = _buffer(c['g'][t], off)
        assert g.data_ptr() % 16 == 4 * off
        ss = torch.from_numpy(np.array([c['ss'][t]], np.float32)).to(DEV) if c['max_norm'] is not None else None
        L.check(L.lib().mmnas_adam_step(L.fptr(p), L.fptr(g), L.fptr(m), L.fptr(v), n, A.LR, c['betas'][0], c['betas'][1], A.EPS,
                                        c['wd'], L.fptr(ss), c['max_norm'] or 0.0, step, L.stream()))
        new = tuple(x.cpu().numpy() for x in (p, m, v))
        for (buf, _), name in zip(bufs, A.NAMES):
            edge = torch.cat([buf[:off], buf[off + n:]]).cpu().numpy()
            assert np.all(edge == SENTINEL), (step, name, 'written outside its n elements')
        assert all(np.all(np.isfinite(x)) for x in new), step
        judge('%s|step %s' % (kind, step if step == 1000 else '1..5'), A.measures(new, A.reference_step(c, t, state)), bar)
        state = new
    judge('%s|end of chain' % kind, A.end_measures(state, A.reference_end(*key)), A.end_bars(*key))
    assert not failures, failures


@pytest.mark.parametrize('clip', A.CLIPS, ids=lambda x: 'clip_%s' % x)
@pytest.mark.parametrize('wd', A.WDS)
@pytest.mark.parametrize('betas', A.BETAS, ids=lambda x: str(x))
@pytest.mark.parametrize('n', A.SMALL_N)
def test_adam_step_per_element_against_float64(n, betas, wd, clip):
    _chain(A.case(n, betas, wd, clip), 0, 'small')


@pytest.mark.parametrize('n,off,betas,wd,clip,steps', A.BIG, ids=lambda x: str(x))
def test_adam_step_past_the_grid_stride_wrap(n, off, betas, wd, clip, steps):
    _chain(A.case(n, betas, wd, clip, steps), off, 'misaligned wrap' if off else 'float4 wrap')


@pytest.mark.parametrize('wd', A.ALPHA_WDS)
@pytest.mark.parametrize('betas', A.ALPHA_BETAS, ids=lambda x: str(x))
@pytest.mark.parametrize('rows,width', A.ALPHA_SHAPES)
def test_alpha_full_step_per_element_against_float64(rows, width, betas, wd):
    """mmnas_alpha_full_step (wd = 0) / mmnas_alpha_full_step_wd through ops.alpha_full_step: alphas, m, v and prob_grad after
    each of five steps; padding columns stay -inf, their moments and prob_grad 0; prob_grad is the same bits whatever the
    weight decay."""
    from mmnas_amd import ops
    c = A.alpha_case(rows, width, betas, wd)
    bar = A.alpha_bars(rows, width, betas, wd)
    live, pad = c['live'], ~c['live']
    prob = torch.from_numpy(c['a0'].copy()).to(DEV)
    m, v = torch.zeros_like(prob), torch.zeros_like(prob)
    state = (c['a0'].copy(), np.zeros((rows, width), np.float32), np.zeros((rows, width), np.float32))
    failures = []
    for t in range(A.ALPHA_STEPS):
        g = torch.from_numpy(c['gg'][t].copy()).to(DEV)
        twin = [x.clone() for x in (prob, m, v)]
        pg, pg_twin = torch.full_like(prob, SENTINEL), torch.full_like(prob, SENTINEL)
        ops.alpha_full_step(prob, g, m, v, pg, A.ALPHA_LR, betas, A.ALPHA_EPS, t + 1, weight_decay=wd)
        ops.alpha_full_step(*twin[:1], g, *twin[1:], pg_twin, A.ALPHA_LR, betas, A.ALPHA_EPS, t + 1, weight_decay=0.0 if wd else 1e-3)
        assert torch.equal(pg, pg_twin), 'prob_grad depends on the weight decay'
        new = tuple(x.cpu().numpy() for x in (prob, m, v, pg))
        assert np.all(np.isneginf(new[0][pad])) and np.all(np.isfinite(new[0][live])), 'padding columns stay -inf'
        assert not new[1][pad].any() and not new[2][pad].any() and not new[3][pad].any(), 'padding moments and prob_grad stay 0'
        for k, e in A.alpha_measures(new, A.alpha_reference_step(c, t, state), live).items():
            _note('alpha_full_step|%s' % k, e)
            _note('alpha_full_step|%s|share_of_bar' % k, e / bar[k] if e else 0.0)
            print('%dx%d step %d %s: %.3g (bar %.3g)' % (rows, width, t + 1, k, e, bar[k]))
            if not e <= bar[k]:
                failures.append((t + 1, k, e, bar[k]))
        state = new[:3]
    assert not failures, failures
