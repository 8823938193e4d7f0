"""Cases of the cost-aware architecture update (ops.alpha_cost_step), shared by tests/test_arch_cost_host.py and
tests/test_arch_cost_gpu.py.

The generator mirrors tests/test_arch_two_gpu._case: ragged rows (n_r in 2..width, n_0 = width), alphas 0.5 N(0, 1) with -inf
padding, per step one random pair inside n_r and gate gradients uniform in (-1, 1).  Costs are uniform in [0.5, 4.0], each
row's last live candidate costs 0 (the `none` operator), padding 0.  cost_ref = 2.0, cost_weight 0.3 and 3.0, both forms, the
three optimizer settings of tests/test_arch_two_host.SETTINGS, four chained updates.

Conditioning (a condition on the inputs, not a tolerance): with beta1 = 0 a column moves by lr g / sqrt(v), and a column that
only ever sees the cost gradient k p (cost - E_r) inherits the cancellation in cost - E_r, so float32 arithmetic alone can
stand some 1e-5 from float64 on an unlucky draw (1e-4 was met).  The cases are therefore selected by the float32 torch
restatement ALONE -- never by a kernel: it must stay within CONDITION = 2.5e-6 (tests/util.rel_err) of the float64 restatement
on prob, m, v and prob_grad at every one of the four steps under all three settings, four times inside the 1e-5 the kernels
are held to.  SEEDS holds, per (mode, shape, form, weight), the first seed of 0..29 that meets half of that (room for another
host's float32 arithmetic), or the best of the thirty where none does.  tests/test_arch_cost_host.py asserts the condition for
every case the GPU test uses."""
import functools

import numpy as np
import torch

from tests.test_arch_two_host import SETTINGS, fin
from tests.util import rel_err

T = torch.from_numpy
EPS = 1e-8
STEPS = 4
COST_REF = 2.0
WEIGHTS = (0.3, 3.0)
FORMS = ('linear', 'log')
CONDITION = 2.5e-6
# 1 x 2; the supernet's own block; a last row alone in a second wave; the 'two' entry's limit; 'full' only: past the
# 256-thread stride with a ragged last pass
SHAPES = {'two': ((1, 2), (30, 5), (65, 4), (128, 5)), 'full': ((1, 2), (30, 5), (65, 4), (128, 5), (300, 3))}
NAMES = ('prob', 'm', 'v', 'prob_grad')

# (mode, rows, width, form, weight) -> seed; every other combination takes seed 0 (tools: `python -m tests.arch_cost_cases`
# prints the table from a survey of the seeds 0..29)
SEEDS = {
    ('full', 1, 2, 'linear', 0.3): 2,      # float32 vs float64: 5.8e-07
    ('full', 300, 3, 'log', 0.3): 4,       # 1.1e-06
    ('full', 300, 3, 'log', 3.0): 2,       # 1.2e-06
    ('two', 1, 2, 'linear', 0.3): 2,       # 7.1e-07
    ('two', 1, 2, 'log', 0.3): 2,          # 6.2e-07
    ('two', 30, 5, 'log', 0.3): 1,         # 6.8e-07
    ('two', 128, 5, 'linear', 3.0): 1,     # 4.2e-07
    ('two', 128, 5, 'log', 0.3): 12,       # 1.7e-06 (the best of 0..29)
    ('two', 128, 5, 'log', 3.0): 5,        # 1.2e-06
}


def combos(mode):
    return [(mode, rows, width, form, w) for rows, width in SHAPES[mode] for form in FORMS for w in WEIGHTS]


def generate(rows, width, seed):
    rs = np.random.RandomState(seed)
    n = rs.randint(2, width + 1, size=rows)
    n[0] = width                                            # the block's width is used
    live = np.arange(width)[None, :] < n[:, None]
    a = (0.5 * rs.standard_normal((rows, width))).astype(np.float32)
    a[~live] = -np.inf
    pairs = np.zeros((STEPS, rows, 2), np.int64)
    gg = np.zeros((STEPS, rows, width), np.float32)
    for t in range(STEPS):
        for r in range(rows):
            pairs[t, r] = rs.choice(n[r], size=2, replace=False)
            gg[t, r, :n[r]] = rs.uniform(-1.0, 1.0, n[r]).astype(np.float32)
    cost = rs.uniform(0.5, 4.0, (rows, width)).astype(np.float32)
    cost[~live] = 0.0
    cost[np.arange(rows), n - 1] = 0.0                      # the `none` operator
    return dict(n=n, live=live, a0=a, pairs=pairs, gg=gg, cost=cost)


@functools.lru_cache(maxsize=None)
def case(mode, rows, width, form, weight):
    c = generate(rows, width, SEEDS.get((mode, rows, width, form, weight), 0))
    c.update(mode=mode, rows=rows, width=width, form=form, weight=weight)
    return c


def replay(c, setting, dtype, dev='cpu', with_stats=True, with_prob_grad=True):
    """The case's four chained updates through ops.alpha_cost_step on `dev` in `dtype`; returns one dict per step with
    prob, m, v, prob_grad and stats as float64 numpy arrays (copies)."""
    from mmnas_amd import ops
    lr, betas, wd = SETTINGS[setting]
    rows, width = c['rows'], c['width']
    prob = T(c['a0'].copy()).to(dev, dtype)
    m, v = torch.zeros_like(prob), torch.zeros_like(prob)
    pg = torch.full_like(prob, 7.0) if with_prob_grad else None          # (written, not accumulated)
    stats = torch.full((rows + 2,), 7.0, dtype=dtype, device=dev) if with_stats else None
    cost = T(c['cost']).to(dev, dtype)
    out = []
    for t in range(STEPS):
        pl = [tuple(int(x) for x in p) for p in c['pairs'][t]] if c['mode'] == 'two' else None
        ops.alpha_cost_step(prob, T(c['gg'][t]).to(dev, dtype), m, v, pg, cost, lr, betas, EPS, t + 1, weight_decay=wd,
                            cost_weight=c['weight'], cost_ref=COST_REF, cost_form=c['form'], pairs=pl, stats=stats)
        out.append({k: (None if x is None else x.detach().cpu().double().numpy().copy())
                    for k, x in (('prob', prob), ('m', m), ('v', v), ('prob_grad', pg), ('stats', stats))})
    return out


@functools.lru_cache(maxsize=None)
def reference(mode, rows, width, form, weight, setting):
    """The float64 restatement of one case under one setting: computed once, shared, never written to."""
    out = replay(case(mode, rows, width, form, weight), setting, torch.float64)
    for step in out:
        for x in step.values():
            x.setflags(write=False)
    return out


def distance(got, ref, names=NAMES):
    """Worst tests/util.rel_err per quantity over the steps (padding -inf on both sides compares as 0)."""
    return {k: max(rel_err(fin(g[k]), fin(r[k])) for g, r in zip(got, ref)) for k in names}


def conditioning(c):
    """Worst float32-against-float64 distance of the torch restatement over the three settings."""
    worst = 0.0
    for s in range(len(SETTINGS)):
        d = distance(replay(c, s, torch.float32), replay(c, s, torch.float64))
        worst = max(worst, max(d.values()))
    return worst


if __name__ == '__main__':      # the survey SEEDS comes from
    for mode in ('full', 'two'):
        for key in combos(mode):
            met = []
            for seed in range(30):
                c = generate(key[1], key[2], seed)
                c.update(mode=mode, rows=key[1], width=key[2], form=key[3], weight=key[4])
                met.append((conditioning(c), seed))
                if met[-1][0] < CONDITION / 2:
                    break
            e, seed = met[-1] if met[-1][0] < CONDITION / 2 else min(met)
            if e >= CONDITION:
                raise SystemExit('no seed of 0..29 conditions %r' % (key,))
            if seed:
                print('    %r: %d,      # float32 vs float64: %.2g' % (key, seed, e))
