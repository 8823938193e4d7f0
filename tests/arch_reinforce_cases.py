"""Cases of the REINFORCE architecture update (ops.alpha_reinforce_step), shared by tests/test_arch_reinforce_host.py and
tests/test_arch_reinforce_gpu.py.  Modelled on tests/arch_cost_cases.py, whose CONDITION, cost recipe and optimizer settings
these reuse.

The generator: ragged rows (n_r in 2..width, n_0 = width; at width 2 every row is full), alphas 0.5 N(0, 1) with -inf padding,
per step M sampled architectures (one live candidate per row, uniform) and M qualities uniform in (0.3, 0.7).  Costs are
uniform in [0.5, 4.0], each row's last live candidate costs 0 (the `none` operator), padding 0.  cost_ref is rows * 1.5 (near
the expected price of a uniform sample), baseline_decay 0.9, four chained updates under the three settings of
tests/test_arch_two_host.SETTINGS.  Rewards: no cost; 'mul' with w = -0.07; 'add' with w = -0.3.

Conditioning (a condition on the inputs, not a tolerance): with beta1 = 0 a column moves by lr g / sqrt(v), so a column whose
gradient is a near-cancellation of sum_{i: a_ir = j} A_i against p sum_i A_i carries the rounding of the float32 rewards and
probabilities straight into the alpha.
The cases are therefore selected by the float32 torch restatement ALONE -- never by a kernel: it must stay within CONDITION =
2.5e-6 (tests/util.rel_err) of the float64 restatement on prob, m, v, prob_grad and stats at every one of the four steps under
all three settings.  SEEDS holds, per (rows, width, M, reward), the first seed of 0..29 that meets half of that (room for
another host's float32 arithmetic), or the best of the thirty where none does; a combination no seed conditions is dropped and
named in DROPPED.  tests/test_arch_reinforce_host.py asserts the condition for every case the GPU test uses."""
import functools

import numpy as np
import torch

from tests.arch_cost_cases import CONDITION
from tests.test_arch_two_host import SETTINGS, fin
from tests.util import rel_err

T = torch.from_numpy
EPS = 1e-8
STEPS = 4
DECAY = 0.9
# 1 x 2; the supernet's own block; a last row alone in a second wave; 128 rows; past the 256-thread stride, ragged last pass
SHAPES = ((1, 2), (30, 5), (65, 4), (128, 5), (300, 3))
REWARDS = {'none': (None, 0.0), 'mul': ('mul', -0.07), 'add': ('add', -0.3)}
NAMES = ('prob', 'm', 'v', 'prob_grad', 'stats')

# (rows, width, M, reward) -> seed; every other combination takes seed 0 (`python -m tests.arch_reinforce_cases` prints the
# table from a survey of the seeds 0..29)
SEEDS = {
    (1, 2, 1, 'none'): 1,        # float32 vs float64: 9.4e-07
    (1, 2, 1, 'mul'): 1,         # 9.4e-07
    (1, 2, 1, 'add'): 1,         # 9.4e-07
    (1, 2, 4, 'none'): 2,        # 8.8e-07
    (1, 2, 4, 'mul'): 3,         # 5.3e-07
    (30, 5, 1, 'none'): 1,       # 1.1e-06
    (30, 5, 1, 'mul'): 1,        # 8.6e-07
    (30, 5, 16, 'mul'): 2,       # 1.2e-06
    (65, 4, 1, 'mul'): 1,        # 2.5e-07
    (128, 5, 4, 'add'): 1,       # 6.7e-07
    (128, 5, 16, 'mul'): 3,      # 4.6e-07
    (128, 5, 16, 'add'): 8,      # 1.1e-06
}
DROPPED = ()                     # (the survey conditioned every combination)


def samples(rows, width):
    return (1, 4, 16) if (rows, width) in ((30, 5), (128, 5)) else (1, 4)


def combos():
    return [k for k in ((rows, width, M, rw) for rows, width in SHAPES for M in samples(rows, width) for rw in REWARDS)
            if k not in DROPPED]


def generate(rows, width, M, seed):
    rs = np.random.RandomState(seed)
    n = rs.randint(2, width + 1, size=rows)
    n[0] = width                                            # the block's width is used
    live = np.arange(width)[None, :] < n[:, None]
    a = (0.5 * rs.standard_normal((rows, width))).astype(np.float32)
    a[~live] = -np.inf
    choice = np.stack([rs.randint(0, n, size=(M, rows)) for _ in range(STEPS)]).astype(np.int64)      # [STEPS, M, rows]
    quality = rs.uniform(0.3, 0.7, (STEPS, M)).astype(np.float32)
    cost = rs.uniform(0.5, 4.0, (rows, width)).astype(np.float32)
    cost[~live] = 0.0
    cost[np.arange(rows), n - 1] = 0.0                      # the `none` operator
    return dict(n=n, live=live, a0=a, choice=choice, quality=quality, cost=cost, cost_ref=1.5 * rows)


@functools.lru_cache(maxsize=None)
def case(rows, width, M, reward):
    c = generate(rows, width, M, SEEDS.get((rows, width, M, reward), 0))
    c.update(rows=rows, width=width, M=M, reward=reward)
    return c


def replay(c, setting, dtype, dev='cpu', with_stats=True, with_prob_grad=True, with_cost=True, baseline0=None):
    """The case's four chained updates through ops.alpha_reinforce_step on `dev` in `dtype`; returns one dict per step with
    prob, m, v, prob_grad, stats, baseline as float64 numpy arrays (copies) and err as an int.  baseline0: start from an
    initialised baseline of that value instead of a fresh one."""
    from mmnas_amd import ops
    lr, betas, wd = SETTINGS[setting]
    M = c['M']
    form, w = REWARDS[c['reward']]
    prob = T(c['a0'].copy()).to(dev, dtype)
    m, v = torch.zeros_like(prob), torch.zeros_like(prob)
    pg = torch.full_like(prob, 7.0) if with_prob_grad else None          # (written, not accumulated)
    stats = torch.full((M + 3,), 7.0, dtype=dtype, device=dev) if with_stats else None
    cost = T(c['cost']).to(dev, dtype) if form is not None and with_cost else None
    baseline = torch.tensor([0.0, 0.0] if baseline0 is None else [baseline0, 1.0], dtype=dtype, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = []
    for t in range(STEPS):
        ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][t], T(c['quality'][t]).to(dev, dtype), baseline, lr, betas, EPS, t + 1,
                                 weight_decay=wd, cost=cost, cost_weight=w, cost_ref=c['cost_ref'], reward_form=form or 'mul',
                                 baseline_decay=DECAY, stats=stats, err=err, n_choices=c['n'])
        step = {k: (None if x is None else x.detach().cpu().double().numpy().copy())
                for k, x in (('prob', prob), ('m', m), ('v', v), ('prob_grad', pg), ('stats', stats), ('baseline', baseline))}
        step['err'] = int(err.cpu()[0])
        out.append(step)
    return out


@functools.lru_cache(maxsize=None)
def reference(rows, width, M, reward, setting):
    """The float64 restatement of one case under one setting: computed once, shared, never written to."""
    out = replay(case(rows, width, M, reward), setting, torch.float64)
    for step in out:
        for x in step.values():
            if isinstance(x, np.ndarray):
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
    for key in combos():
        met = []
        for seed in range(30):
            c = generate(key[0], key[1], key[2], seed)
            c.update(rows=key[0], width=key[1], M=key[2], reward=key[3])
            met.append((conditioning(c), seed))
            if met[-1][0] < CONDITION / 2:
                break
        e, seed = met[-1] if met[-1][0] < CONDITION / 2 else min(met)
        if e >= CONDITION:
            print('    DROP %r: best %.2g at seed %d' % (key, e, seed))
        elif seed:
            print('    %r: %d,      # float32 vs float64: %.2g' % (key, seed, e))
