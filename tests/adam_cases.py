"""Cases, float64 references, float32 restatements and error bars of mmnas_adam_step and mmnas_alpha_full_step[_wd], shared by
tests/test_adam_kernels_host.py and tests/test_adam_kernels_gpu.py.  CPU only: nothing here touches the GPU or the native
library.

Reference: torch.optim.Adam on CPU double tensors, the clip by torch.nn.utils.clip_grad_norm_.  It takes the hyper-parameters
as the decimals a caller writes (0.999, 1e-3); the kernels take them as floats.  The moments start at zero and are carried
across the steps by the code under test; every step is judged on its own: the reference takes that step from the state the code
under test had before it (read as doubles), so an error of an earlier step is judged at that step and not again, against a
later, smaller yardstick.

Restatement: adam_one of util.hip statement by statement in numpy float32, with Adam's four coefficients (1 - beta1^t,
sqrt(1 - beta2^t), 1 - beta1, 1 - beta2) formed in double from the decimals and rounded once to float.  float_formed=True forms
them as the library did before (1.f - 0.999f, powf): the host test shows that the v bar rejects that.

Error measures, per element and step:
  v   (|v - V| - VFLOOR) / V                      VFLOOR = 2^-126: where V underflows float, v may be flushed to 0
  m   |m - M| / max(|M|, (1 - beta1) |g'|)        g' the clipped, decayed gradient: cancellation between beta1 m and the term
                                                  just added is not charged to the kernel
  p   (|p - P| - ulp32(P)) / |dP|                 dP the float64 update of that step
A measure is 0 where its numerator is <= 0, inf where only its denominator is 0.

Condition on the inputs: |g| >= 0.3 (except the two fixed elements below), so that with weight decay g' = s g + wd p never
cancels -- at step 1 v is (1 - beta2) g'^2 alone and would inherit that cancellation.

Bars: 4 x the worst value the restatement reaches against float64 on the same setting (betas, weight decay, clip, step
schedule, input distribution) -- room for another legitimate rounding order, FMA contraction and the ulps of sqrtf and
division.  The worst value over a handful of elements is no statistic (over one element it is often 0), so a setting is
measured on at least BAR_N elements; a case that is longer is measured on itself.  No bar comes from a kernel.  Measured on
the host that wrote this (BAR_N elements, all 18 settings): v 1.5e-7 ... 4.2e-7 (bar_v 6e-7 ... 1.7e-6), with float-formed
coefficients at beta2 = 0.999 1.30e-5 ... 1.32e-5; m 0 (beta1 = 0 without a clip: m = g exactly) ... 3.2e-7; p 1.3e-7 ... 3.3e-4
(the large values without weight decay, at elements whose m and with it dP passes through 0)."""
import functools
import math

import numpy as np
import torch

F32 = np.float32
VFLOOR = 2.0 ** -126
LR, EPS = 1e-3, 1e-9
BETAS = ((0.9, 0.98), (0.0, 0.999), (0.9, 0.999))
WDS = (0.0, 1e-2)
CLIPS = (None, 'below', 'above')      # max_norm below / above the gradient's norm: min(1, .) takes both branches
STEPS = (1, 2, 3, 4, 5, 1000)         # the last: carried moments, both bias corrections near 1
SMALL_N = (1, 3, 4, 5, 1023, 1024, 1027)
BAR_N = 20000
# (n, pointer offset in floats, betas, wd, clip, steps): a float4 body past the 4096 x 256-thread grid with a 3-element tail;
# the scalar kernel alone (every pointer off by one float) past its own 4096 x 256 threads
BIG = ((4194304 + 1203, 0, (0.9, 0.999), 1e-2, 'below', (1, 2)),
       (1048576 + 300, 1, (0.9, 0.999), 1e-2, 'below', (1, 2)))
NAMES = ('p', 'm', 'v')


def coefficients(betas, step, float_formed=False):
    """-> (c1, c2s, 1 - beta1, 1 - beta2) as float32."""
    b1, b2 = betas
    if float_formed:
        f1, f2, one, t = F32(b1), F32(b2), F32(1), F32(step)
        return one - np.power(f1, t), np.sqrt(one - np.power(f2, t)), one - f1, one - f2
    return F32(1 - b1 ** step), F32(math.sqrt(1 - b2 ** step)), F32(1 - b1), F32(1 - b2)


@functools.lru_cache(maxsize=64)
def case(n, betas, wd, clip, steps=STEPS):
    """Inputs of one chain of updates.  p0 ~ N(0, 1), without weight decay 1e-3 N(0, 1) so that the update and not p's ulp
    is what the p measure sees; g ~ 3 N(0, 1) pushed out to |g| >= 0.3, anew at every step; from 8 elements on, element 0
    always sees g = 0 and element 1 g = 1e-25 (without weight decay its V underflows float).  ss: the float32 sum-of-squares
    word of each step's gradient."""
    rs = np.random.RandomState((n * 31 + int(betas[0] * 10) * 7 + int(betas[1] * 1000) + (3 if wd else 0) + CLIPS.index(clip)) % (2 ** 31))
    p0 = ((1.0 if wd else 1e-3) * rs.standard_normal(n)).astype(F32)
    g = []
    for _ in steps:
        gt = (3.0 * rs.standard_normal(n)).astype(F32)
        gt = np.where(np.abs(gt) < 0.3, np.copysign(F32(0.3), gt), gt).astype(F32)
        if n >= 8:
            gt[0], gt[1] = 0.0, 1e-25
        g.append(gt)
    sumsq = [float((gt.astype(np.float64) ** 2).sum()) for gt in g]
    max_norm = None
    if clip is not None:
        norms = np.sqrt(np.array(sumsq))
        max_norm = float(F32(0.5 * norms.min() if clip == 'below' else 2.0 * norms.max()))
    for a in [p0] + g:
        a.setflags(write=False)
    return dict(n=n, betas=betas, wd=wd, clip=clip, steps=tuple(steps), p0=p0, g=g, ss=[F32(s) for s in sumsq], max_norm=max_norm)


def reference_step(c, t, state):
    """Step c['steps'][t] of torch.optim.Adam in float64 from `state` = (p, m, v) before it -> dict(p, m, v, mden, dp): the
    state after the step, the m measure's denominator max(|M|, (1 - beta1) |g'|) and the update."""
    p, m, v = (torch.from_numpy(np.asarray(a, np.float64).copy()) for a in state)
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=c['betas'], eps=EPS, weight_decay=c['wd'])
    opt.state[pt] = {'step': torch.tensor(float(c['steps'][t] - 1)), 'exp_avg': m, 'exp_avg_sq': v}
    pt.grad = torch.from_numpy(c['g'][t].astype(np.float64))
    if c['max_norm'] is not None:
        torch.nn.utils.clip_grad_norm_([pt], c['max_norm'])
    gp = pt.grad + c['wd'] * p
    opt.step()
    st = opt.state[pt]
    assert int(st['step']) == c['steps'][t]
    M, V = st['exp_avg'].numpy(), st['exp_avg_sq'].numpy()
    return dict(p=pt.detach().numpy(), m=M, v=V, mden=np.maximum(np.abs(M), (1 - c['betas'][0]) * gp.abs().numpy()),
                dp=(pt.detach() - p).numpy())


def clip_scale(ss, max_norm):
    """The kernels' min(1, max_norm / (sqrt(sumsq) + 1e-6)) in float32."""
    if max_norm is None:
        return F32(1)
    return min(F32(1), F32(max_norm) / (np.sqrt(F32(ss)) + F32(1e-6)))


def restate_step(c, t, state, float_formed=False):
    """adam_one of util.hip in numpy float32: (p, m, v) before step c['steps'][t] -> (p, m, v) after it."""
    p, m, v = state
    b1, b2 = F32(c['betas'][0]), F32(c['betas'][1])
    lr, eps, wd = F32(LR), F32(EPS), F32(c['wd'])
    c1, c2, omb1, omb2 = coefficients(c['betas'], c['steps'][t], float_formed)
    with np.errstate(under='ignore'):
        gi = c['g'][t] * clip_scale(c['ss'][t], c['max_norm'])
        if c['wd']:
            gi = gi + wd * p
        m = b1 * m + omb1 * gi
        v = b2 * v + omb2 * gi * gi
        p = p - (lr / c1) * m / (np.sqrt(v) / c2 + eps)
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v


def _ratio(num, den):
    """Worst num / den; 0 where num <= 0, inf where num > 0 = den."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(num > 0, num / den, 0.0)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def measures(got, ref):
    """Worst error measures of one step: got = (p, m, v) after it, ref = reference_step() from the same state before it."""
    p, m, v = (np.asarray(a, np.float64) for a in got)
    ulp = np.spacing(np.abs(ref['p']).astype(F32)).astype(np.float64)
    return dict(v=_ratio(np.abs(v - ref['v']) - VFLOOR, ref['v']),
                m=_ratio(np.abs(m - ref['m']), ref['mden']),
                p=_ratio(np.abs(p - ref['p']) - ulp, np.abs(ref['dp'])))


def restate_distance(c, float_formed=False):
    """Worst measures of the restatement over the chain, per quantity."""
    state = (c['p0'].copy(), np.zeros(c['n'], F32), np.zeros(c['n'], F32))
    out = dict.fromkeys(NAMES, 0.0)
    for t in range(len(c['steps'])):
        new = restate_step(c, t, state, float_formed)
        for k, e in measures(new, reference_step(c, t, state)).items():
            out[k] = max(out[k], e)
        state = new
    return out


@functools.lru_cache(maxsize=None)
def bars(n, betas, wd, clip, steps=STEPS):
    """4 x what the float32 restatement reaches on this setting, on max(n, BAR_N) elements."""
    return {k: 4.0 * e for k, e in restate_distance(case(max(n, BAR_N), betas, wd, clip, steps)).items()}


# ------------------------------------------------------------------------------------------------- the free-running chain
# The per-step judgement never sums a slow drift; one comparison at the end of the chain against the float64 chain that runs
# on its own closes that: v per element relative to V (floored as above), m and p relative to the largest |M| and |P| -- the
# yardsticks of a carried chain, where an element's own m or update may have shrunk since its error was made.
@functools.lru_cache(maxsize=8)
def reference_end(n, betas, wd, clip, steps=STEPS):
    c = case(n, betas, wd, clip, steps)
    state = (c['p0'].astype(np.float64), np.zeros(n), np.zeros(n))
    for t in range(len(steps)):
        r = reference_step(c, t, state)
        state = (r['p'], r['m'], r['v'])
    return state


def end_measures(got, ref):
    """v per element; m and p against the largest |M| and |P| -- from 1000 elements on only: the largest of a handful of
    elements is no yardstick that compares with the BAR_N elements the bar is measured on."""
    p, m, v = (np.asarray(a, np.float64) for a in got)
    P, M, V = ref
    out = dict(v=_ratio(np.abs(v - V) - VFLOOR, V))
    if P.size >= 1000:
        out.update(m=_ratio(np.abs(m - M), np.full_like(M, np.abs(M).max())), p=_ratio(np.abs(p - P), np.full_like(P, np.abs(P).max())))
    return out


@functools.lru_cache(maxsize=None)
def end_bars(n, betas, wd, clip, steps=STEPS):
    """4 x the restatement's distance from the free-running float64 chain at the end, on max(n, BAR_N) elements."""
    nb = max(n, BAR_N)
    c = case(nb, betas, wd, clip, steps)
    state = (c['p0'].copy(), np.zeros(nb, F32), np.zeros(nb, F32))
    for t in range(len(steps)):
        state = restate_step(c, t, state)
    return {k: 4.0 * e for k, e in end_measures(state, reference_end(nb, betas, wd, clip, steps)).items()}


# ------------------------------------------------------------------------------- mmnas_alpha_full_step[_wd] ('full' mode)
# The same judgement, step by step from the state before the step.  Reference: torch.optim.Adam in float64 over the live
# entries, their gradients the softmax-weighted gate gradients sum_j g_j p_j (delta_ij - p_i).  A fourth measure joins:
#   g   |pg - PG| / (p_i (|g_i| + sum_j |g_j| p_j))     prob_grad against the sum of the absolute values of its terms
# Condition on the inputs: alphas start uniform in (-0.4, 0.4) (five steps of lr = 0.1 keep every p_i well above 0.05) and a
# row's gate gradients are redrawn until every |g_i - sum_j g_j p_j| >= ALPHA_SEPARATION x max_j |g_j| on the free-running
# float64 chain, so that v = (1 - beta2) grad^2 does not inherit a cancellation in g_i - dot.  Measured on the host that wrote
# this (300 rows, all 12 settings): v 5.2e-7 ... 7.4e-7 (bar_v 2.1e-6 ... 3.0e-6), float-formed coefficients 1.33e-5 ... 1.37e-5;
# m 3.3e-7 ... 4.2e-7; g 2.0e-7 ... 2.3e-7.
ALPHA_SHAPES = ((1, 2), (65, 4), (300, 3))      # one row; a last row alone in a second wave; five waves, a ragged last one
ALPHA_BETAS = ((0.0, 0.999), (0.5, 0.999))
ALPHA_WDS = (0.0, 1e-3)
ALPHA_LR, ALPHA_EPS, ALPHA_STEPS = 0.1, 1e-8, 5
ALPHA_BAR_ROWS = 300
ALPHA_SEPARATION = 0.25
ALPHA_NAMES = ('p', 'm', 'v', 'g')


def _alpha_grad(a, g, live):
    """sum_j g_j p_j (delta_ij - p_i) per row in float64 -> (grad, p, dot); padding columns: 0."""
    z = np.where(live, a, -np.inf)
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    dot = (g * p).sum(1, keepdims=True)
    return p * (g - dot), p, dot


def _full(live, x, fill=0.0):
    out = np.full(live.shape, fill)
    out[live] = x
    return out


def alpha_reference_step(c, t, state, g=None):
    """Step t + 1 in float64 from `state` = (alpha, m, v) [rows, width] before it -> dict(p, m, v, g, gden, mden, dp)."""
    live, betas, wd = c['live'], c['betas'], c['wd']
    a, m, v = (np.asarray(x, np.float64) for x in state)
    g64 = np.asarray(c['gg'][t] if g is None else g, np.float64)
    grad, pr, _ = _alpha_grad(a, g64, live)
    gden = pr * (np.abs(g64) + (np.abs(g64) * pr).sum(1, keepdims=True))
    before = torch.from_numpy(a[live].copy())
    pt = before.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=ALPHA_LR, betas=betas, eps=ALPHA_EPS, weight_decay=wd)
    opt.state[pt] = {'step': torch.tensor(float(t)), 'exp_avg': torch.from_numpy(m[live].copy()),
                     'exp_avg_sq': torch.from_numpy(v[live].copy())}
    pt.grad = torch.from_numpy(grad[live].copy())
    gp = pt.grad + wd * before
    opt.step()
    st = opt.state[pt]
    M, V = _full(live, st['exp_avg'].numpy()), _full(live, st['exp_avg_sq'].numpy())
    return dict(p=_full(live, pt.detach().numpy(), -np.inf), m=M, v=V, g=grad, gden=gden, dp=_full(live, (pt.detach() - before).numpy()),
                mden=np.maximum(np.abs(M), (1 - betas[0]) * _full(live, gp.abs().numpy())))


@functools.lru_cache(maxsize=None)
def alpha_case(rows, width, betas, wd):
    """Inputs of ALPHA_STEPS chained 'full' updates: ragged rows (2..width live columns, row 0 all of them, the rest -inf),
    the conditioned gate gradients gg[t] (zero on padding)."""
    rs = np.random.RandomState(rows * 1000 + width * 10 + int(betas[0] * 10) + (5 if wd else 0))
    nlive = rs.randint(2, width + 1, size=rows)
    nlive[0] = width
    live = np.arange(width)[None, :] < nlive[:, None]
    a0 = rs.uniform(-0.4, 0.4, (rows, width)).astype(F32)
    a0[~live] = -np.inf
    c = dict(rows=rows, width=width, betas=betas, wd=wd, a0=a0, live=live, gg=[])
    state = (a0.astype(np.float64), np.zeros((rows, width)), np.zeros((rows, width)))
    for t in range(ALPHA_STEPS):
        g = np.zeros((rows, width), F32)
        for r in range(rows):
            for _ in range(20000):
                g[r, :nlive[r]] = rs.uniform(-1.0, 1.0, nlive[r]).astype(F32)
                _, _, dot = _alpha_grad(state[0][r:r + 1], g[r:r + 1].astype(np.float64), live[r:r + 1])
                if np.abs(g[r:r + 1] - dot)[live[r:r + 1]].min() >= ALPHA_SEPARATION * np.abs(g[r]).max():
                    break
            else:
                raise AssertionError('row %d: no separated gate gradients at alphas %r' % (r, state[0][r]))
        ref = alpha_reference_step(c, t, state, g)
        state = (ref['p'], ref['m'], ref['v'])
        g.setflags(write=False)
        c['gg'].append(g)
    a0.setflags(write=False)
    return c


def alpha_restate_step(c, t, state, float_formed=False):
    """alpha_full_row of alpha.hip in numpy float32: (alpha, m, v) before step t + 1 -> (alpha, m, v, prob_grad) after it."""
    live, width = c['live'], c['width']
    a, m, v = state
    b1, b2 = F32(c['betas'][0]), F32(c['betas'][1])
    lr, eps, wd = F32(ALPHA_LR), F32(ALPHA_EPS), F32(c['wd'])
    c1, c2, omb1, omb2 = coefficients(c['betas'], t + 1, float_formed)
    g = c['gg'][t]
    with np.errstate(under='ignore', invalid='ignore'):
        e = np.exp(a - a.max(1, keepdims=True))
        den, dot = np.zeros(a.shape[0], F32), np.zeros(a.shape[0], F32)
        for i in range(width):
            den = den + e[:, i]
        pr = e / den[:, None]
        for i in range(width):
            dot = dot + g[:, i] * pr[:, i]
        grad = pr * (g - dot[:, None])
        pg = grad.copy()
        if c['wd']:
            grad = grad + wd * np.where(live, a, F32(0))
        mi = b1 * m + omb1 * grad
        vi = b2 * v + omb2 * grad * grad
        an = np.where(live, a - (lr / c1) * mi / (np.sqrt(vi) / c2 + eps), a)
        m, v = np.where(live, mi, m), np.where(live, vi, v)
    assert an.dtype == F32 and m.dtype == F32 and v.dtype == F32 and pg.dtype == F32
    return an, m, v, pg


def alpha_measures(got, ref, live):
    """Worst error measures of one step over the live entries: got = (alpha, m, v, prob_grad) after it."""
    p, m, v, g = (np.asarray(x, np.float64)[live] for x in got)
    r = {k: x[live] for k, x in ref.items()}
    ulp = np.spacing(np.abs(r['p']).astype(F32)).astype(np.float64)
    return dict(v=_ratio(np.abs(v - r['v']) - VFLOOR, r['v']), m=_ratio(np.abs(m - r['m']), r['mden']),
                p=_ratio(np.abs(p - r['p']) - ulp, np.abs(r['dp'])), g=_ratio(np.abs(g - r['g']), r['gden']))


def alpha_restate_distance(c, float_formed=False):
    zero = np.zeros((c['rows'], c['width']), F32)
    state = (c['a0'].copy(), zero, zero)
    out = dict.fromkeys(ALPHA_NAMES, 0.0)
    for t in range(ALPHA_STEPS):
        new = alpha_restate_step(c, t, state, float_formed)
        for k, e in alpha_measures(new, alpha_reference_step(c, t, state), c['live']).items():
            out[k] = max(out[k], e)
        state = new[:3]
    return out


@functools.lru_cache(maxsize=None)
def alpha_bars(rows, width, betas, wd):
    """4 x what the float32 restatement reaches on this setting and width, on max(rows, ALPHA_BAR_ROWS) rows."""
    return {k: 4.0 * e for k, e in alpha_restate_distance(alpha_case(max(rows, ALPHA_BAR_ROWS), width, betas, wd)).items()}
