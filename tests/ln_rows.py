"""Degenerate LayerNorm rows for the hand-written copies of the reference's LayerNorm (modules.py:44-56: Bessel-corrected
std, eps = 1e-6 added to the std): row classes, the float64 yardstick and the judge.

The row arithmetic is written out in rowops.hip (ln_fwd / ln_bwd), mixed.hip (node_mix), gemmln.hip (row-panel epilogue),
small.hip (short self-attention forward + backward, short feed-forward), vgdhead.hip (grounding head, both directions) and
retrieval.hip (pair head).  On randn-like rows (sd ~ 1) a misplaced eps, a one-pass variance and the sd == 0 case are all
invisible at the project's bars; each class below makes one of them visible.

Yardstick: the module's own statement `a * (x - mean) / (x.std(-1) + eps) + b` through torch autograd in float64 (torch
masks std's backward to 0 where std == 0, so a constant row has the finite gradient (g - mean(g)) / eps) -- not the closed
form of oracle.layer_norm_backward, which the kernels were written from.

Judge: max|got - ref| / max|ref| per output and PER CLASS (a 1e15 row cannot hide a 1e-12 row).  Bars: test_layernorm's
1e-5 forward / 1e-4 backward, except `offset`, where the float32 module itself is up to 1e-5 away from float64 (the mean of
d values near 64 rounds): there the bar is max(project bar, 4 x the float32 module's own error on the same case); 4 leaves
room for another summation order across 64 lanes and sits far below a one-pass variance (>= 3e-4 at mean 64).

MMNAS_LN_ROWS_STATS=<file>: the GPU module writes the worst error per (kernel, class, output) there, each beside its bar
and, for `offset`, beside the float32-module figure the bar came from."""
import json
import os

import numpy as np
import torch

EPS = 1e-6
FWD_BAR, BWD_BAR = 1e-5, 1e-4
CLASSES = ('randn', 'const', 'sd_eps', 'sd_tiny', 'offset', 'big', 'small', 'outlier')
CONSTS = (0.0, 2.5, -3.0, 0.5, 1024.0, -0.125)
FWD_OUTPUTS = ('y', 'out', 'z', 'scores', 'reg', 'logits')   # every other output is a gradient
T = torch.from_numpy


def _seed(cls, R, d, seed):
    return (seed * 1000003 + CLASSES.index(cls) * 7919 + R * 31 + d) % (2 ** 31 - 1)


def rows(cls, R, d, seed=0):
    """[R, d] float32 rows of one class (deterministic in (cls, R, d, seed))."""
    rs = np.random.RandomState(_seed(cls, R, d, seed))
    n = rs.standard_normal((R, d))
    if cls == 'randn':
        x = 2 * n + 0.3
    elif cls == 'const':
        x = np.repeat(np.asarray([CONSTS[(i + seed) % len(CONSTS)] for i in range(R)])[:, None], d, axis=1)
    elif cls == 'sd_eps':
        x = n * 2.0 ** -20
    elif cls == 'sd_tiny':
        x = n * 2.0 ** -27
    elif cls == 'offset':
        x = 64 + n
    elif cls == 'big':
        x = n * 1e15
    elif cls == 'small':
        x = n * 1e-12
    elif cls == 'outlier':
        x = n
        x[np.arange(R), rs.randint(0, d, size=R)] = 1e4
    else:
        raise KeyError(cls)
    return np.ascontiguousarray(x, dtype=np.float32)


def interleaved(R, d, seed=0):
    """[R, d] rows with the classes interleaved (row i is of class CLASSES[i % 8]) and the class index of every row."""
    per = -(-R // len(CLASSES))
    x = np.empty((R, d), np.float32)
    which = np.arange(R) % len(CLASSES)
    for k, cls in enumerate(CLASSES):
        x[which == k] = rows(cls, per, d, seed)[:int((which == k).sum())]
    return x, which


def params(d, seed=0):
    rs = np.random.RandomState(7001 + 13 * d + seed)
    return (1 + 0.2 * rs.standard_normal(d)).astype(np.float32), (0.1 * rs.standard_normal(d)).astype(np.float32)


def grad_out(R, d, seed=0):
    return np.random.RandomState(9001 + 17 * d + R + seed).standard_normal((R, d)).astype(np.float32)


def module_ln(x, a, b, eps=EPS):
    """The reference module, as written (modules.py:52-56)."""
    return a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + b


def ln_reference(x, a, b, gy, mask=None, dtype=torch.float64):
    """y, dx, da, db of the module through autograd in `dtype`; with a dropout multiplier `mask` also ddrop = dx * mask and its
    column sums dcol.  float64 numpy arrays."""
    X, A, B = (T(np.asarray(v)).to(dtype).requires_grad_(True) for v in (x, a, b))
    y = module_ln(X, A, B)
    y.backward(T(np.asarray(gy)).to(dtype))
    res = {'y': y.detach(), 'dx': X.grad, 'da': A.grad, 'db': B.grad}
    if mask is not None:
        res['ddrop'] = X.grad * T(np.asarray(mask)).to(dtype)
        res['dcol'] = res['ddrop'].sum(0)
    return {k: v.double().numpy() for k, v in res.items()}


def err(got, ref, floor=0.0):
    """max|got - ref| / max(max|ref|, floor) (absolute where that is 0).  floor: the sum of the absolute values of the terms
    of an output that is a cancelling sum -- its own size says nothing about the rounding it may carry."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    den = max(float(np.abs(ref).max()), float(floor))
    num = float(np.abs(got - ref).max())
    return num / den if den > 0 else num


def project_bar(name):
    return FWD_BAR if name in FWD_OUTPUTS else BWD_BAR


def bars(cls, ref64, ref32=None, floors=None):
    """output -> (bar, float32-module error or None).  `offset` needs ref32: the same reference run in float32."""
    out = {}
    for name in ref64:
        if cls == 'offset':
            assert ref32 is not None, 'the offset bar is measured against the float32 module on the same case'
            e32 = err(ref32[name], ref64[name], (floors or {}).get(name, 0.0))
            out[name] = (max(project_bar(name), 4 * e32), e32)
        else:
            out[name] = (project_bar(name), None)
    return out


STATS = {}   # 'kernel|class|output' -> {'err', 'bar', 'ref32_err'?}: the worst case seen in this process


def _record(kernel, cls, name, e, bar, e32):
    key = '%s|%s|%s' % (kernel, cls, name)
    cur = STATS.get(key)
    # the worst case is the one that uses most of its bar
    if cur is None or e / bar > cur['err'] / cur['bar']:
        STATS[key] = {'err': e, 'bar': bar}
        if e32 is not None:
            STATS[key]['ref32_err'] = e32


def first_bad_row(a):
    bad = np.argwhere(~np.isfinite(np.asarray(a)))
    return None if bad.size == 0 else int(bad[0][0])


def judge(kernel, cls, got, ref64, ref32=None, where='', floors=None):
    """Every output of `ref64` (name -> array; the rows are of class `cls` only): finite, then within its bar.  The message
    names the kernel, the class, the output and the first offending row.  floors: output -> err()'s floor."""
    problems = []
    for name, (bar, e32) in bars(cls, ref64, ref32, floors).items():
        g = np.asarray(got[name], np.float64)
        r = first_bad_row(g)
        if r is not None:
            problems.append('%s%s: %s is not finite on class %s: %d of %d elements, first in row %d'
                            % (kernel, where, name, cls, int((~np.isfinite(g)).sum()), g.size, r))
            continue
        e = err(g, ref64[name], (floors or {}).get(name, 0.0))
        _record(kernel, cls, name, e, bar, e32)
        if not e <= bar:
            d = np.abs(g - np.asarray(ref64[name], np.float64))
            problems.append('%s%s: %s on class %s: error %.3e above the bar %.3e (worst in row %d)'
                            % (kernel, where, name, cls, e, bar, int(np.unravel_index(int(d.argmax()), d.shape)[0])))
    assert not problems, '\n'.join(problems)


def write_stats():
    path = os.environ.get('MMNAS_LN_ROWS_STATS')
    if not path or not STATS:
        return
    doc = {'bars': {'forward': FWD_BAR, 'backward': BWD_BAR,
                    'offset': 'max(project bar, 4 * ref32_err): ref32_err = the float32 module against float64 on the same case'},
           'metric': 'max|got - float64 module| / max|float64 module|, per output and per row class',
           'worst': {k: STATS[k] for k in sorted(STATS)}}
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
