"""Generate tests/golden/arch_two.npz: the reference's own architecture update of ALPHA_BINARY_MODE 'two' -- per node
MixedOp.set_arch_param_grad over the sampled pair, torch.optim.Adam over the alpha_prob parameters, then
MixedOp.rescale_updated_arch_param (search_vqa.py:330-335, mixed.py:179-208) -- on a column of reference MixedOps of
widths 2, 4 and 5 for STEPS consecutive updates, under three optimizer settings.  Needs the reference tree, like
make_golden.py (whose import helper it uses):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_arch_two.py

Fixed and recorded: the initial alphas, every step's (active, inactive) pair per node and every step's gate gradients.
With beta1 = 0 Adam turns any non-zero gradient into a full +-lr move, so a pair gradient near zero would make the
reference's own float32 sign a coin toss: the gate gradients are drawn such that |g_i - g_j| >= MIN_GAP on every sampled
pair (asserted), and the reference is run a second time in float64 -- the two runs must agree to 1e-6, which excludes
inputs on which the reference itself is ill-conditioned by construction instead of by a tolerance.

Keys ([T] steps, [N] nodes, width W = 5, alphas padded with -inf, everything else with 0):
    widths [N], alpha0 [N, W], pairs [T, N, 2], gate_grad [T, N, W], eps,
    s<k>|hyper = (lr, beta1, beta2, weight_decay), s<k>|prob_grad / alpha / exp_avg / exp_avg_sq [T, N, W] after each step.
Recorded results only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import cases
from tests.golden import make_golden as G

KINDS = ('enc_safe', 'dec_safe', 'dec', 'enc_safe', 'dec_safe', 'dec')     # 2, 4, 5 candidates, twice
SETTINGS = ((0.1, (0.0, 0.999), 0.0),       # the scripts' alpha_optim (search_vqa.py:194)
            (0.1, (0.5, 0.999), 1e-3),
            (1.0, (0.0, 0.999), 0.0))
STEPS = 6
WIDTH = 5
MIN_GAP = 0.1
EPS = 1e-8


def draw_inputs(widths, rs):
    alpha0 = [(0.5 * rs.standard_normal(n)).astype(np.float32) for n in widths]
    pairs = np.zeros((STEPS, len(widths), 2), np.int64)
    gg = np.zeros((STEPS, len(widths), WIDTH), np.float32)
    for t in range(STEPS):
        for k, n in enumerate(widths):
            i, j = (int(x) for x in rs.choice(n, size=2, replace=False))
            while True:
                g = rs.uniform(-1.0, 1.0, n).astype(np.float32)
                if abs(float(g[i]) - float(g[j])) >= MIN_GAP:
                    break
            pairs[t, k] = (i, j)
            gg[t, k, :n] = g
    return alpha0, pairs, gg


def run_reference(cfg, widths, alpha0, pairs, gg, lr, betas, wd, dtype):
    MixedOp = G.RMIX.MixedOp
    mops = [MixedOp(cfg, kind).to(dtype) for kind in KINDS]
    for m, n, a in zip(mops, widths, alpha0):
        assert m.n_choices == n
        m.alpha_prob.data.copy_(torch.from_numpy(a).to(dtype))
    optim = torch.optim.Adam([m.alpha_prob for m in mops], lr, betas=betas, eps=EPS, weight_decay=wd)
    rec = {k: np.zeros((STEPS, len(mops), WIDTH), np.float64) for k in ('prob_grad', 'alpha', 'exp_avg', 'exp_avg_sq')}
    rec['alpha'][:] = -np.inf
    MixedOp.MODE = 'two'
    try:
        for t in range(STEPS):
            for k, m in enumerate(mops):
                m.active_index, m.inactive_index = [int(pairs[t, k, 0])], [int(pairs[t, k, 1])]
                m.alpha_gate.grad = torch.from_numpy(gg[t, k, :m.n_choices].copy()).to(dtype)
                m.alpha_prob.grad = None                   # (the script's net.zero_grad(), search_vqa.py:328)
                m.set_arch_param_grad()
                rec['prob_grad'][t, k, :m.n_choices] = m.alpha_prob.grad.numpy()
            optim.step()
            for k, m in enumerate(mops):
                m.rescale_updated_arch_param()
                n = m.n_choices
                rec['alpha'][t, k, :n] = m.alpha_prob.detach().numpy()
                rec['exp_avg'][t, k, :n] = optim.state[m.alpha_prob]['exp_avg'].numpy()
                rec['exp_avg_sq'][t, k, :n] = optim.state[m.alpha_prob]['exp_avg_sq'].numpy()
    finally:
        MixedOp.MODE = None
    return rec


def rel(a, b):
    a, b = (np.where(np.isfinite(x), x, 0.0) for x in (a, b))
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def gen_arch_two(fname='arch_two.npz'):
    cfg = cases.small_cfg(HSIZE=128)
    widths = [len(G.ROA.OpsAdapter().Used_OPS[k]) for k in KINDS]
    assert sorted(set(widths)) == [2, 4, 5], widths
    alpha0, pairs, gg = draw_inputs(widths, np.random.RandomState(9900))
    for t in range(STEPS):
        for k in range(len(widths)):
            i, j = pairs[t, k]
            assert i != j and abs(float(gg[t, k, i]) - float(gg[t, k, j])) >= MIN_GAP, (t, k)
    a0 = np.full((len(widths), WIDTH), -np.inf, np.float32)
    for k, a in enumerate(alpha0):
        a0[k, :a.size] = a
    out = {'widths': np.array(widths, np.int64), 'alpha0': a0, 'pairs': pairs, 'gate_grad': gg, 'eps': np.float64(EPS)}
    for s, (lr, betas, wd) in enumerate(SETTINGS):
        r32 = run_reference(cfg, widths, alpha0, pairs, gg, lr, betas, wd, torch.float32)
        r64 = run_reference(cfg, widths, alpha0, pairs, gg, lr, betas, wd, torch.float64)
        worst = {k: rel(r32[k], r64[k]) for k in r32}
        print('setting', s, (lr, betas, wd), 'float32 run against float64 run:', worst)
        assert max(worst.values()) < 1e-6, worst      # the reference is well-conditioned on these inputs
        out['s%d|hyper' % s] = np.array([lr, betas[0], betas[1], wd], np.float64)
        for k, v in r32.items():
            out['s%d|%s' % (s, k)] = v.astype(np.float32)
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, len(out), 'arrays,', os.path.getsize(os.path.join(HERE, fname)), 'bytes')


if __name__ == '__main__':
    gen_arch_two()
