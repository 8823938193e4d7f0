"""Generate tests/golden/itm_search_traj.npz: the reference's own ITM search statements (search_itm.py:381-447) on the
reference hygr_itm.Net_Search -- three forwards (positive, negative caption, negative image), BCE_Loss, the three `0 * sum`
lines, zero_grad, backward, clip_grad_norm_, warm-up Adam; every ALPHA_EVERY-th step the architecture step: three forwards
under ALPHA_BINARY_MODE, set_arch_param_grad, Adam on the alphas and, in mode 'two', rescale_updated_arch_param -- for
ROUNDS bilevel rounds in each of the modes 'full' and 'two'.  The case (dimensions, batches, injected samples, optimizer
settings) is tests/golden/cases_itm_search.py's.  Needs the reference tree, like make_golden.py (whose import helper it uses):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_itm_search.py

With beta1 = 0 the alphas' Adam turns any gradient into a full +-lr move, and the weights' Adam does the same on a first step:
a gradient near zero would make the reference's own float32 sign a coin toss.  So the reference is run a second time in
float64 and the two runs must agree (losses to 1e-5, alphas to 1e-4, the recorded weights to 1e-2 of their largest motion), which
excludes a case on which the reference itself is ill-conditioned by construction instead of by a tolerance.

Keys, per mode m in ('full', 'two'): m|losses [ROUNDS * 3] float64 (weight, weight, arch per round), m|alphas
[ROUNDS, 30, 4] after every arch step (padded with 0), m|plan<r>_<s> [30, 2] the injected (active, inactive-or--1) sample of
round r step s, m|P:<key> the three weight tensors of cases_itm_search.weight_keys after the last round; and weight_keys, the
checksum of the generated inputs.  Recorded results only."""
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import cases
from tests.golden import cases_itm_search as CS
from tests.golden import make_golden as G

T = torch.from_numpy


def run_reference(mode, dtype):
    from mmnas.utils.itm_loss import BCE_Loss
    from mmnas.utils.optimizer import WarmupOptimizer
    MixedOp = G.RMIX.MixedOp
    c, batches, plans = CS.setup()
    H = CS.HYPER
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = G.hygr_itm.Net_Search(c['cfg'], init)
    net.train()
    G.load_state(net, c['P'])
    net.to(dtype)
    net_optim = WarmupOptimizer(H['net_lr'], torch.optim.Adam(net.net_parameters(), lr=0, betas=H['net_betas'], eps=H['net_eps'],
                                                              weight_decay=0), H['epoch_steps'], warmup=True)
    alpha_optim = torch.optim.Adam(net.alpha_prob_parameters(), H['alpha_lr'], betas=H['alpha_betas'], weight_decay=0)
    loss_fn = BCE_Loss(SimpleNamespace(REDUCTION='sum'))
    mops = net.redundant_modules

    def triplet(pair):
        pos, neg = (tuple(T(a).to(dtype) if a.dtype == np.float32 else T(a) for a in t) for t in pair)
        return pos, (pos[0], pos[1], pos[2], neg[3], neg[4]), (neg[0], neg[1], neg[2], pos[3], pos[4])

    losses, alphas = [], []
    try:
        for r in range(CS.ROUNDS):
            for s in range(CS.ALPHA_EVERY):          # network step (search_itm.py:381-406)
                inp_pos, inp_negc, inp_negi = triplet(batches['train'][s])
                G._inject(mops, CS.flat(plans[mode][r][s]), MixedOp, None)
                net.unused_modules_off()
                loss = loss_fn(net(inp_pos), net(inp_negc), net(inp_negi))
                loss += 0 * sum(p.sum() for p in net.alpha_prob_parameters())
                loss += 0 * sum(p.sum() for p in net.alpha_gate_parameters())
                loss += 0 * sum(p.sum() for p in net.net_parameters())
                net.zero_grad()
                loss.backward()
                losses.append(loss.item())
                torch.nn.utils.clip_grad_norm_(net.net_parameters(), H['clip'])
                net_optim.step()
                net.unused_modules_back()
            inp_pos, inp_negc, inp_negi = triplet(batches['eval'])      # architecture step (search_itm.py:408-447)
            G._inject(mops, CS.flat(plans[mode][r][CS.ALPHA_EVERY]), MixedOp, mode)
            net.unused_modules_off()
            loss = loss_fn(net(inp_pos), net(inp_negc), net(inp_negi))
            loss += 0 * sum(p.sum() for p in net.alpha_prob_parameters())
            loss += 0 * sum(p.sum() for p in net.net_parameters())
            net.zero_grad()
            loss.backward()
            losses.append(loss.item())
            net.set_arch_param_grad()
            alpha_optim.step()
            if MixedOp.MODE == 'two':
                net.rescale_updated_arch_param()
            net.unused_modules_back()
            MixedOp.MODE = None
            alphas.append(np.stack([np.pad(m.alpha_prob.detach().double().numpy(), (0, 4 - m.n_choices)) for m in mops]))
    finally:
        MixedOp.MODE = None
    sd = net.state_dict()
    return dict(losses=np.array(losses, np.float64), alphas=np.stack(alphas),
                weights={k: sd[k].detach().double().numpy().copy() for k in CS.weight_keys(plans)})


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def gen(fname='itm_search_traj.npz'):
    c, batches, plans = CS.setup()
    names = G.ROA.OpsAdapter().Used_OPS
    assert len(names['enc_safe']) == 2 and len(names['dec_safe']) == 4
    out = {'weight_keys': np.array(CS.weight_keys(plans))}
    arrs = {}
    for name, pairs in (('t0', batches['train'][0]), ('t1', batches['train'][1]), ('e', batches['eval'])):
        for j, tup in enumerate(pairs):
            for i, a in enumerate(tup):
                arrs['%s%d%d' % (name, j, i)] = a
    out['inputs_checksum'] = np.float64(cases.checksum(arrs))
    for mode in CS.MODES:
        r32, r64 = run_reference(mode, torch.float32), run_reference(mode, torch.float64)
        worst = {'losses': rel(r32['losses'], r64['losses']), 'alphas': rel(r32['alphas'], r64['alphas']),
                 'weights': max(rel(r32['weights'][k] - c['P'][k], r64['weights'][k] - c['P'][k]) for k in r32['weights'])}
        print(mode, 'float32 run against float64 run:', worst, 'losses', r32['losses'])
        assert worst['losses'] < 1e-5 and worst['alphas'] < 1e-4 and worst['weights'] < 1e-2, worst
        out[mode + '|losses'] = r32['losses']
        out[mode + '|alphas'] = r32['alphas'].astype(np.float32)
        for k, v in r32['weights'].items():
            out['%s|P:%s' % (mode, k)] = v.astype(np.float32)
            assert np.abs(v - c['P'][k]).max() > 0, k            # the recorded tensors do move
        for r in range(CS.ROUNDS):
            for s, plan in enumerate(plans[mode][r]):
                out['%s|plan%d_%d' % (mode, r, s)] = np.array(
                    [[a[0], i[0] if len(i) == 1 else -1] for a, i in CS.flat(plan)], np.int64)
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, len(out), 'arrays,', os.path.getsize(os.path.join(HERE, fname)), 'bytes')


if __name__ == '__main__':
    gen()
