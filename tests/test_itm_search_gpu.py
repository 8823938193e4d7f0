"""The ITM search loop on the MI355X: SearchLoop + harness.triplet_batch / BatchedTriplet replay tests/golden/itm_search_traj.npz
-- the reference's own statements of search_itm.py:381-447 (three forwards per step), two bilevel rounds in each ALPHA_BINARY_MODE,
made by tests/golden/make_golden_itm_search.py -- and one weight step as the 3B batch against three B-forwards.

MMNAS_ITM_SEARCH_STATS=<file>: the worst errors of the replay are written there as json."""
import json
import os

import numpy as np
import pytest
import torch

from tests import supernet_plans as SP
from tests.golden import cases_itm_search as CS
from tests.util import load, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy
STATS = {}


def _dev(t):
    return tuple(T(a).to(DEV) for a in t)


def _write_stats():
    path = os.environ.get('MMNAS_ITM_SEARCH_STATS')
    if path:
        with open(path, 'w') as f:
            json.dump(STATS, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('mode,fused', [('full', False), ('two', False), ('two', True)], ids=['full', 'two', 'two_fused_update'])
def test_itm_search_trajectory_vs_reference_loop(mode, fused):
    """Bars: 1e-3 relative (max-norm) on the losses, on the alphas after every arch step and on the three recorded weight
    tensors -- the bar of test_harness_gpu.py's trajectory test for its alphas.  At the script's learning rate four steps
    move a weight by 2.5e-4 at most, which 1e-3 of a tensor whose largest entry is 0.4 does not resolve; so the MOTION of each
    recorded tensor is compared too, as check_trajectory does (its tol_delta): the norm of the difference of the two motions
    within 2e-2 of the norm of the reference's motion."""
    from mmnas_amd.harness import BCE_Loss, BatchedTriplet, SearchLoop, triplet_batch
    npz = load('itm_search_traj.npz')
    c, batches, plans = CS.setup()
    H = CS.HYPER
    net = SP.build_supernet(c, DEV).train()
    loop = SearchLoop(net, loss_fn=BatchedTriplet(BCE_Loss(c['cfg'])), net_lr=H['net_lr'], net_betas=H['net_betas'],
                      net_eps=H['net_eps'], clip=H['clip'], epoch_steps=H['epoch_steps'], warmup=True, alpha_lr=H['alpha_lr'],
                      alpha_betas=H['alpha_betas'], alpha_every=CS.ALPHA_EVERY, arch_mode=mode, fused_arch_update=fused)
    try:
        train = [triplet_batch(_dev(pos), _dev(neg)) for pos, neg in batches['train']]
        held_out = triplet_batch(*(_dev(t) for t in batches['eval']))
        assert train[0][0].shape[0] == 3 * CS.B
        losses, alphas = [], []
        for r in range(CS.ROUNDS):
            for s in range(CS.ALPHA_EVERY):
                losses.append(float(loop.weight_step(train[s], None, plan=CS.flat(plans[mode][r][s])).detach()))
            losses.append(float(loop.arch_step(held_out, None, plan=CS.flat(plans[mode][r][CS.ALPHA_EVERY])).detach()))
            alphas.append(np.stack([np.pad(m.alpha_prob.detach().cpu().numpy(), (0, 4 - m.n_choices))
                                    for m in net.redundant_modules]))
        named = dict(net.named_parameters())
        weights = {k: named[k].detach().cpu().numpy() for k in CS.weight_keys(plans)}
    finally:
        loop.reducer.fg.disable_sinks()
    want = npz[mode + '|losses']
    st = STATS.setdefault('%s%s' % (mode, '_fused_update' if fused else ''), {})
    st['loss'] = float(np.max(np.abs(np.array(losses) - want) / np.abs(want)))
    st['alphas'] = rel_err(np.stack(alphas), npz[mode + '|alphas'])
    st['weights'] = {k: rel_err(v, npz['%s|P:%s' % (mode, k)]) for k, v in weights.items()}
    st['weight_motion'] = {}
    for k, v in weights.items():
        ref_motion = npz['%s|P:%s' % (mode, k)].astype(np.float64) - c['P'][k]
        st['weight_motion'][k] = float(np.linalg.norm((v.astype(np.float64) - c['P'][k]) - ref_motion) / np.linalg.norm(ref_motion))
    print('ITM search replay, mode %s%s: %s' % (mode, ' (fused update)' if fused else '', json.dumps(st)))
    _write_stats()
    assert st['loss'] <= 1e-3, (losses, want.tolist())
    assert st['alphas'] <= 1e-3
    assert max(st['weights'].values()) <= 1e-3
    assert max(st['weight_motion'].values()) <= 2e-2


def test_the_3B_batch_is_three_B_forwards():
    """One weight step at dropout 0: the loss and the flat gradient of the 3B batch through SearchLoop against three forwards of B
    samples with itm_triplet_step's accumulation (plain autograd on a second copy of the net), to 1e-5 relative."""
    from mmnas.model.mixed import MixedOp
    from mmnas_amd.harness import BCE_Loss, BatchedTriplet, SearchLoop, itm_triplet_step, triplet_batch
    c, batches, plans = CS.setup()
    plan = CS.flat(plans['full'][0][0])
    pos, neg = (_dev(t) for t in batches['train'][0])
    net = SP.build_supernet(c, DEV).train()
    loop = SearchLoop(net, loss_fn=BatchedTriplet(BCE_Loss(c['cfg'])))
    try:
        loss_3b = float(loop.weight_step(triplet_batch(pos, neg), None, optimize=False, plan=plan).detach())
        fg = loop.reducer.fg
        names = {id(p): n for n, p in net.named_parameters()}
        got = {names[id(p)]: v.detach().clone() for p, v in zip(fg.params, fg.views)}
    finally:
        loop.reducer.fg.disable_sinks()
    three = SP.build_supernet(c, DEV).train()
    assert MixedOp.MODE is None
    three.set_sampled(plan)
    loss_3 = float(itm_triplet_step(three, BCE_Loss(c['cfg']), pos, neg).detach())
    named = dict(three.named_parameters())
    want = {k: (named[k].grad if named[k].grad is not None else torch.zeros_like(named[k])) for k in got}
    sampled = [k for k in got if named[k].grad is not None]
    assert len(sampled) > 100 and any('candidate_ops' in k for k in sampled)
    flat_got = torch.cat([got[k].reshape(-1) for k in got]).cpu().numpy()
    flat_want = torch.cat([want[k].reshape(-1) for k in got]).cpu().numpy()
    e_loss, e_grad = abs(loss_3b - loss_3) / abs(loss_3), rel_err(flat_got, flat_want)
    STATS['batched_vs_three_forwards'] = {'loss': e_loss, 'flat_gradient': e_grad}
    print('3B batch vs three B-forwards: loss %.3e, flat gradient %.3e (%d elements)' % (e_loss, e_grad, flat_got.size))
    _write_stats()
    assert e_loss <= 1e-5 and e_grad <= 1e-5
