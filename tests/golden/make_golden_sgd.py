"""Generate tests/golden/traj_sgd.npz: the reference's own loop statements (search_vqa.py:279-337) on the reference
Net_Search with the NET_OPTIM = 'sgd' branch -- torch.optim.SGD(net_parameters(), NET_LR_BASE, momentum, weight_decay)
under CosineAnnealingLR(MAX_EPOCH, eta_min=NET_LR_MIN) stepped at the top of an epoch (search_vqa.py:175-177,243-244,261-262)
-- and alpha_optim with ALPHA_WEIGHT_DECAY.  Needs the reference tree, like make_golden.py (whose helpers it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sgd.py

Sequence: lr_scheduler.step(), weight steps w1, w2, lr_scheduler.step(), w3, one 'full' arch step, the forward loss of a
further weight step.  Keys as traj.npz's (make_golden.gen_traj) with a third weight snapshot 'w3', and traj|lr = the rate
each of the three optimizer steps ran at.  Recorded results only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np
import torch

from tests.golden import cases
from tests.golden.cases_sgd import SGD_HYPER as H, SGD_WEIGHT_PLANS
from tests.golden import make_golden as G

T = torch.from_numpy


def gen_traj_sgd(fname='traj_sgd.npz'):
    out = {}
    MixedOp = G.RMIX.MixedOp
    c, c2, plans = cases.traj_setup()
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = G.hygr_vqa.Net_Search(c['cfg'], init)
    net.train()
    G.load_state(net, c['P'])
    net_optim = torch.optim.SGD(net.net_parameters(), H['net_lr'], momentum=H['net_momentum'], weight_decay=H['net_weight_decay'])
    alpha_optim = torch.optim.Adam(net.alpha_prob_parameters(), H['alpha_lr'], betas=H['alpha_betas'],
                                   weight_decay=H['alpha_weight_decay'])
    lr_scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(net_optim, H['max_epoch'], eta_min=H['net_lr_min'])
    loss_fn = torch.nn.BCEWithLogitsLoss(reduction='sum')
    mops = net.redundant_modules
    inp = tuple(T(a) for a in c['inputs']); tgt = T(c['target'])
    inp2 = tuple(T(a) for a in c2['inputs']); tgt2 = T(c2['target'])
    losses, gnorms, lrs = [], [], []
    P0 = {k: v.detach().clone() for k, v in net.state_dict().items()}

    def weight_step(plan, step_optim=True):
        G._inject(mops, plan['enc'] + plan['dec'], MixedOp, None)
        net.unused_modules_off()
        pred = net(inp)
        loss = loss_fn(pred, tgt)
        loss += 0 * sum(p.sum() for p in net.alpha_prob_parameters())
        loss += 0 * sum(p.sum() for p in net.alpha_gate_parameters())
        loss += 0 * sum(p.sum() for p in net.net_parameters())
        net.zero_grad()
        loss.backward()
        losses.append(loss.item())
        if step_optim:
            gnorms.append(float(torch.nn.utils.clip_grad_norm_(net.net_parameters(), H['clip'])))
            lrs.append(net_optim.param_groups[0]['lr'])
            net_optim.step()
        net.unused_modules_back()

    def snapshot(tag):
        sd = net.state_dict()
        keys = sorted(k for k in sd if 'alpha' not in k)
        out['traj|%s|keys' % tag] = np.array(keys)
        out['traj|%s|delta_norm' % tag] = np.array([float((sd[k].double() - P0[k].double()).norm()) for k in keys])
        ds = [G.esample(sd[k].double() - P0[k].double()) for k in keys]
        out['traj|%s|delta_sample' % tag] = np.concatenate(ds)
        out['traj|%s|delta_off' % tag] = np.cumsum([0] + [d.size for d in ds]).astype(np.int64)
        for k in cases.TRAJ_FULL_KEYS:
            out['traj|%s|P:%s' % (tag, k)] = sd[k].detach().numpy().copy()

    w = [plans[i] for i in SGD_WEIGHT_PLANS]
    lr_scheduler.step()
    weight_step(w[0]); snapshot('w1')
    weight_step(w[1]); snapshot('w2')
    lr_scheduler.step()
    weight_step(w[2]); snapshot('w3')
    # arch step (search_vqa.py:317-337)
    G._inject(mops, plans[2]['enc'] + plans[2]['dec'], MixedOp, 'full')
    net.unused_modules_off()
    pred = net(inp2)
    loss = loss_fn(pred, tgt2)
    loss += 0 * sum(p.sum() for p in net.alpha_prob_parameters())
    loss += 0 * sum(p.sum() for p in net.net_parameters())
    net.zero_grad()
    loss.backward()
    losses.append(loss.item())
    out['traj|arch|gate_grads'] = np.stack([np.pad(m.alpha_gate.grad.numpy(), (0, 4 - m.n_choices)) for m in mops])
    net.set_arch_param_grad()
    out['traj|arch|prob_grads'] = np.stack([np.pad(m.alpha_prob.grad.numpy(), (0, 4 - m.n_choices)) for m in mops])
    alpha_optim.step()
    net.unused_modules_back()
    MixedOp.MODE = None
    out['traj|arch|alpha_after'] = np.stack([np.pad(m.alpha_prob.detach().numpy(), (0, 4 - m.n_choices)) for m in mops])
    snapshot('a')   # the arch step must leave the network weights alone
    weight_step(w[3], step_optim=False)
    out['traj|losses'] = np.array(losses, np.float64)
    out['traj|grad_norms'] = np.array(gnorms, np.float64)
    out['traj|lr'] = np.array(lrs, np.float64)
    for i, pl in enumerate(plans):
        out['traj|plan%d' % i] = np.array([a[0] for a, _ in pl['enc'] + pl['dec']], np.int64)
    np.savez_compressed(os.path.join(HERE, fname), **out)
    print(fname, len(out), 'arrays; losses', losses, 'grad norms', gnorms, 'lr', lrs)


if __name__ == '__main__':
    gen_traj_sgd()
