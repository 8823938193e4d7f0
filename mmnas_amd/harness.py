"""Step harness: the statement sequences of the reference's entry scripts around the hot path, as calls.

The reference scripts cannot be imported (datasets, spaCy, torchvision); what they DO per step is short and is
restated here against the same model API, so that the bench, the tests and an integrator's loop share one
implementation:

  * SearchLoop.weight_step / arch_step / bilevel_round -- search_vqa.py:279-337 (and its _vgd / _itm twins):
    sample -> forward -> loss -> backward -> (gradient exchange) -> clip + Adam, and every ALPHA_EVERY-th step the
    architecture step in mode 'full'.  Differences from the script are mechanical, not arithmetic:
      - no `0 * sum(p.sum())` terms (search_vqa.py:285-288): they exist to give DDP a gradient for every parameter.
        Their arithmetic consequence -- torch Adam steps EVERY net parameter at every step, unsampled candidates
        included (zero gradient, decaying moments, stale-momentum motion) -- is kept by FlatAdam(absent_grads='zero');
      - gradients live in one flat buffer (dp.SupernetReducer); clip_grad_norm_ + Adam are two kernels (optim.FlatAdam);
      - the arch step's alpha gradient + alpha_optim.step() are one kernel (ArchAdam, mode 'full'; mode 'two', with the
        pair's rescale in the same kernel, under fused_arch_update=True).
    Pinned against the reference loop itself by tests/golden/traj.npz (tests/test_harness_gpu.py::test_bilevel_trajectory_vs_reference_loop).
    net_optim='sgd' is the scripts' other NET_OPTIM branch (search_vqa.py:122-131,175-177,228-244,261): optim.FlatSGD +
    optim.CosineSchedule stepped by begin_epoch(); pinned by tests/golden/traj_sgd.npz (tests/test_sgd_gpu.py).
  * itm_triplet_step -- train_itm.py:380-391: three forwards (positive, negative caption, negative image), BCE_Loss.
  * triplet_batch / BatchedTriplet -- the triplet steps of search_itm.py:381-447 for SearchLoop: the three forwards as one batch
    of 3B samples, the three-argument loss over the three thirds of its scores.  Pinned against the reference's three forwards by
    tests/golden/itm_search_traj.npz (tests/test_itm_search_gpu.py).
  * BCE_Loss -- mmnas/utils/itm_loss.py:4-24.  vgd_loss -- train_vgd.py:316-333.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import cost as cost_tables
from . import dp, ops
from .model.mixed import MixedOp
from .optim import CosineSchedule, FlatAdam, FlatSGD, WarmupOptimizer


class BCEWithLogitsSum(nn.Module):
    """torch.nn.BCEWithLogitsLoss(reduction='sum') (search_vqa.py:211) as one HIP kernel per direction on the GPU."""

    def forward(self, pred, target):
        if pred.is_cuda and pred.dtype == torch.float32:
            return ops.bce_with_logits_sum(pred, target)
        return F.binary_cross_entropy_with_logits(pred, target, reduction='sum')


def fused_loss(loss_fn):
    """The HIP form of a loss module the scripts use, when there is one."""
    if isinstance(loss_fn, nn.BCEWithLogitsLoss) and loss_fn.reduction == 'sum' and loss_fn.weight is None and loss_fn.pos_weight is None:
        return BCEWithLogitsSum()
    return loss_fn


class BCE_Loss(nn.Module):
    """mmnas/utils/itm_loss.py:4-24: BCE on the sigmoid scores, label 1 for the matching pair and 0 for the two
    negatives; the positive term enters twice (`loss_pos + loss_negc + loss_pos + loss_negi`)."""

    def __init__(self, __C=None):
        super().__init__()
        self.reduction = getattr(__C, 'REDUCTION', 'sum') if __C is not None else 'sum'

    def forward(self, scores_pos, scores_negc, scores_negi):
        lp = F.binary_cross_entropy(scores_pos, torch.ones_like(scores_pos), reduction=self.reduction)
        lc = F.binary_cross_entropy(scores_negc, torch.zeros_like(scores_negc), reduction=self.reduction)
        li = F.binary_cross_entropy(scores_negi, torch.zeros_like(scores_negi), reduction=self.reduction)
        return lp + lc + lp + li


def vgd_loss(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask, lam=0.5, scores_loss='kld', loss_avg=True,
             batch_size=None):
    """train_vgd.py:316-333 (REDUCTION='sum'): KLDiv (or BCE-with-logits) on the masked scores + lam * SmoothL1 on the
    masked box targets, each divided by its mask count when LOSS_AVG."""
    if scores_loss == 'bce':
        ls = F.binary_cross_entropy_with_logits(pred_scores, scores, reduction='sum')
    else:
        ls = F.kl_div(pred_scores * scores_mask, scores * scores_mask, reduction='sum')
    lr = F.smooth_l1_loss(pred_reg * bbox_mask, bbox * bbox_mask, reduction='sum')
    if loss_avg:
        if batch_size is None:
            batch_size = pred_scores.shape[0]     # train_vgd.py divides by the loader's batch size
        ls = ls / (batch_size if scores_loss == 'bce' else scores_mask.sum())
        lr = lr / bbox_mask.sum()
    return ls + lam * lr


def itm_triplet_step(net, loss_fn, pos, neg, reducer=None, optim=None):
    """train_itm.py:380-395: `pos` / `neg` are the 5-tuples (frcn, bbox, rel_img, cap_ix, rel_cap) of the matching
    pair and of the mined negatives; three forwards share the weights, one backward."""
    if reducer is not None:
        reducer.begin_step()
    elif optim is not None:
        optim.zero_grad()
    negc = (pos[0], pos[1], pos[2], neg[3], neg[4])
    negi = (neg[0], neg[1], neg[2], pos[3], pos[4])
    loss = loss_fn(net(pos), net(negc), net(negi))
    loss.backward()
    if reducer is not None:
        reducer.finish()
    if optim is not None:
        optim.step()
    return loss


def triplet_batch(pos, neg):
    """The three forwards of an ITM triplet step (search_itm.py:373-375,385-387) as ONE batch of 3B samples
    [pos; negc; negi]: the image fields (frcn, bbox, rel_img) come from (pos, pos, neg), the caption fields (cap_ix, rel_cap)
    from (pos, neg, pos).  `pos` / `neg` are the 5-tuples of the matching pairs and of the mined negatives."""
    def cat(i, a, b, c):
        if a[i] is None:
            return None
        out = torch.cat((a[i], b[i], c[i]), 0)
        # the parts' lengths (data.DevicePrefetcher(lengths=...)) travel with the batch: without them the ragged streams
        # (ops.set_unpad / set_unpad_x) pay a device-to-host copy for every fresh 3B batch
        lens = [getattr(t, '_mmnas_lengths', None) for t in (a[i], b[i], c[i])]
        if all(l is not None for l in lens):
            out._mmnas_lengths = [int(v) for l in lens for v in l]
        return out
    return (cat(0, pos, pos, neg), cat(1, pos, pos, neg), cat(2, pos, pos, neg), cat(3, pos, neg, pos), cat(4, pos, neg, pos))


class BatchedTriplet(nn.Module):
    """A three-argument ITM loss (BCE_Loss, Margin_Loss, losses.TripletBCELoss, ...) behind the (prediction, target) signature
    of SearchLoop / TrainLoop: forward(scores, target) = loss_fn(scores[:B], scores[B:2B], scores[2B:]) for the [3B] scores of
    a triplet_batch; the target is ignored.  fused_loss() and losses.fused() hand it back unchanged (wrap the fused loss
    instead: BatchedTriplet(losses.fused(BCE_Loss(cfg)))).

        loop = SearchLoop(net, loss_fn=BatchedTriplet(BCE_Loss(cfg)), arch_mode=...)
        loop.weight_step(triplet_batch(pos, neg), None)      # search_itm.py:381-406
        loop.arch_step(triplet_batch(epos, eneg), None)      # search_itm.py:408-447

    One forward over 3B samples is, sample by sample, the arithmetic of the script's three forwards under the one sampled
    architecture, with a third of the launches.  Dropout masks are drawn per sample of the one batch: the same distribution as
    the three forwards', not the same draws."""

    def __init__(self, loss_fn):
        super().__init__()
        self.loss_fn = loss_fn

    def forward(self, scores, target=None):
        if scores.shape[0] % 3:
            raise ValueError('BatchedTriplet: %d scores are not the 3B of a triplet_batch' % scores.shape[0])
        B = scores.shape[0] // 3
        return self.loss_fn(scores[:B], scores[B:2 * B], scores[2 * B:])


def hard_negative_indices(scores, neg_idx, hard_size):
    """The selection step of the ITM hard-negative mining pass (train_itm.py:349-353): `scores` are the net's matching
    scores of every anchor against its NEG_RANDSIZE random candidates (flattened), `neg_idx` [N, NEG_RANDSIZE] the
    candidates' dataset indices; returns [N, hard_size] -- per anchor the indices of its highest-scoring candidates."""
    scores = scores.view(-1, neg_idx.shape[1])
    top = torch.argsort(scores, dim=-1, descending=True)[:, :hard_size]
    rows = torch.arange(top.size(0), device=top.device).unsqueeze(1).expand_as(top)
    return neg_idx.to(scores.device)[rows, top]


class NegLossReward:
    """reward(pred, target) = -scale * loss_fn(pred, target): the default reward of SearchLoop(arch_mode='reinforce'), the
    loop's own loss with scale = 1 / batch size.  Works with every loss of the three tasks (VgdLoss and BatchedTriplet
    included).  It is negative, so it suits reward_form 'add'; with 'mul' and a cost table the loop raises ValueError."""

    def __init__(self, loss_fn, scale=1.0):
        self.loss_fn, self.scale = loss_fn, float(scale)

    def __call__(self, pred, target):
        return -self.scale * self.loss_fn(pred, target)


def _sample_plain(net, plan):
    """One MODE = None sample that leaves every .grad as it is: drawn from the alphas, or an injected (active, inactive)
    list per node."""
    if plan is not None:
        net.set_sampled(plan)
        return
    keep = getattr(net, 'keep_candidate_grads', False)
    net.keep_candidate_grads = True
    try:
        net.reset_binary_gates()
    finally:
        net.keep_candidate_grads = keep


def reinforce_arch_step(net, alpha_optim, reward, inputs, target, reducer=None, optimize=True, plan=None):
    """The REINFORCE architecture step of SearchLoop(arch_mode='reinforce'): for each of alpha_optim.n_samples samples, sample
    with MixedOp.MODE = None, record the row of active indices, run pred = net(inputs) in eval mode under no_grad and copy
    reward(pred, target) (a device scalar) into alpha_optim.quality on the device; then alpha_optim.step(), one launch.  No
    backward, no begin_arch_step, no write to a gradient or a weight; every module's training flag and MixedOp.MODE = None are
    put back, also after an exception.  `plan`: a list of n_samples plans (tests, replay).  With a `reducer` whose process
    group is up, the [M] rewards are averaged over the ranks with ONE all-reduce before the update: every rank samples the
    same M architectures (mixed.seed_arch_sampler alike) on its own shard, so the ranks' alphas stay bit-identical.
    Returns the mean quality, a device tensor."""
    M = alpha_optim.n_samples
    if plan is not None and len(plan) != M:
        raise ValueError("arch_step(arch_mode='reinforce'): plan is a list of %d plans, one per sample, got %d" % (M, len(plan)))
    flags = [(m, m.training) for m in net.modules()]
    MixedOp.MODE = None
    try:
        net.eval()
        with torch.no_grad():
            for i in range(M):
                _sample_plain(net, None if plan is None else plan[i])
                alpha_optim.choice[i] = torch.tensor([int(m.active_index[0]) for m in net.redundant_modules])
                q = reward(net(inputs), target)
                alpha_optim.quality[i].copy_(q.detach().reshape(()))      # device to device
    finally:
        for m, t in flags:
            m.training = t
        MixedOp.MODE = None
    if reducer is not None and reducer.comm:
        dp._all_reduce_avg(alpha_optim.quality, reducer.group, reducer.world)
    mean = alpha_optim.quality.mean()
    if optimize:
        alpha_optim.step()
    return mean


class ArchAdam:
    """alpha_optim of search_vqa.py:194 (torch.optim.Adam over alpha_prob_parameters, lr 0.1, betas (0, 0.999)) fused
    with Net_Search.set_arch_param_grad() for ALPHA_BINARY_MODE 'full': one kernel over the [n_nodes, width] blocks.
    mode='two': the same for ALPHA_BINARY_MODE 'two' -- set_arch_param_grad over each node's sampled pair, the Adam step and
    rescale_updated_arch_param (search_vqa.py:330-335, mixed.py:179-208) as one kernel (ops.alpha_two_step); the pairs are
    read from the nodes' active_index / inactive_index when step() runs.  The checkpoint format is the same in both modes.
    cost (a [nodes, width] block or a cost.CostTable) with cost_weight > 0: the expected-cost regulariser of a hardware-aware
    search, 'linear' or 'log' around cost_ref (default: the expected cost under uniform alphas), joins the objective in the
    same launch (ops.alpha_cost_step); `cost_stats` then holds E_r per node, E and R of the last update on the device.
    mode='reinforce': the REINFORCE update (ops.alpha_reinforce_step) -- no gate gradients.  The caller records the
    n_samples sampled architectures in `choice` (a CPU [M, nodes] int64 block) and their rewards in `quality` (device [M],
    never read by the host); step() is the one launch.  `baseline` (device: value, initialised) is the moving average of the
    mean reward, `reinforce_stats` (device [M + 3]) R_i, mean R, the baseline used and the one after, `err` (device int32)
    is set -- and nothing moves -- when a reward is not finite.  Here cost prices the architecture actually sampled,
    reward_form 'mul' (R = Q (C / cost_ref)^w) or 'add' (R = Q + w log(C / cost_ref)), and cost_weight may be negative.
    state_dict() adds one top-level key 'reinforce' (baseline, initialised) to torch Adam's format."""

    def __init__(self, net, lr=0.1, betas=(0.0, 0.999), eps=1e-8, weight_decay=0, mode='full', cost=None, cost_weight=0.0,
                 cost_form='linear', cost_ref=None, n_samples=4, baseline_decay=0.95, reward_form='mul'):
        if mode not in ('full', 'two', 'reinforce'):
            raise ValueError("ArchAdam: mode is 'full', 'two' or 'reinforce', got %r" % (mode,))
        self.mode = mode
        if mode == 'reinforce':
            self._init_reinforce(net, lr, betas, eps, weight_decay, cost, cost_weight, cost_ref, n_samples, baseline_decay,
                                 reward_form)
            return
        self.net, self.lr, self.betas, self.eps = net, lr, betas, eps
        self.weight_decay = weight_decay      # ALPHA_WEIGHT_DECAY (search_vqa.py:156-157,195)
        prob, _ = net._flat_alphas()
        self.m = torch.zeros_like(prob)
        self.v = torch.zeros_like(prob)
        self.steps = 0
        # hardware-aware search: the expected-cost regulariser joins the objective inside the same launch
        # (ops.alpha_cost_step).  Configuration, not state: nothing of it enters state_dict().  Without a table or with
        # cost_weight == 0 step() is the update above, call for call.
        self.cost = self.cost_stats = None
        self.cost_weight, self.cost_form, self.cost_ref = float(cost_weight), cost_form, cost_ref
        if cost is not None and self.cost_weight != 0.0:
            if cost_form not in ops.COST_FORMS:
                raise ValueError("ArchAdam: cost_form is 'linear' or 'log', got %r" % (cost_form,))
            if not (math.isfinite(self.cost_weight) and self.cost_weight > 0):
                raise ValueError('ArchAdam: cost_weight must be finite and not negative, got %r' % (cost_weight,))
            self.cost, self.cost_ref = self._prepare_cost(net, cost, cost_form, cost_ref)
            self.cost_stats = torch.zeros(prob.shape[0] + 2, device=prob.device)      # E_r per node, E, R of the last update

    @staticmethod
    def _prepare_cost(net, cost, form, cost_ref):
        """-> (the checked [nodes, width] cost block on the alphas' device, cost_ref: by default the expected cost under
        uniform alphas)."""
        prob, _ = net._flat_alphas()
        n_choices = [m.n_choices for m in net.redundant_modules]
        block = cost.for_net(net, form) if isinstance(cost, cost_tables.CostTable) else cost
        if tuple(block.shape) != tuple(prob.shape):
            raise ValueError('ArchAdam: the cost block is %s, the alpha block %s' % (tuple(block.shape), tuple(prob.shape)))
        block = cost_tables.check_block(block.detach().to('cpu', torch.float32), n_choices, form)
        cost_ref = float(cost_tables.uniform_expected(block, n_choices) if cost_ref is None else cost_ref)
        if not (math.isfinite(cost_ref) and cost_ref > 0):
            raise ValueError('ArchAdam: cost_ref must be finite and positive, got %r (the default is the expected cost under '
                             'uniform alphas: pass one for a table of zeros)' % (cost_ref,))
        return block.to(prob.device).contiguous(), cost_ref

    def _init_reinforce(self, net, lr, betas, eps, weight_decay, cost, cost_weight, cost_ref, n_samples, baseline_decay, reward_form):
        self.net, self.lr, self.betas, self.eps, self.weight_decay = net, lr, betas, eps, weight_decay
        prob, _ = net._flat_alphas()
        rows, width = prob.shape
        self.m, self.v, self.steps = torch.zeros_like(prob), torch.zeros_like(prob), 0
        if int(n_samples) != n_samples or n_samples < 1:
            raise ValueError("ArchAdam(mode='reinforce'): n_samples >= 1, got %r" % (n_samples,))
        self.n_samples = M = int(n_samples)
        if prob.is_cuda and (M > ops.ALPHA_REINFORCE_MAX_SAMPLES or M * rows > ops.ALPHA_REINFORCE_MAX_CHOICES):
            raise ValueError("ArchAdam(mode='reinforce'): %d samples of %d nodes; at most %d samples and %d indices travel with "
                             "the launch" % (M, rows, ops.ALPHA_REINFORCE_MAX_SAMPLES, ops.ALPHA_REINFORCE_MAX_CHOICES))
        if reward_form not in ops.REWARD_FORMS:
            raise ValueError("ArchAdam: reward_form is 'mul' or 'add', got %r" % (reward_form,))
        self.baseline_decay, self.reward_form = float(baseline_decay), reward_form
        if not 0.0 <= self.baseline_decay < 1.0:
            raise ValueError('ArchAdam: baseline_decay lies in [0, 1), got %r' % (baseline_decay,))
        self.n_choices = [m.n_choices for m in net.redundant_modules]
        self.cost = self.cost_stats = None
        self.cost_weight, self.cost_form, self.cost_ref = float(cost_weight), None, cost_ref
        if not math.isfinite(self.cost_weight):
            raise ValueError('ArchAdam: cost_weight must be finite, got %r' % (cost_weight,))
        if cost is not None and self.cost_weight != 0.0:
            self.cost, self.cost_ref = self._prepare_cost(net, cost, 'linear', cost_ref)
        else:
            self.cost_ref = 1.0 if cost_ref is None else float(cost_ref)
        dev = prob.device
        self.choice = torch.zeros(M, rows, dtype=torch.int64)                  # host: it travels in the kernel arguments
        self.quality = torch.zeros(M, device=dev)
        self.baseline = torch.zeros(2, device=dev)                             # (value, initialised)
        self.reinforce_stats = torch.zeros(M + 3, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)

    def _step_reinforce(self):
        net = self.net
        prob, _ = net._flat_alphas()
        if net._flat_grads is None:
            net._flat_grads = (torch.zeros_like(prob), torch.zeros_like(prob))
        pg = net._flat_grads[1]
        self.steps += 1
        ops.alpha_reinforce_step(prob, self.m, self.v, pg, self.choice, self.quality, self.baseline, self.lr, self.betas, self.eps,
                                 self.steps, self.weight_decay, cost=self.cost, cost_weight=self.cost_weight, cost_ref=self.cost_ref,
                                 reward_form=self.reward_form, baseline_decay=self.baseline_decay, stats=self.reinforce_stats,
                                 err=self.err, n_choices=self.n_choices)
        self._publish(pg)

    def _sampled_pairs(self):
        pairs = []
        for i, m in enumerate(self.net.redundant_modules):
            act, inact = m.active_index, m.inactive_index
            if not act or not inact or len(act) != 1 or len(inact) != 1:
                raise ValueError("ArchAdam(mode='two'): node %d has no sampled pair (active_index %r, inactive_index %r): "
                                 "sample with MixedOp.MODE = 'two' first" % (i, act, inact))
            a, b = int(act[0]), int(inact[0])
            if a == b or not (0 <= a < m.n_choices and 0 <= b < m.n_choices):
                raise ValueError("ArchAdam(mode='two'): node %d: pair (%d, %d) must be two different candidates of 0..%d"
                                 % (i, a, b, m.n_choices - 1))
            pairs.append((a, b))
        return pairs

    def step(self):
        if self.mode == 'reinforce':
            return self._step_reinforce()
        net = self.net
        prob, _ = net._flat_alphas()
        gg, pg = net._flat_grads
        pairs = self._sampled_pairs() if self.mode == 'two' else None      # (before anything is written)
        for i, m in enumerate(net.redundant_modules):    # gate gradients autograd produced outside the block
            g = m.alpha_gate.grad
            if g is not None and g.data_ptr() != gg[i].data_ptr():
                gg[i, :m.n_choices].copy_(g)
        self.steps += 1
        if self.cost is not None:
            ops.alpha_cost_step(prob, gg, self.m, self.v, pg, self.cost, self.lr, self.betas, self.eps, self.steps, self.weight_decay,
                                cost_weight=self.cost_weight, cost_ref=self.cost_ref, cost_form=self.cost_form, pairs=pairs,
                                stats=self.cost_stats)
        elif pairs is not None:
            ops.alpha_two_step(prob, gg, self.m, self.v, pg, pairs, self.lr, self.betas, self.eps, self.steps, self.weight_decay)
        else:
            ops.alpha_full_step(prob, gg, self.m, self.v, pg, self.lr, self.betas, self.eps, self.steps, self.weight_decay)
        self._publish(pg)

    def _publish(self, pg):
        for i, m in enumerate(self.net.redundant_modules):
            m.alpha_prob.grad = pg[i, :m.n_choices]
            m.alpha_version += 1                          # (the update wrote through the flat block: drop the sampling cache)

    # torch.optim.Adam's checkpoint format over alpha_prob_parameters() in module order (search_vqa.py:350: the reference
    # saves `alpha_optim.state_dict()` beside the network's)
    def state_dict(self):
        state = {}
        mods = self.net.redundant_modules
        if self.steps:
            for i, m in enumerate(mods):
                n = m.n_choices
                state[i] = {'step': torch.tensor(float(self.steps)), 'exp_avg': self.m[i, :n].clone(),
                            'exp_avg_sq': self.v[i, :n].clone()}
        group = {'lr': self.lr, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': self.weight_decay, 'amsgrad': False,
                 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                 'params': list(range(len(mods)))}
        sd = {'state': state, 'param_groups': [group]}
        if self.mode == 'reinforce':      # (one host read: a checkpoint is being written anyway)
            b = self.baseline.detach().cpu()
            sd['reinforce'] = {'baseline': b[0].clone(), 'initialised': bool(b[1] != 0)}
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        mods = self.net.redundant_modules
        g0 = sd['param_groups'][0]
        order = [i for g in sd['param_groups'] for i in g['params']]
        if len(order) != len(mods):
            raise ValueError('ArchAdam.load_state_dict: %d parameters in the file, %d alpha blocks here' % (len(order), len(mods)))
        self.lr, self.betas, self.eps = g0.get('lr', self.lr), tuple(g0.get('betas', self.betas)), g0.get('eps', self.eps)
        self.weight_decay = g0.get('weight_decay', self.weight_decay)
        self.m.zero_()
        self.v.zero_()
        steps = set()
        for pos, key in enumerate(order):
            st = sd['state'].get(key)
            if st is None:
                continue
            n = mods[pos].n_choices
            self.m[pos, :n].copy_(st['exp_avg'].to(self.m.device, torch.float32))
            self.v[pos, :n].copy_(st['exp_avg_sq'].to(self.v.device, torch.float32))
            steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError('ArchAdam keeps one step count for all alpha blocks; the file holds %s' % sorted(steps))
        self.steps = steps.pop() if steps else 0
        if self.mode == 'reinforce':      # (a file of another mode carries no baseline: a fresh one)
            rf = sd.get('reinforce')
            self.baseline.zero_()
            if rf is not None and rf['initialised']:
                self.baseline[0] = torch.as_tensor(rf['baseline'], dtype=torch.float32)
                self.baseline[1] = 1.0


class TrainLoop:
    """The fixed-architecture training loop body of train_vqa.py:291-311 (train_vgd.py / train_itm.py use the same
    statements around their own losses) for one data-parallel rank: zero_grad, forward, loss, backward with the
    bucketed gradient exchange, clip_grad_norm_, warm-up Adam step -- the clip and the update as two launches over the
    flat buffers.  `decay(r)` is the epoch-boundary learning-rate decay (train_vqa.py:285-287)."""

    def __init__(self, net, loss_fn=None, lr=1e-4, betas=(0.9, 0.98), eps=1e-9, clip=1.0, epoch_steps=1000, warmup=True,
                 group=None, bucket_mb=64.0, force_collectives=False):
        self.net = net
        self.loss_fn = fused_loss(loss_fn if loss_fn is not None else nn.BCEWithLogitsLoss(reduction='sum'))
        self.reducer = dp.GradReducer(list(net.parameters()), bucket_mb=bucket_mb, group=group,
                                      force_collectives=force_collectives)
        # every parameter of a fixed architecture receives a gradient, so "absent gradients" never occur; 'zero' keeps
        # the arithmetic of the reference's `0 * sum(p.sum())` line (train_vqa.py:299) for parameters an architecture
        # leaves unused
        self.net_optim = WarmupOptimizer(lr, FlatAdam(self.reducer.fg.params, betas=betas, eps=eps, grads=self.reducer.fg,
                                                      absent_grads='zero'),
                                         epoch_steps=epoch_steps, warmup=warmup, max_norm=clip if clip and clip > 0 else None)
        self.steps = 0

    def step(self, inputs, target, optimize=True):
        red = self.reducer
        red.begin_step()
        loss = self.loss_fn(self.net(inputs), target)
        loss.backward()
        red.finish()
        if optimize:
            self.net_optim.step()
        self.steps += 1
        return loss

    def decay(self, decay_r):
        self.net_optim.decay(decay_r)


class SearchLoop:
    """The bilevel NAS loop body of search_vqa.py:279-337 for one data-parallel rank.

    net_optim: the scripts' NET_OPTIM.  'wadam' (default): warm-up Adam, `net_lr` = NET_LR_BASE, decay() by the caller.
    'sgd': torch.optim.SGD(net_lr, momentum=net_momentum, weight_decay=net_weight_decay) as FlatSGD under
    CosineAnnealingLR(max_epoch, eta_min=net_lr_min) as CosineSchedule; call begin_epoch(epoch) at the start of every epoch
    (search_vqa.py:261-262).  To resume, pass start_epoch=CKPT_EPOCH and load the checkpoint's 'net_optim' into
    `loop.net_optim` (search_vqa.py:226-231).  net_weight_decay / alpha_weight_decay: NET_WEIGHT_DECAY / ALPHA_WEIGHT_DECAY.
    fused_arch_update (arch_mode='two' only): the architecture update as ArchAdam(mode='two') instead of the per-node
    statements around torch Adam; the checkpoints of the two are interchangeable.
    cost_table / cost_weight / cost_form / cost_ref: ArchAdam's expected-cost term ('two' carries it only under
    fused_arch_update=True); without a table or with cost_weight 0 the architecture update is unchanged.
    arch_mode='reinforce': the architecture step is `reinforce_samples` plain MODE = None forwards in eval mode under no_grad
    -- no backward, no inactive candidates -- each scored by `reward(pred, target)` (a device scalar; default
    NegLossReward(loss_fn, 1 / batch size)), then ArchAdam(mode='reinforce').step(), one launch.  cost_table / cost_weight /
    cost_ref price the sampled architecture in `reward_form` 'mul' or 'add' (cost_weight may be negative: -0.07 is MnasNet's);
    cost_form is not used.  With a process group the [M] rewards are averaged with one all-reduce before the update."""

    def __init__(self, net, loss_fn=None, net_lr=4e-4, net_betas=(0.9, 0.98), net_eps=1e-9, clip=1.0, epoch_steps=1000,
                 warmup=True, alpha_lr=0.1, alpha_betas=(0.0, 0.999), alpha_every=5, arch_mode='full', group=None,
                 absent_grads='zero', n_buckets=3, force_collectives=False, net_optim='wadam', net_momentum=0.9,
                 net_weight_decay=0.0, net_lr_min=0.0005, max_epoch=None, start_epoch=0, alpha_weight_decay=0.0,
                 fused_arch_update=False, cost_table=None, cost_weight=0.0, cost_form='linear', cost_ref=None,
                 reinforce_samples=4, reward=None, baseline_decay=0.95, reward_form='mul'):
        if arch_mode not in ('full', 'two', 'reinforce'):
            raise ValueError("ALPHA_BINARY_MODE is 'full' or 'two' (search_vqa.py:151), got %r" % (arch_mode,))
        if arch_mode == 'reinforce':
            if int(reinforce_samples) != reinforce_samples or reinforce_samples < 1:
                raise ValueError("arch_mode='reinforce': reinforce_samples >= 1, got %r" % (reinforce_samples,))
            priced = cost_table is not None and float(cost_weight) != 0.0
            if priced and reward_form == 'mul' and (reward is None or isinstance(reward, NegLossReward)):
                raise ValueError("arch_mode='reinforce': NegLossReward is negative, and a negative quality times the cost factor of "
                                 "reward_form='mul' rewards cost: use reward_form='add' or a non-negative reward")
        if cost_table is not None and arch_mode == 'two' and not fused_arch_update:
            raise ValueError("cost_table with arch_mode='two' needs fused_arch_update=True: the per-node statements around torch "
                             "Adam do not carry the expected-cost term")
        if net_optim not in ('wadam', 'sgd'):
            raise ValueError("NET_OPTIM is 'wadam' or 'sgd' (search_vqa.py:117-118), got %r" % (net_optim,))
        if net_optim == 'sgd' and max_epoch is None:
            raise ValueError("net_optim='sgd' anneals the rate over MAX_EPOCH epochs (search_vqa.py:131,243-244): pass max_epoch")
        self.net = net
        self.loss_fn = fused_loss(loss_fn if loss_fn is not None else nn.BCEWithLogitsLoss(reduction='sum'))
        dense = absent_grads == 'zero'
        self.reducer = dp.SupernetReducer(net, group=group, n_buckets=n_buckets, force_collectives=force_collectives,
                                          attach_all=dense)
        net.keep_candidate_grads = dense
        max_norm = self._max_norm = clip if clip and clip > 0 else None
        self.lr_scheduler = None
        if net_optim == 'sgd':
            # the script's net_optim IS the torch SGD here (no WarmupOptimizer around it): state_dict() / load_state_dict()
            # are the optimizer's own, the clip travels with every step
            self.net_optim = FlatSGD(self.reducer.fg.params, lr=net_lr, momentum=net_momentum, weight_decay=net_weight_decay,
                                     grads=self.reducer.fg, absent_grads=absent_grads)
            if start_epoch:
                self.net_optim.param_groups[0]['initial_lr'] = net_lr      # (what the checkpoint's param group carries)
            self.lr_scheduler = CosineSchedule(self.net_optim, max_epoch, eta_min=net_lr_min,
                                               last_epoch=start_epoch if start_epoch else -1)
            # (a resumed CosineAnnealingLR counts its constructor's step on top of last_epoch, a fresh one starts at 0)
            self._epoch_shift = self.lr_scheduler.last_epoch - start_epoch
        else:
            self.net_optim = WarmupOptimizer(net_lr, FlatAdam(self.reducer.fg.params, betas=net_betas, eps=net_eps,
                                                              weight_decay=net_weight_decay, grads=self.reducer.fg,
                                                              absent_grads=absent_grads),
                                             epoch_steps=epoch_steps, warmup=warmup, max_norm=max_norm)
        # 'full' (the shipped setting): alpha gradient + Adam as one kernel over the [n_nodes, width] blocks.  'two': the
        # reference's own statements -- MixedOp.set_arch_param_grad over the sampled pair, torch Adam on the alpha
        # parameters, rescale_updated_arch_param (search_vqa.py:330-334, mixed.py:179-208)
        # fused_arch_update=True gives 'two' the same device-resident update: ArchAdam(mode='two'), one launch
        # (ops.alpha_two_step) for those three statements; with 'full' the keyword changes nothing
        self.fused_arch_update = bool(fused_arch_update) and arch_mode == 'two'
        cost_kw = dict(cost=cost_table, cost_weight=cost_weight, cost_form=cost_form, cost_ref=cost_ref)
        self.reward = reward
        if arch_mode == 'reinforce':
            self.alpha_optim = ArchAdam(net, alpha_lr, alpha_betas, weight_decay=alpha_weight_decay, mode='reinforce',
                                        cost=cost_table, cost_weight=cost_weight, cost_ref=cost_ref,
                                        n_samples=int(reinforce_samples), baseline_decay=baseline_decay, reward_form=reward_form)
        elif arch_mode == 'full':
            self.alpha_optim = ArchAdam(net, alpha_lr, alpha_betas, weight_decay=alpha_weight_decay, **cost_kw)
        elif self.fused_arch_update:
            self.alpha_optim = ArchAdam(net, alpha_lr, alpha_betas, weight_decay=alpha_weight_decay, mode='two', **cost_kw)
        else:
            net._flat_alphas()          # (the parameters' storage moves into the flat blocks before Adam sees them)
            self.alpha_optim = torch.optim.Adam(list(net.alpha_prob_parameters()), alpha_lr, betas=tuple(alpha_betas),
                                                weight_decay=alpha_weight_decay)
        self.alpha_every = alpha_every
        self.arch_mode = arch_mode
        self.steps = 0

    def begin_epoch(self, epoch=None):
        """The top of the scripts' epoch loop (search_vqa.py:261-265): 'sgd' steps the cosine schedule -- before the epoch's
        weight steps; 'wadam' has nothing to do here (its decay() at the epochs of NET_LR_DECAY_LIST stays the caller's).
        `epoch` (0-based, the scripts' loop variable) is checked against the schedule's own count when given: the schedule
        moves by one per call, so an epoch skipped or begun twice is an error, not a silently shifted rate."""
        if self.lr_scheduler is None:
            return
        if epoch is not None and epoch + self._epoch_shift != self.lr_scheduler.last_epoch:
            raise ValueError('begin_epoch(%d): the cosine schedule stands before epoch %d (start_epoch plus the epochs begun so '
                             'far)' % (epoch, self.lr_scheduler.last_epoch - self._epoch_shift))
        self.lr_scheduler.step()

    def _net_step(self):
        # whatever `self.net_optim` is NOW (a caller may replace it): a bare FlatSGD takes the clip with every step, the
        # WarmupOptimizer carries its own
        if isinstance(self.net_optim, FlatSGD):
            self.net_optim.step(max_norm=self._max_norm)
        else:
            self.net_optim.step()

    def _sample(self, plan):
        if plan is None:
            self.net.reset_binary_gates()
        else:            # injected (active, inactive) lists per node: tests / replay of a logged search
            self.net.set_sampled(plan)
            if not getattr(self.net, 'keep_candidate_grads', False):
                for m in self.net.redundant_modules:
                    m.clear_candidate_grads()

    def weight_step(self, inputs, target, optimize=True, plan=None):
        net, red = self.net, self.reducer
        MixedOp.MODE = None
        self._sample(plan)
        red.begin_weight_step()
        loss = self.loss_fn(net(inputs), target)
        loss.backward()
        red.finish_weight_step()
        if optimize:
            self._net_step()
        self.steps += 1
        return loss

    def _reinforce_arch_step(self, inputs, target, optimize, plan):
        reward = self.reward
        if reward is None:      # the loop's own loss per sample of the batch, negated
            reward = NegLossReward(self.loss_fn, 1.0 / max(int(target.shape[0]), 1))
        return reinforce_arch_step(self.net, self.alpha_optim, reward, inputs, target, reducer=self.reducer, optimize=optimize,
                                   plan=plan)

    def arch_step(self, inputs, target, optimize=True, plan=None):
        if self.arch_mode == 'reinforce':
            return self._reinforce_arch_step(inputs, target, optimize, plan)
        net, red = self.net, self.reducer
        MixedOp.MODE = self.arch_mode
        try:
            self._sample(plan)
            net.begin_arch_step()
            # the network weights take no update here (search_vqa.py:331 steps alpha_optim only); their gradients are
            # produced -- as in the reference -- into the flat buffer, which the next weight step zeroes
            red.fg.zero()
            red.fg.attach()
            loss = self.loss_fn(net(inputs), target)
            loss.backward()
            red.reduce_alpha_gate_grads()
            if self.arch_mode == 'two' and not self.fused_arch_update:
                for m in net.redundant_modules:      # (the script's net.zero_grad() before backward, search_vqa.py:328)
                    m.alpha_prob.grad = None
                net.set_arch_param_grad()
                if optimize:
                    self.alpha_optim.step()
                    net.rescale_updated_arch_param()
            elif optimize:
                self.alpha_optim.step()
        finally:
            MixedOp.MODE = None
        return loss

    def bilevel_round(self, train_batches, eval_batch):
        """ALPHA_EVERY weight steps on training batches, then one arch step on a held-out batch
        (search_vqa.py:149-150,303-305).  Returns the list of losses (device tensors)."""
        out = [self.weight_step(inp, tgt) for inp, tgt in train_batches]
        out.append(self.arch_step(*eval_batch))
        return out
