"""The architecture-parameter updates of the search over the [rows, width] alpha block, one launch each (csrc/alpha.hip):
'full' mode, 'two' mode, both with the expected-cost term, and REINFORCE.  CUDA float32 tensors take the kernels; CPU tensors
the same arithmetic in torch.  mmnas_amd.ops re-exports the public names."""
import ctypes as C
import math

import torch

from . import _lib as L

ALPHA_TWO_MAX_ROWS = 128              # mmnas_alpha_two_step carries the pairs in its kernel arguments
COST_FORMS = ('linear', 'log')        # cost_form of mmnas_alpha_*_step_cost: 0, 1
REWARD_FORMS = ('mul', 'add')         # reward_form of mmnas_alpha_reinforce_step: 0, 1
ALPHA_REINFORCE_MAX_CHOICES = 3072    # M * rows: the sampled indices travel in the kernel arguments, one byte each
ALPHA_REINFORCE_MAX_SAMPLES = 256


def _check_step(who, step, width=None, min_width=1):
    if int(step) < 1:
        raise ValueError('%s: step counts from 1, got %r' % (who, step))
    if width is not None and width < min_width:
        raise ValueError('%s: width %d' % (who, width))


def _check_pairs(who, pairs, rows, width, with_pairs=''):
    """-> one (active, inactive) tuple of two different columns per row."""
    pairs = [(int(p[0]), int(p[1])) for p in pairs]
    if len(pairs) != rows:
        raise ValueError('%s: %d pairs for %d rows' % (who, len(pairs), rows))
    if rows > ALPHA_TWO_MAX_ROWS:
        raise ValueError('%s: %d rows%s, at most %d' % (who, rows, with_pairs, ALPHA_TWO_MAX_ROWS))
    for r, (i, j) in enumerate(pairs):
        if not (0 <= i < width and 0 <= j < width) or i == j:
            raise ValueError('%s: row %d: pair (%d, %d) must be two different columns of 0..%d' % (who, r, i, j, width - 1))
    return pairs


def _check_cost_scalars(who, cost_ref, cost_weight, any_sign=False):
    """-> (cost_ref, cost_weight) as floats; any_sign: REINFORCE's weight may be negative."""
    cost_ref, cost_weight = float(cost_ref), float(cost_weight)
    if not (math.isfinite(cost_ref) and cost_ref > 0):
        raise ValueError('%s: cost_ref must be finite and positive, got %r' % (who, cost_ref))
    if not (math.isfinite(cost_weight) and (any_sign or cost_weight >= 0)):
        raise ValueError('%s: cost_weight must be finite%s, got %r' % (who, '' if any_sign else ' and not negative', cost_weight))
    return cost_ref, cost_weight


def _check_block(prob, others, message, dtype=False, missing=False):
    """Every tensor of `others` (None: absent) has the shape and device (dtype: and the dtype) of prob."""
    if missing or any(t is not None and (t.shape != prob.shape or t.device != prob.device or (dtype and t.dtype != prob.dtype))
                      for t in others):
        raise ValueError(message)


def _pair_index(who, prob, pairs):
    idx = torch.tensor(pairs, dtype=torch.int64, device=prob.device)
    if bool(torch.isinf(prob.gather(1, idx)).any()):      # (host tensors: the logits are at hand)
        raise ValueError('%s: a pair names a padding column' % who)
    return idx


def _adam_tail_torch(prob, m, v, grad, lr, betas, eps, step, weight_decay):
    """torch Adam over the live columns of the block, in place, in the tensors' own dtype: the kernels' element update."""
    b1, b2 = float(betas[0]), float(betas[1])
    c1 = 1.0 - b1 ** step
    c2s = math.sqrt(1.0 - b2 ** step)
    valid = prob > float('-inf')                      # padding columns: logit, m and v stay as they are
    if weight_decay:
        grad = grad + weight_decay * torch.where(valid, prob, torch.zeros_like(prob))
    mi = b1 * m + (1.0 - b1) * grad
    vi = b2 * v + (1.0 - b2) * grad * grad
    m.copy_(torch.where(valid, mi, m))
    v.copy_(torch.where(valid, vi, v))
    prob.copy_(torch.where(valid, prob - (lr / c1) * mi / (vi.sqrt() / c2s + eps), prob))


def alpha_full_step(prob, gate_grad, m, v, prob_grad, lr, betas, eps, step, weight_decay=0.0):
    """All nodes' architecture update in one launch (mmnas_alpha_full_step): prob/gate_grad/m/v [nodes, width].
    weight_decay != 0: torch Adam's decay folded into the same launch (mmnas_alpha_full_step_wd)."""
    ptrs = [L.fptr(t) for t in (prob, gate_grad, m, v, prob_grad)]
    hyper = (prob.shape[0], prob.shape[1], float(lr), float(betas[0]), float(betas[1]), float(eps))
    if weight_decay:
        L.check(L.lib().mmnas_alpha_full_step_wd(*ptrs, *hyper, float(weight_decay), int(step), L.stream()))
        return
    L.check(L.lib().mmnas_alpha_full_step(*ptrs, *hyper, int(step), L.stream()))


def alpha_two_pair_grad(prob, gate_grad, idx):
    """set_arch_param_grad of ALPHA_BINARY_MODE 'two' (mixed.py:179-186) for all rows at once, in torch: prob / gate_grad
    [rows, width], idx [rows, 2] int64 (active, inactive).  Returns the [rows, width] gradient, zero outside the pairs."""
    a = prob.gather(1, idx)
    p = torch.softmax(a, dim=1)                       # over the pair only
    gp = gate_grad.gather(1, idx) * p
    return torch.zeros_like(prob).scatter_(1, idx, gp - p * gp.sum(dim=1, keepdim=True))


def alpha_two_rescale(prob, old_pair, idx):
    """rescale_updated_arch_param (mixed.py:200-208) for all rows at once, in place: `old_pair` [rows, 2] are the pairs'
    logits before the optimizer step.  The offset is formed in float64, as the reference's math.log / math.exp do."""
    new = prob.gather(1, idx)
    off = torch.logsumexp(new.double(), dim=1, keepdim=True) - torch.logsumexp(old_pair.double(), dim=1, keepdim=True)
    prob.scatter_(1, idx, (new.double() - off).to(prob.dtype))
    return prob


def _alpha_two_step_torch(prob, gate_grad, m, v, prob_grad, idx, lr, betas, eps, step, weight_decay):
    """mmnas_alpha_two_step's arithmetic, statement for statement, in the tensors' own dtype."""
    old = prob.gather(1, idx)
    grad = alpha_two_pair_grad(prob, gate_grad, idx)
    if prob_grad is not None:
        prob_grad.copy_(grad)
    _adam_tail_torch(prob, m, v, grad, lr, betas, eps, step, weight_decay)
    alpha_two_rescale(prob, old, idx)


def alpha_two_step(prob, gate_grad, m, v, prob_grad, pairs, lr, betas, eps, step, weight_decay=0.0):
    """All nodes' architecture update of ALPHA_BINARY_MODE 'two' (mixed.py:179-208, search_vqa.py:330-335) in one launch
    (mmnas_alpha_two_step): the gradient over each node's sampled pair, torch Adam over the node's row, the pair's rescale.
    prob / gate_grad / m / v [nodes, width] (padding columns of prob hold -inf), prob_grad the same or None, `pairs` one
    (active, inactive) column pair per node (a host sequence: it travels in the kernel arguments, nothing is copied).
    CUDA float32 tensors take the kernel; CPU tensors the same arithmetic in torch."""
    rows, width = prob.shape
    who = 'alpha_two_step'
    _check_step(who, step)
    pairs = _check_pairs(who, pairs, rows, width)
    _check_block(prob, (gate_grad, m, v, prob_grad),
                 'alpha_two_step: prob, gate_grad, m, v and prob_grad share one [rows, width] shape and one device')
    if rows == 0:
        return
    if prob.is_cuda:
        arr = (C.c_int * (2 * rows))(*[c for p in pairs for c in p])
        L.check(L.lib().mmnas_alpha_two_step(L.fptr(prob), L.fptr(gate_grad), L.fptr(m), L.fptr(v), L.fptr(prob_grad), rows, width,
                                             arr, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                             int(step), L.stream()))
        return
    idx = _pair_index(who, prob, pairs)
    with torch.no_grad():
        _alpha_two_step_torch(prob, gate_grad, m, v, prob_grad, idx, float(lr), betas, float(eps), int(step), float(weight_decay))


def alpha_expected_cost(prob, cost, cost_weight, cost_ref, cost_form):
    """The expected-cost term of a hardware-aware search over the [rows, width] alpha block (padding columns -inf in prob,
    0 in cost): p = softmax(prob) per row, E_r = sum_j p_j cost[r, j], E = sum_r E_r and
      'linear': R = cost_weight * (E - cost_ref) / cost_ref, k = cost_weight / cost_ref
      'log':    R = cost_weight * log(E / cost_ref),          k = cost_weight / E      (E <= 0: both 0)
    Returns (p, E_r, E, R, k); dR/dprob = k * p * (cost - E_r).  Tensors throughout: nothing is read back."""
    p = torch.softmax(prob, dim=1)
    er = (p * cost).sum(dim=1)
    E = er.sum()
    if cost_form == 'linear':
        return p, er, E, cost_weight * (E - cost_ref) / cost_ref, torch.full_like(E, cost_weight / cost_ref)
    pos = E > 0
    safe = torch.where(pos, E, torch.ones_like(E))
    zero = torch.zeros_like(E)
    return p, er, E, torch.where(pos, cost_weight * torch.log(safe / cost_ref), zero), torch.where(pos, cost_weight / safe, zero)


def _alpha_cost_step_torch(prob, gate_grad, m, v, prob_grad, cost, idx, lr, betas, eps, step, weight_decay, cost_weight, cost_ref,
                           cost_form, stats):
    """mmnas_alpha_full_step_cost (idx None) / mmnas_alpha_two_step_cost (idx [rows, 2]), statement for statement, in the
    tensors' own dtype."""
    p, er, E, R, k = alpha_expected_cost(prob, cost, cost_weight, cost_ref, cost_form)      # from the alphas before the update
    if idx is None:
        grad = p * (gate_grad - (gate_grad * p).sum(dim=1, keepdim=True))                   # 'full': mixed.py:194-198
    else:
        old = prob.gather(1, idx)
        grad = alpha_two_pair_grad(prob, gate_grad, idx)
    grad = grad + k * p * (cost - er.unsqueeze(1))
    if prob_grad is not None:
        prob_grad.copy_(grad)
    if stats is not None:
        stats[:-2].copy_(er)
        stats[-2].copy_(E)
        stats[-1].copy_(R)
    _adam_tail_torch(prob, m, v, grad, lr, betas, eps, step, weight_decay)
    if idx is not None:
        alpha_two_rescale(prob, old, idx)


def alpha_cost_step(prob, gate_grad, m, v, prob_grad, cost, lr, betas, eps, step, weight_decay=0.0, cost_weight=0.0, cost_ref=1.0,
                    cost_form='linear', pairs=None, stats=None):
    """The architecture update with the expected-cost regulariser R of alpha_expected_cost() in the objective, one launch
    (mmnas_alpha_full_step_cost; with `pairs`, one (active, inactive) column pair per node as in alpha_two_step,
    mmnas_alpha_two_step_cost).  The cost gradient k p_j (cost_j - E_r), p the softmax over the whole row, reaches every live
    column in both modes; in 'two' mode the task gradient stays the one over the sampled pair and the pair is rescaled after
    Adam as in alpha_two_step.  prob_grad (or None) receives task part + cost part; `stats` (or None; rows + 2) E_r per row,
    E, R -- all from the alphas before the update.  cost [rows, width]: 0 in the padding columns.
    CUDA float32 tensors take the kernels; CPU tensors of any float dtype the same arithmetic in torch."""
    rows, width = prob.shape
    who = 'alpha_cost_step'
    if cost_form not in COST_FORMS:
        raise ValueError("%s: cost_form is 'linear' or 'log', got %r" % (who, cost_form))
    cost_ref, cost_weight = _check_cost_scalars(who, cost_ref, cost_weight)
    _check_step(who, step, width, 1 if pairs is None else 2)
    if pairs is not None:
        pairs = _check_pairs(who, pairs, rows, width, ' with pairs')
    _check_block(prob, (gate_grad, m, v, prob_grad, cost), missing=cost is None,
                 message='%s: prob, gate_grad, m, v, prob_grad and cost share one [rows, width] shape and one device' % who)
    if stats is not None and (tuple(stats.shape) != (rows + 2,) or stats.device != prob.device):
        raise ValueError('%s: stats holds rows + 2 = %d values on the device of prob' % (who, rows + 2))
    form = COST_FORMS.index(cost_form)
    if prob.is_cuda and rows:
        hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), cost_weight, cost_ref, form, int(step),
                 L.stream())
        ptrs = [L.fptr(t) for t in (prob, gate_grad, m, v, prob_grad, cost, stats)]
        if pairs is None:
            L.check(L.lib().mmnas_alpha_full_step_cost(*ptrs, rows, width, *hyper))
        else:
            arr = (C.c_int * (2 * rows))(*[c for p in pairs for c in p])
            L.check(L.lib().mmnas_alpha_two_step_cost(*ptrs, rows, width, arr, *hyper))
        return
    idx = _pair_index(who, prob, pairs) if pairs is not None and rows else None
    with torch.no_grad():      # (also a device block without rows: nothing to launch over, E = 0)
        _alpha_cost_step_torch(prob, gate_grad, m, v, prob_grad, cost, idx, float(lr), betas, float(eps), int(step),
                               float(weight_decay), cost_weight, cost_ref, cost_form, stats)


def alpha_reinforce_rewards(quality, choice, cost, cost_weight, cost_ref, reward_form):
    """R_i of M sampled architectures: quality [M], choice [M, rows] int64, cost [rows, width] or None.
      C_i = sum_r cost[r, a_ir];  'mul': R_i = Q_i (C_i / cost_ref)^w;  'add': R_i = Q_i + w log(C_i / cost_ref)
    (C_i <= 0: R_i = Q_i; no table or w == 0: R_i = Q_i).  C_i and the cost factor are formed in float64 and R_i is rounded
    once to the dtype of quality, as the kernel does.  Tensors throughout: nothing is read back."""
    if cost is None or cost_weight == 0:
        return quality.clone()
    C = cost.double().gather(1, choice.t()).sum(dim=0)
    pos = C > 0
    ratio = torch.where(pos, C, torch.full_like(C, cost_ref)) / cost_ref
    if reward_form == 'mul':
        return (quality.double() * ratio.pow(cost_weight)).to(quality.dtype)
    return (quality.double() + cost_weight * ratio.log()).to(quality.dtype)


def _alpha_reinforce_step_torch(prob, m, v, prob_grad, choice, quality, baseline, lr, betas, eps, step, weight_decay, cost,
                                cost_weight, cost_ref, reward_form, baseline_decay, stats, err):
    """mmnas_alpha_reinforce_step, statement for statement, in the tensors' own dtype; Rbar, A_i, sum_i A_i and the sums of A
    over the samples that chose a column are formed in float64 from the rewards and g is rounded once, as the kernel does."""
    M = choice.shape[0]
    R = alpha_reinforce_rewards(quality, choice, cost, cost_weight, cost_ref, reward_form)
    if not bool(torch.isfinite(quality).all() & torch.isfinite(R).all()):     # (host tensors: the values are at hand)
        err.fill_(1)
        return
    rbar = R.double().sum() / M
    init = bool(baseline[1] != 0)
    b = baseline[0].double() if init else rbar
    A64 = R.double() - b
    sum_a = torch.zeros((), dtype=torch.float64)
    p = torch.softmax(prob, dim=1)                                             # alphas before the update
    hit = torch.zeros(prob.shape, dtype=torch.float64)
    for i in range(M):                                                         # samples ascending, as the kernel adds them
        sum_a = sum_a + A64[i]
        hit.scatter_add_(1, choice[i].unsqueeze(1), A64[i].expand(prob.shape[0], 1))
    grad = (-(hit - p.double() * sum_a) / M).to(prob.dtype)
    if prob_grad is not None:
        prob_grad.copy_(grad)
    b_new = (baseline_decay * b + (1.0 - baseline_decay) * rbar) if init else rbar
    if stats is not None:
        stats[:M].copy_(R)
        stats[M].copy_(rbar)
        stats[M + 1].copy_(b)
        stats[M + 2].copy_(b_new)
    baseline[0].copy_(b_new)
    baseline[1].fill_(1)
    _adam_tail_torch(prob, m, v, grad, lr, betas, eps, step, weight_decay)


def alpha_reinforce_step(prob, m, v, prob_grad, choice, quality, baseline, lr, betas, eps, step, weight_decay=0.0, cost=None,
                         cost_weight=0.0, cost_ref=1.0, reward_form='mul', baseline_decay=0.95, stats=None, err=None,
                         n_choices=None):
    """The REINFORCE architecture update (ProxylessNAS 3.3.2, MnasNet's reward) over the [rows, width] alpha block in one launch
    (mmnas_alpha_reinforce_step).  `choice` [M, rows]: the candidate each of M sampled architectures took per node (a host
    sequence or CPU integer tensor: it travels in the kernel arguments); `quality` [M]: their task rewards, on the device of
    prob, never read here; `baseline` [2]: (value, initialised), the moving average of the mean reward.  With R_i of
    alpha_reinforce_rewards(), Rbar = mean R, b = baseline if initialised else Rbar, A_i = R_i - b:
      g[r, j] = -(1 / M) (sum_{i: a_ir = j} A_i - p[r, j] sum_i A_i),  p = softmax(prob) per row, before the update
    then torch Adam on g + weight_decay * prob (prob_grad, or None, keeps g) and baseline <- decay * baseline + (1 - decay) * Rbar
    (the first update: Rbar).  M = 1: the first update has A = 0 and moves nothing but the moments -- the rule, not a defect.
    `stats` (or None; M + 3): R_i, Rbar, the b used, the baseline after.  `err` (one int32): set to 1, and nothing else is
    written, when a quality or reward is not finite.  cost_weight may have either sign.  `n_choices` (or None: read from the
    -inf padding of a CPU prob, `width` for a device block): live columns per row, the indices are checked against it.
    CUDA float32 tensors take the kernel; CPU tensors of any float dtype the same arithmetic in torch."""
    rows, width = prob.shape
    who = 'alpha_reinforce_step'
    if reward_form not in REWARD_FORMS:
        raise ValueError("%s: reward_form is 'mul' or 'add', got %r" % (who, reward_form))
    cost_ref, cost_weight = _check_cost_scalars(who, cost_ref, cost_weight, any_sign=True)
    baseline_decay = float(baseline_decay)
    if not 0.0 <= baseline_decay < 1.0:
        raise ValueError('%s: baseline_decay lies in [0, 1), got %r' % (who, baseline_decay))
    _check_step(who, step, width)
    ch = torch.as_tensor(choice).detach().to('cpu', torch.int64)
    if ch.dim() != 2 or ch.shape[0] < 1 or ch.shape[1] != rows:
        raise ValueError('%s: choice is [M >= 1, rows = %d], got %s' % (who, rows, tuple(ch.shape)))
    M = ch.shape[0]
    if n_choices is None:
        # (a device block is not read back: without the counts every column passes, and an index into the padding only
        #  writes prob_grad there -- padding logits and moments stay)
        n_choices = torch.full((rows,), width) if prob.is_cuda else (prob > float('-inf')).sum(dim=1)
    nc = torch.as_tensor(n_choices).detach().to('cpu', torch.int64)
    if tuple(nc.shape) != (rows,) or (rows and (int(nc.min()) < 1 or int(nc.max()) > width)):
        raise ValueError('%s: n_choices holds one count of 1..%d per row' % (who, width))
    if rows and bool(((ch < 0) | (ch >= nc.unsqueeze(0))).any()):
        raise ValueError("%s: a sampled index lies outside its row's live columns" % who)
    _check_block(prob, (m, v, prob_grad, cost), dtype=True,
                 message='%s: prob, m, v, prob_grad and cost share one [rows, width] shape, one dtype and one device' % who)
    for name, t, n in (('quality', quality, M), ('baseline', baseline, 2), ('stats', stats, M + 3)):
        if (t is None and name != 'stats') or (t is not None and (tuple(t.shape) != (n,) or t.device != prob.device or t.dtype != prob.dtype)):
            raise ValueError('%s: %s holds %d values of the dtype and on the device of prob' % (who, name, n))
    if err is None or err.numel() != 1 or err.dtype != torch.int32 or err.device != prob.device:
        raise ValueError('%s: err is one int32 on the device of prob' % who)
    if prob.is_cuda:
        if M > ALPHA_REINFORCE_MAX_SAMPLES or width > 256 or M * rows > ALPHA_REINFORCE_MAX_CHOICES:
            raise ValueError('%s: M = %d (<= %d), width = %d (<= 256), M * rows = %d (<= %d)' % (
                who, M, ALPHA_REINFORCE_MAX_SAMPLES, width, M * rows, ALPHA_REINFORCE_MAX_CHOICES))
        arr = (C.c_ubyte * max(M * rows, 1))(*ch.flatten().tolist())
        ncs = (C.c_int * max(rows, 1))(*nc.tolist())
        L.check(L.lib().mmnas_alpha_reinforce_step(L.fptr(prob), L.fptr(m), L.fptr(v), L.fptr(prob_grad), rows, width, arr, ncs, M,
                                                   L.fptr(quality), L.fptr(cost), cost_weight, cost_ref,
                                                   REWARD_FORMS.index(reward_form), L.fptr(baseline), baseline_decay, L.fptr(stats),
                                                   L.ptr(err), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                   float(weight_decay), int(step), L.stream()))
        return
    with torch.no_grad():
        _alpha_reinforce_step_torch(prob, m, v, prob_grad, ch, quality, baseline, float(lr), betas, float(eps), int(step),
                                    float(weight_decay), cost, cost_weight, cost_ref, reward_form, baseline_decay, stats, err)
