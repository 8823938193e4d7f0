"""The grounding (train_vgd) and retrieval (train_itm) training losses as one HIP launch per direction.

* VgdLoss / vgd_loss_fused -- harness.vgd_loss (train_vgd.py:320-334, REDUCTION 'sum'): KLDiv or BCE-with-logits on the region
  scores + LOSS_LAMBDA * SmoothL1 on the masked box targets, each over its LOSS_AVG denominator.
* TripletBCELoss / TripletMarginLoss -- harness.BCE_Loss / utils.itm_loss.Margin_Loss (mmnas/utils/itm_loss.py) over the three
  score vectors of harness.itm_triplet_step, without label tensors.
* fused(loss_fn) -- the HIP form of a BCE_Loss / Margin_Loss instance; anything else is returned as it is.

float32 CUDA tensors run csrc/losses.hip: the forward launch (one workgroup, float64 sums, no atomics -- the same inputs give the
same bits on every call) writes the loss and, when a prediction requires a gradient, every gradient for an upstream gradient of
1; the backward launch multiplies them by the upstream scalar, which stays on the device.  Nothing synchronises with the host.
Gradients flow to the predictions only.  The gradients live in the autograd graph like any saved tensor: a second backward()
needs retain_graph=True on the first, otherwise torch raises its usual "backward through the graph a second time" error.

CPU tensors, other dtypes and mask shapes outside the ones below run the torch composition itself (harness.vgd_loss,
harness.BCE_Loss, Margin_Loss).

Numerics: the kernels sum in float64 and round once, so they sit closer to the reference run in float64 than the float32 torch
composition does; against the composition they differ by float32 round-off of its sums.
"""
import torch
import torch.nn as nn

from . import _lib as L
from . import harness
from .utils.itm_loss import Margin_Loss

__all__ = ['VgdLoss', 'vgd_loss_fused', 'TripletBCELoss', 'TripletMarginLoss', 'fused']

_MODES = {'kld': 0, 'bce': 1}
_TARGET_KEYS = ('scores', 'scores_mask', 'bbox', 'bbox_mask')


def _aligned(t):
    """Contiguous with a 16-byte aligned base (the kernel reads the box tensors as float4)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _scale_grads(saved, go):
    go = go.to(torch.float32).contiguous()
    out = torch.empty_like(saved)
    with torch.cuda.device(saved.device):
        L.check(L.lib().mmnas_loss_grad_scale(L.fptr(saved), L.fptr(go), L.fptr(out), saved.numel(), L.stream()))
    return out


# ---- VGD -----------------------------------------------------------------------------------------------------------------------
def _vgd_launch(ps, pr, sc, sm, bb, bm, lam, mode, loss_avg, batch_size, want_grad):
    B, S = ps.shape
    dev = ps.device
    ps, sc, sm = ps.contiguous(), sc.contiguous(), sm.contiguous()
    pr, bb, bm = _aligned(pr), _aligned(bb), _aligned(bm)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    parts = torch.empty(4, dtype=torch.float32, device=dev)
    grads = torch.empty(5 * B * S, dtype=torch.float32, device=dev) if want_grad else None   # d pred_reg (float4 rows), then d pred_scores
    n = B * S
    with torch.cuda.device(dev):
        L.check(L.lib().mmnas_vgd_loss_fwd(L.fptr(ps), L.fptr(pr), L.fptr(sc), L.fptr(bb), L.fptr(sm), L.fptr(bm), B, S,
                                           int(sm.shape[1] == S), int(bm.shape[2] == 4), mode, int(bool(loss_avg)),
                                           float(batch_size), float(lam), L.fptr(loss), L.fptr(parts),
                                           None if grads is None else grads.data_ptr() + 16 * n,
                                           None if grads is None else grads.data_ptr(), L.stream()))
    return loss, parts, grads


class _VgdLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ps, pr, sc, sm, bb, bm, lam, mode, loss_avg, batch_size):
        loss, parts, grads = _vgd_launch(ps, pr, sc, sm, bb, bm, lam, mode, loss_avg, batch_size, True)
        ctx.save_for_backward(grads)
        ctx.shape = tuple(ps.shape)
        ctx.mark_non_differentiable(parts)
        return loss, parts

    @staticmethod
    def backward(ctx, go, _):
        grads, = ctx.saved_tensors
        B, S = ctx.shape
        g = _scale_grads(grads, go)
        return (g[4 * B * S:].view(B, S), g[:4 * B * S].view(B, S, 4)) + (None,) * 8


def _bad(name, t, want):
    return ValueError('%s must have shape %s, got %s' % (name, want, tuple(t.shape)))


def _broadcasts(shape, onto):
    if len(shape) > len(onto):
        return False
    return all(a == 1 or a == b for a, b in zip(reversed(shape), reversed(onto)))


def _vgd_check(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask):
    """ValueError for shapes the loss cannot mean; True when the masks have one of the layouts the kernel reads."""
    for name, t in (('pred_scores', pred_scores), ('pred_reg', pred_reg), ('scores', scores), ('scores_mask', scores_mask),
                    ('bbox', bbox), ('bbox_mask', bbox_mask)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s must be a torch.Tensor, got %s' % (name, type(t).__name__))
    if pred_scores.dim() != 2:
        raise _bad('pred_scores', pred_scores, '[B, S]')
    B, S = pred_scores.shape
    if tuple(pred_reg.shape) != (B, S, 4):
        raise _bad('pred_reg', pred_reg, (B, S, 4))
    if tuple(scores.shape) != (B, S):
        raise _bad('scores', scores, (B, S))
    if tuple(bbox.shape) != (B, S, 4):
        raise _bad('bbox', bbox, (B, S, 4))
    if not _broadcasts(tuple(scores_mask.shape), (B, S)):
        raise _bad('scores_mask', scores_mask, '%s or %s' % ((B, S), (B, 1)))
    if not _broadcasts(tuple(bbox_mask.shape), (B, S, 4)):
        raise _bad('bbox_mask', bbox_mask, '%s or %s' % ((B, S, 4), (B, S, 1)))
    return tuple(scores_mask.shape) in ((B, S), (B, 1)) and tuple(bbox_mask.shape) in ((B, S, 4), (B, S, 1))


def _vgd(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask, lam, scores_loss, loss_avg, batch_size):
    """(loss, parts); parts is None on the torch path."""
    kernel_layout = _vgd_check(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask)
    if scores_loss not in _MODES:
        raise ValueError("scores_loss must be 'kld' or 'bce', got %r" % (scores_loss,))
    ts = (pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask)
    dev = pred_scores.device
    if not (kernel_layout and pred_scores.numel() and all(t.is_cuda and t.device == dev and t.dtype == torch.float32 for t in ts)):
        return harness.vgd_loss(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask, lam=lam, scores_loss=scores_loss,
                                loss_avg=loss_avg, batch_size=batch_size), None
    if batch_size is None:
        batch_size = pred_scores.shape[0]
    args = (scores.detach(), scores_mask.detach(), bbox.detach(), bbox_mask.detach(), lam, _MODES[scores_loss], loss_avg, batch_size)
    if torch.is_grad_enabled() and (pred_scores.requires_grad or pred_reg.requires_grad):
        return _VgdLossFn.apply(pred_scores, pred_reg, *args)
    return _vgd_launch(pred_scores.detach(), pred_reg.detach(), *args, False)[:2]


def vgd_loss_fused(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask, lam=0.5, scores_loss='kld', loss_avg=True,
                   batch_size=None):
    """harness.vgd_loss with its signature, as one launch per direction for float32 CUDA tensors.

    pred_scores, scores [B,S]; pred_reg, bbox [B,S,4]; scores_mask [B,S] or [B,1]; bbox_mask [B,S,4] or [B,S,1] (what
    grounding_targets returns, and the full shapes of the loader).  LOSS_AVG divides by the sum of each mask tensor as given (the
    number of supervised samples for a [B,1] scores_mask), in 'bce' mode the score term by batch_size (default: B).  An all-zero
    mask gives the reference's own 0 / 0 = NaN; it is not special-cased."""
    return _vgd(pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask, lam, scores_loss, loss_avg, batch_size)[0]


class VgdLoss(nn.Module):
    """The loss of train_vgd.py:320-334 as a module: forward((pred_scores, pred_reg), targets), targets the dict
    grounding_targets returns or the 4-tuple (scores, scores_mask, bbox, bbox_mask) -- so
    TrainLoop(net, loss_fn=VgdLoss(cfg)).step(inputs, grounding_targets(...)) is a VGD training step.  cfg supplies LOSS_LAMBDA,
    SCORES_LOSS, LOSS_AVG and BATCH_SIZE where it has them.

    After a call on the kernel path `.parts` is a float32 device vector (score term, box term, sum of scores_mask, sum of
    bbox_mask), the terms as they enter the loss -- for logging without a host synchronisation; None after a call that took
    the torch composition.  An all-zero mask gives NaN, as the reference's 0 / 0 does."""

    def __init__(self, cfg=None, lam=0.5, scores_loss='kld', loss_avg=True, batch_size=None):
        super().__init__()
        self.lam = float(getattr(cfg, 'LOSS_LAMBDA', lam))
        self.scores_loss = getattr(cfg, 'SCORES_LOSS', scores_loss)
        self.loss_avg = bool(getattr(cfg, 'LOSS_AVG', loss_avg))
        self.batch_size = getattr(cfg, 'BATCH_SIZE', batch_size)
        if self.scores_loss not in _MODES:
            raise ValueError("SCORES_LOSS must be 'kld' or 'bce', got %r" % (self.scores_loss,))
        self.parts = None

    def forward(self, pred, targets):
        if not isinstance(pred, (tuple, list)) or len(pred) != 2:
            raise ValueError('pred must be the pair (pred_scores, pred_reg)')
        if isinstance(targets, dict):
            missing = [k for k in _TARGET_KEYS if k not in targets]
            if missing:
                raise ValueError('targets lacks %s' % ', '.join(missing))
            targets = tuple(targets[k] for k in _TARGET_KEYS)
        elif not isinstance(targets, (tuple, list)) or len(targets) != 4:
            raise ValueError('targets must be a dict or the 4-tuple (%s)' % ', '.join(_TARGET_KEYS))
        loss, self.parts = _vgd(pred[0], pred[1], *targets, self.lam, self.scores_loss, self.loss_avg, self.batch_size)
        return loss


# ---- ITM -----------------------------------------------------------------------------------------------------------------------
def _triplet_launch(sp, sc, si, mode, margin, mean, want_grad):
    n = sp.numel()
    loss = torch.empty((), dtype=torch.float32, device=sp.device)
    grads = torch.empty(3, n, dtype=torch.float32, device=sp.device) if want_grad else None
    with torch.cuda.device(sp.device):
        L.check(L.lib().mmnas_itm_triplet_loss_fwd(L.fptr(sp.contiguous()), L.fptr(sc.contiguous()), L.fptr(si.contiguous()), n, mode,
                                                   float(margin), int(mean), L.fptr(loss), L.fptr(grads), L.stream()))
    return loss, grads


class _TripletLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sp, sc, si, mode, margin, mean):
        loss, grads = _triplet_launch(sp, sc, si, mode, margin, mean, True)
        ctx.save_for_backward(grads)
        ctx.shape = tuple(sp.shape)
        return loss

    @staticmethod
    def backward(ctx, go):
        grads, = ctx.saved_tensors
        g = _scale_grads(grads, go)
        return g[0].view(ctx.shape), g[1].view(ctx.shape), g[2].view(ctx.shape), None, None, None


def _triplet_kernel_path(scores_pos, scores_negc, scores_negi):
    """ValueError when the three shapes differ; True when the kernel takes these tensors."""
    for name, t in (('scores_negc', scores_negc), ('scores_negi', scores_negi)):
        if tuple(t.shape) != tuple(scores_pos.shape):
            raise ValueError('%s must have scores_pos\' shape %s, got %s' % (name, tuple(scores_pos.shape), tuple(t.shape)))
    ts = (scores_pos, scores_negc, scores_negi)
    return all(t.is_cuda and t.device == scores_pos.device and t.dtype == torch.float32 for t in ts)


def _triplet(sp, sc, si, mode, margin, mean):
    if torch.is_grad_enabled() and any(t.requires_grad for t in (sp, sc, si)):
        return _TripletLossFn.apply(sp, sc, si, mode, margin, mean)
    return _triplet_launch(sp.detach(), sc.detach(), si.detach(), mode, margin, mean, False)[0]


class TripletBCELoss(nn.Module):
    """harness.BCE_Loss (mmnas/utils/itm_loss.py:4-24) as one launch per direction: BCE on probabilities with the labels
    1 / 0 / 0, the positive term twice, log clamped at -100 and the backward's denominator at 1e-12 as torch.nn.BCELoss does;
    reduction 'sum' or 'mean' (cfg.REDUCTION).  Scores outside [0, 1] give NaN where torch raises."""

    def __init__(self, cfg=None):
        super().__init__()
        self.reduction = getattr(cfg, 'REDUCTION', 'sum') if cfg is not None else 'sum'

    def forward(self, scores_pos, scores_negc, scores_negi):
        if _triplet_kernel_path(scores_pos, scores_negc, scores_negi) and self.reduction in ('sum', 'mean'):
            return _triplet(scores_pos, scores_negc, scores_negi, 0, 0.0, self.reduction == 'mean')
        ref = harness.BCE_Loss()
        ref.reduction = self.reduction
        return ref(scores_pos, scores_negc, scores_negi)


class TripletMarginLoss(nn.Module):
    """utils.itm_loss.Margin_Loss (mmnas/utils/itm_loss.py:27-37) as one launch per direction: the hinge
    sum(max(0, 0.2 + s_negc - s_pos)) + sum(max(0, 0.2 + s_negi - s_pos))."""

    def __init__(self, cfg=None):
        super().__init__()
        self.margin = 0.2

    def forward(self, scores_pos, scores_negc, scores_negi):
        if _triplet_kernel_path(scores_pos, scores_negc, scores_negi):
            return _triplet(scores_pos, scores_negc, scores_negi, 1, self.margin, False)
        ref = Margin_Loss()
        ref.margin = self.margin
        return ref(scores_pos, scores_negc, scores_negi)


def fused(loss_fn):
    """The HIP form of an ITM loss module: harness.BCE_Loss -> TripletBCELoss (with its reduction), Margin_Loss ->
    TripletMarginLoss (with its margin); anything else comes back unchanged."""
    if isinstance(loss_fn, harness.BCE_Loss):
        out = TripletBCELoss()
        out.reduction = loss_fn.reduction
        return out
    if isinstance(loss_fn, Margin_Loss):
        out = TripletMarginLoss()
        out.margin = loss_fn.margin
        return out
    return loss_fn
