"""Visual grounding (configs[3], train_vgd) training targets and IoU accuracy, on the device.

* grounding_targets -- the loader's per-sample proc_bbox_label (load_data_vgd.py:228-282 with bbox_transform.py:10-27 and
  overlaps.py) for a whole batch: soft (kld) or stepped (bce) region scores, the score and box masks and the regression targets,
  in the shapes harness.vgd_loss takes.
* ground_batch -- one evaluation batch of train_vgd.py:436-453: per sample the argmax region, its decoded box
  (bbox_transform_inv), clipped to the image, its IoU with the ground truth and hit = IoU >= OVERLAP_THRESHOLD.
* GroundingEvaluator -- the whole evaluation of train_vgd.py:387-478: network forward in eval mode with proj_reg rescaled for
  BBOX_NORM, ground_batch, (hits, count) accumulated on the device, all-reduced by compute().

CUDA tensors run the HIP kernels of csrc/grounding.hip (mmnas_vgd_targets / mmnas_vgd_ground); CPU tensors run a numpy
restatement of the same arithmetic (the kernels are checked against it).

Tie rule: the argmax takes the lowest index among equal scores (np.argmax), and padded region rows are candidates, as in the
reference.

Numerics: IoU is computed in float64 in overlaps.py's order, the regression targets with the proposal side in float32 and the
rest in float64, rounded to float32 once; kld scores divide by numpy's float32 pairwise sum.  These match the reference's host
bit for bit or within 1 ulp.  The decoded box goes through a float32 exp, whose last bits differ between math libraries (numpy's
SIMD exp is off the correctly rounded result by up to 2 ulp): boxes agree with the reference host to a few ulp, and a sample
whose IoU lies within that of the threshold can count differently.
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib as L

__all__ = ['GroundingEvaluator', 'grounding_targets', 'ground_batch', 'GroundingError']

MAX_REGIONS = 1024
ERR_NONFINITE, ERR_NOBJ = 1, 2
_MODES = {'kld': 0, 'bce': 1}


class GroundingError(ValueError):
    """Invalid values found in the inputs (a NaN / infinite coordinate, score or delta; nobj outside 1..S)."""


def _raise_flag(flag, what):
    msgs = []
    if flag & ERR_NONFINITE:
        msgs.append('a NaN or infinite input')
    if flag & ERR_NOBJ:
        msgs.append('nobj outside 1..S')
    if msgs:
        raise GroundingError('%s: %s' % (what, ' and '.join(msgs)))


def _cfg_norm(cfg):
    if not getattr(cfg, 'BBOX_NORM', False):
        return None
    mean = np.asarray(cfg.BBOX_NORM_MEANS, dtype=np.float64).reshape(-1)
    std = np.asarray(cfg.BBOX_NORM_STDS, dtype=np.float64).reshape(-1)
    if mean.shape != (4,) or std.shape != (4,):
        raise ValueError('BBOX_NORM_MEANS / BBOX_NORM_STDS must hold 4 values each')
    return mean, std


def _require(t, name, shape, dtypes):
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if t.dtype not in dtypes:
        raise TypeError('%s must be %s, got %s' % (name, ' or '.join(str(d) for d in dtypes), t.dtype))
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError('%s must have shape %s, got %s' % (name, tuple('*' if s is None else s for s in shape), tuple(t.shape)))


_INT = (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8)


# ---- numpy restatement (CPU tensors) -------------------------------------------------------------------------------------------
def _iou_np(b, q):
    """overlaps.py bbox_overlaps, vectorised: b [N,4] float64 against one query q [4] float64 (same operations, same order)."""
    box_area = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
    iw = np.where(q[2] < b[:, 2], q[2], b[:, 2]) - np.where(q[0] > b[:, 0], q[0], b[:, 0]) + 1
    ih = np.where(q[3] < b[:, 3], q[3], b[:, 3]) - np.where(q[1] > b[:, 1], q[1], b[:, 1]) + 1
    with np.errstate(divide='ignore', invalid='ignore'):
        ua = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1) + box_area - iw * ih
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, 0.0)


def _targets_np(bbox, nobj, gt, thr, mode, norm):
    B, S = bbox.shape[:2]
    f32 = np.float32
    scores = np.zeros((B, S), f32)
    smask = np.zeros((B, 1), f32)
    trans = np.zeros((B, S, 4), f32)
    bmask = np.zeros((B, S, 1), f32)
    for b in range(B):
        n = int(nobj[b])
        p, q = bbox[b, :n], gt[b]
        ov = _iou_np(p.astype(np.float64), q)
        if ov.max() >= thr:
            smask[b, 0] = 1
            sel = ov >= thr
            s = np.zeros(S, f32)
            if mode == 'kld':
                s[:n][sel] = ov[sel]
                s = s / (s.sum() + f32(1e-8))
            else:
                s[:n][sel] = np.where(ov[sel] < .6, .8, np.where(ov[sel] < .7, .9, 1.))
            scores[b] = s
            bmask[b, :n, 0][sel] = 1
        # bbox_transform: the proposal side is float32 arithmetic, the ground-truth side, division and log float64
        ew = p[:, 2] - p[:, 0] + f32(1.0)
        eh = p[:, 3] - p[:, 1] + f32(1.0)
        ecx = p[:, 0] + f32(0.5) * ew
        ecy = p[:, 1] + f32(0.5) * eh
        gw, gh = q[2] - q[0] + 1.0, q[3] - q[1] + 1.0
        gcx, gcy = q[0] + 0.5 * gw, q[1] + 0.5 * gh
        ew64, eh64 = ew.astype(np.float64), eh.astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.stack(((gcx - ecx.astype(np.float64)) / ew64, (gcy - ecy.astype(np.float64)) / eh64,
                          np.log(gw / ew64), np.log(gh / eh64)), 1)
            if norm is not None:
                t = (t - norm[0]) / norm[1]
        trans[b, :n] = t.astype(f32)
    return scores, smask, trans, bmask


def _ground_np(ps, reg, bbox, shape, gt, thr):
    B = ps.shape[0]
    f32 = np.float32
    idx = np.argmax(ps, axis=1)
    ar = np.arange(B)
    bx, d = bbox[ar, idx], reg[ar, idx]
    w = bx[:, 2] - bx[:, 0] + f32(1.0)
    h = bx[:, 3] - bx[:, 1] + f32(1.0)
    cx = bx[:, 0] + f32(0.5) * w
    cy = bx[:, 1] + f32(0.5) * h
    pcx = d[:, 0] * w + cx
    pcy = d[:, 1] * h + cy
    with np.errstate(over='ignore', invalid='ignore'):
        pw = np.exp(d[:, 2]) * w
        ph = np.exp(d[:, 3]) * h
        box = np.stack((pcx - f32(0.5) * pw, pcy - f32(0.5) * ph, pcx + f32(0.5) * pw, pcy + f32(0.5) * ph), 1)
    xm = shape[:, 1] - f32(1)
    ym = shape[:, 0] - f32(1)
    for k, m in ((0, xm), (1, ym), (2, xm), (3, ym)):
        box[:, k] = np.maximum(np.minimum(box[:, k], m), f32(0))
    g = gt.astype(np.float64)
    iou = np.array([_iou_np(box[b:b + 1].astype(np.float64), g[b])[0] for b in range(B)], np.float64).reshape(B)
    return idx.astype(np.int64), box.astype(f32), iou, iou >= thr


# ---- public functions ----------------------------------------------------------------------------------------------------------
def grounding_targets(bbox, nobj, gt, cfg, check=True):
    """VGD training targets for a batch: bbox [B,S,4] float32 proposals (x1,y1,x2,y2), nobj [B] integer (1 <= nobj <= S: the
    valid rows), gt [B,4] float64 referred box (x1,y1,x2,y2 = x, y, x + w, y + h as the loader forms it).  cfg supplies
    OVERLAP_THRESHOLD, SCORES_LOSS ('kld' / 'bce') and BBOX_NORM (with BBOX_NORM_MEANS / BBOX_NORM_STDS).

    Returns dict(scores [B,S], scores_mask [B,1], bbox [B,S,4], bbox_mask [B,S,1]), float32 on bbox's device: what
    harness.vgd_loss takes.  Rows at or past nobj[b] are zero everywhere.  check=False skips reading back the device's error flag
    (a host sync); invalid values then go unreported."""
    _require(bbox, 'bbox', (None, None, 4), (torch.float32,))
    B, S = bbox.shape[:2]
    _require(nobj, 'nobj', (B,), _INT)
    _require(gt, 'gt', (B, 4), (torch.float64,))
    if not 1 <= S <= MAX_REGIONS:
        raise ValueError('grounding_targets: S=%d regions (1 <= S <= %d)' % (S, MAX_REGIONS))
    for t, name in ((nobj, 'nobj'), (gt, 'gt')):
        if t.device != bbox.device:
            raise ValueError('grounding_targets: %s is on %s, bbox on %s' % (name, t.device, bbox.device))
    mode = cfg.SCORES_LOSS
    if mode not in _MODES:
        raise ValueError("grounding_targets: SCORES_LOSS must be 'kld' or 'bce', got %r" % (mode,))
    thr = float(cfg.OVERLAP_THRESHOLD)
    norm = _cfg_norm(cfg)
    if not bbox.is_cuda:
        n = nobj.numpy()
        if B and (n.min() < 1 or n.max() > S):
            raise GroundingError('grounding_targets: nobj outside 1..S=%d' % S)
        b, g = bbox.detach().numpy(), gt.detach().numpy()
        fin = all(np.isfinite(b[i, :n[i]]).all() for i in range(B)) and np.isfinite(g).all()
        if not fin:
            raise GroundingError('grounding_targets: a NaN or infinite input')
        out = _targets_np(b, n, g, thr, mode, norm)
        return dict(zip(('scores', 'scores_mask', 'bbox', 'bbox_mask'), (torch.from_numpy(a) for a in out)))
    dev = bbox.device
    bbox, gt = bbox.contiguous(), gt.contiguous()
    nobj = nobj.to(torch.int32).contiguous()
    scores = torch.empty(B, S, dtype=torch.float32, device=dev)
    smask = torch.empty(B, 1, dtype=torch.float32, device=dev)
    trans = torch.empty(B, S, 4, dtype=torch.float32, device=dev)
    bmask = torch.empty(B, S, 1, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if B:
        nv = None
        if norm is not None:
            nv = (ctypes.c_double * 8)(*np.concatenate(norm).tolist())
        with torch.cuda.device(dev):
            L.check(L.lib().mmnas_vgd_targets(L.ptr(bbox), L.ptr(nobj), L.ptr(gt), B, S, thr, _MODES[mode], nv, L.ptr(scores),
                                              L.ptr(smask), L.ptr(trans), L.ptr(bmask), L.ptr(flag), L.stream()))
        if check:
            _raise_flag(int(flag.item()), 'grounding_targets')
    return dict(scores=scores, scores_mask=smask, bbox=trans, bbox_mask=bmask)


def _ground_args(pred_scores, pred_reg, bbox, img_shape, gt):
    _require(pred_scores, 'pred_scores', (None, None), (torch.float32,))
    B, S = pred_scores.shape
    if gt.dim() == 3:   # the loader's [B,1,4]: the evaluation reads gt[:, 0]
        _require(gt, 'gt', (B, 1, 4), (torch.float32,))
        gt = gt[:, 0]
    _require(pred_reg, 'pred_reg', (B, S, 4), (torch.float32,))
    _require(bbox, 'bbox', (B, S, 4), (torch.float32,))
    _require(img_shape, 'img_shape', (B, 2), (torch.float32,))
    _require(gt, 'gt', (B, 4), (torch.float32,))
    if not 1 <= S <= MAX_REGIONS:
        raise ValueError('ground_batch: S=%d regions (1 <= S <= %d)' % (S, MAX_REGIONS))
    for t, name in ((pred_reg, 'pred_reg'), (bbox, 'bbox'), (img_shape, 'img_shape'), (gt, 'gt')):
        if t.device != pred_scores.device:
            raise ValueError('ground_batch: %s is on %s, pred_scores on %s' % (name, t.device, pred_scores.device))
    return B, S, gt


def _ground_device(pred_scores, pred_reg, bbox, img_shape, gt, thr, counts, flag):
    B, S = pred_scores.shape
    dev = pred_scores.device
    idx = torch.empty(B, dtype=torch.int64, device=dev)
    box = torch.empty(B, 4, dtype=torch.float32, device=dev)
    iou = torch.empty(B, dtype=torch.float64, device=dev)
    hit = torch.empty(B, dtype=torch.bool, device=dev)
    if B:
        c = [t.contiguous() for t in (pred_scores, pred_reg, bbox, img_shape, gt)]
        with torch.cuda.device(dev):
            L.check(L.lib().mmnas_vgd_ground(*[L.ptr(t) for t in c], B, S, float(thr), L.ptr(idx), L.ptr(box), L.ptr(iou),
                                             L.ptr(hit), L.ptr(counts), L.ptr(flag), L.stream()))
    return dict(idx=idx, box=box, iou=iou, hit=hit)


def ground_batch(pred_scores, pred_reg, bbox, img_shape, gt, thr, check=True):
    """One evaluation batch of train_vgd.py:436-453.  pred_scores [B,S] and pred_reg [B,S,4] (the network's outputs),
    bbox [B,S,4] proposals, img_shape [B,2] = (h, w), gt [B,4] (or the loader's [B,1,4]), all float32; thr = OVERLAP_THRESHOLD.

    Returns dict(idx [B] int64 argmax region (lowest index on a tie), box [B,4] float32 its decoded and clipped box,
    iou [B] float64, hit [B] bool = iou >= thr), on pred_scores' device.  check=False skips reading back the device's error
    flag (a host sync): the call then never synchronises."""
    B, S, gt = _ground_args(pred_scores, pred_reg, bbox, img_shape, gt)
    if not pred_scores.is_cuda:
        arrs = [t.detach().numpy() for t in (pred_scores, pred_reg, bbox, img_shape, gt)]
        if not (np.isfinite(arrs[0]).all() and np.isfinite(arrs[1]).all()):
            raise GroundingError('ground_batch: a NaN or infinite input')
        out = _ground_np(*arrs, float(thr))
        return dict(zip(('idx', 'box', 'iou', 'hit'), (torch.from_numpy(np.asarray(a)) for a in out)))
    flag = torch.zeros(1, dtype=torch.int32, device=pred_scores.device)
    out = _ground_device(pred_scores, pred_reg, bbox, img_shape, gt, thr, None, flag)
    if check:
        _raise_flag(int(flag.item()), 'ground_batch')
    return out


# ---- evaluator -----------------------------------------------------------------------------------------------------------------
class GroundingEvaluator:
    """The evaluation of train_vgd.py:387-478 for a VGD network (mmnas.model.full_vgd.Net_Full, or DDP around one).

    update() runs the network in eval mode under torch.no_grad() on one batch, with proj_reg rescaled for BBOX_NORM
    (W * std, b * std + mean: the reference's float32 operations) for the duration of the call only -- written into the
    parameters in place and restored in place, so their storage (and an optimizer's flat buffer they may be views of) is
    untouched -- then ground_batch; the (hits, count) pair and the error flag stay on the device.  compute() all-reduces them
    over a process group when one is up and returns {'accuracy' (percent), 'hits', 'count'}; it raises GroundingError if any
    batch held a NaN or infinite score or delta."""

    def __init__(self, net, cfg):
        if isinstance(net, torch.nn.parallel.DistributedDataParallel):
            net = net.module
        if getattr(net, 'TASK', None) != 'vgd' or not hasattr(net, 'proj_reg'):
            raise ValueError('GroundingEvaluator: needs a VGD network, got %s' % type(net).__name__)
        self.net, self.cfg = net, cfg
        self.thr = float(cfg.OVERLAP_THRESHOLD)
        self.norm = _cfg_norm(cfg)
        dev = net.proj_reg.weight.device
        self._counts = torch.zeros(2, dtype=torch.int64, device=dev)
        self._flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._host = None   # CPU networks: (hits, count, flag) accumulated on the host

    def reset(self):
        self._counts.zero_()
        self._flag.zero_()
        self._host = None

    @contextlib.contextmanager
    def _eval(self):
        """Eval mode + no_grad + proj_reg rescaled (train_vgd.py:410-420, restored as :455-460 but in place)."""
        net = self.net
        flags = [(m, m.training) for m in net.modules()]
        W, b = net.proj_reg.weight, net.proj_reg.bias
        saved = None
        try:
            net.eval()
            with torch.no_grad():
                if self.norm is not None:
                    saved = (W.detach().clone(), b.detach().clone())
                    std = torch.from_numpy(np.array(self.norm[1])).to(W.device).float()
                    mean = torch.from_numpy(np.array(self.norm[0])).to(W.device).float()
                    W.copy_(saved[0] * torch.unsqueeze(std, 1))
                    b.copy_(saved[1] * std + mean)
                yield
        finally:
            if saved is not None:
                with torch.no_grad():
                    W.copy_(saved[0])
                    b.copy_(saved[1])
            for m, t in flags:
                m.training = t

    def update(self, inputs, bbox, img_shape, gt):
        """One evaluation batch: inputs = the network's 5-tuple (frcn_feat, bbox_feat, rel_img, query_ix, rel_query);
        bbox [B,S,4] proposals, img_shape [B,2] = (h, w), gt [B,4] or [B,1,4].  No host synchronisation on the device."""
        with self._eval():
            pred_scores, pred_reg = self.net(tuple(inputs))
        B, S, g = _ground_args(pred_scores, pred_reg, bbox, img_shape, gt)
        if pred_scores.is_cuda:
            return _ground_device(pred_scores, pred_reg, bbox, img_shape, g, self.thr, self._counts, self._flag)
        try:
            out = ground_batch(pred_scores, pred_reg, bbox, img_shape, g, self.thr)
            h = (int(out['hit'].sum()), B, 0)
        except GroundingError:
            out, h = None, (0, B, ERR_NONFINITE)
        p = self._host or (0, 0, 0)
        self._host = (p[0] + h[0], p[1] + h[1], p[2] | h[2])
        return out

    def compute(self, group=None):
        """{'accuracy': 100 * hits / count, 'hits', 'count'} over every update() since construction / reset(), summed over the
        ranks of `group` (default: the default process group) when torch.distributed is initialised."""
        if self._host is not None:
            v = torch.tensor(self._host, dtype=torch.int64)
        else:
            v = torch.cat((self._counts, self._flag.to(torch.int64)))
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            if dist.get_backend(group) == 'gloo':
                v = v.cpu()
            v = v.clone()
            dist.all_reduce(v, group=group)
        hits, count, flag = (int(x) for x in v.cpu().tolist())
        if flag:
            raise GroundingError('GroundingEvaluator: a NaN or infinite score or delta in an evaluated batch')
        return {'accuracy': hits / float(count) * 100. if count else float('nan'), 'hits': hits, 'count': count}
