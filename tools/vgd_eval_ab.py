"""A/B of the visual grounding evaluation and targets at the train_vgd batch (B = 64, 100 regions), random inputs.

  eval   A  the reference's host evaluation of one batch (train_vgd.py:436-453) statement for statement on outputs that are
            on the device: the device->host copies, bbox_transform_inv of every row, np.argmax, then per sample clip_boxes
            and a bbox_overlaps of the argmax box (the Python twin of the Cython routine);
         B  what GroundingEvaluator.update adds behind the shared forward: mmnas_vgd_ground with the device counters
            (no host synchronisation; timed as --inner back-to-back calls closed by one synchronize).
  targets A  proc_bbox_label per sample x 64 (numpy, vectorised IoU -- as fast as the Cython bbox_overlaps or faster),
            then the host->device copy of the four target tensors;
          B  grounding_targets on the device (check=False, then one synchronize).

A and B alternate, --rounds each; the median microseconds per batch of each and their ratio are printed, then one JSON line.

  python tools/vgd_eval_ab.py [--rounds 7 --inner 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(B, S, dev, seed=5):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(0, 300, (B, S, 2))
    bbox = np.concatenate((xy, xy + rs.uniform(5, 200, (B, S, 2))), -1).astype(np.float32)
    img = np.stack((rs.randint(300, 600, B), rs.randint(300, 700, B)), 1).astype(np.float32)
    logits = torch.log_softmax(torch.from_numpy(rs.standard_normal((B, S)).astype(np.float32)), -1)
    k = rs.randint(0, S, B)
    k[::2] = logits.argmax(1).numpy()[::2]      # half the samples: the referred box lies near the predicted region
    gt64 = bbox[np.arange(B), k].astype(np.float64) + rs.uniform(-8, 8, (B, 4))
    reg = (0.2 * rs.standard_normal((B, S, 4))).astype(np.float32)
    nobj = rs.randint(10, S + 1, B).astype(np.int32)
    host = dict(bbox=bbox, img=img, gt32=gt64.astype(np.float32)[:, None, :], gt64=gt64, nobj=nobj)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
    d['scores'], d['reg'] = logits.to(dev), torch.from_numpy(reg).to(dev)
    return host, d


def reference_eval(d, host, thr):
    """train_vgd.py:436-453 (the outputs arrive on the device, as net() leaves them)."""
    pred_scores = d['scores'].cpu().data.numpy()
    pred_reg = d['reg'].cpu().data.numpy()
    eval_bbox, eval_img_shape, eval_gt_bbox = host['bbox'], host['img'], host['gt32']
    B, S = pred_scores.shape
    # every row decoded (bbox_transform_inv over all B * S rows, float32)
    p, dl = eval_bbox.reshape(-1, 4), pred_reg.reshape(-1, 4)
    w = p[:, 2] - p[:, 0] + np.float32(1)
    h = p[:, 3] - p[:, 1] + np.float32(1)
    cx = p[:, 0] + np.float32(0.5) * w
    cy = p[:, 1] + np.float32(0.5) * h
    ncx, ncy = dl[:, 0] * w + cx, dl[:, 1] * h + cy
    nw, nh = np.exp(dl[:, 2]) * w, np.exp(dl[:, 3]) * h
    half_w, half_h = np.float32(0.5) * nw, np.float32(0.5) * nh
    bbox_reg = np.stack((ncx - half_w, ncy - half_h, ncx + half_w, ncy + half_h), 1).reshape(B, S, 4)
    arg = np.argmax(pred_scores, axis=1)
    acc = n = 0
    for i in range(pred_scores.shape[0]):
        bx, (ih_, iw_) = bbox_reg[i], eval_img_shape[i]     # clip_boxes on all S rows of the sample
        lim = np.array([iw_, ih_, iw_, ih_], np.float32) - np.float32(1)
        bx[:] = np.maximum(np.minimum(bx, lim), np.float32(0))
        b = np.ascontiguousarray(bx[arg[i]][np.newaxis, :], dtype=np.float64)
        q = np.ascontiguousarray(eval_gt_bbox[i], dtype=np.float64)
        ov = 0.0
        box_area = (q[0, 2] - q[0, 0] + 1) * (q[0, 3] - q[0, 1] + 1)
        iw = min(b[0, 2], q[0, 2]) - max(b[0, 0], q[0, 0]) + 1
        if iw > 0:
            ih = min(b[0, 3], q[0, 3]) - max(b[0, 1], q[0, 1]) + 1
            if ih > 0:
                ov = iw * ih / float((b[0, 2] - b[0, 0] + 1) * (b[0, 3] - b[0, 1] + 1) + box_area - iw * ih)
        n += 1
        acc += ov >= thr
    return acc, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--regions', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50)
    args = ap.parse_args()
    from mmnas_amd import grounding as G
    dev = 'cuda:0'
    B, S, thr = args.batch, args.regions, 0.5
    host, d = inputs(B, S, dev)
    cfg = type('cfg', (), dict(OVERLAP_THRESHOLD=thr, SCORES_LOSS='kld', BBOX_NORM=True, BBOX_NORM_MEANS=[0.0] * 4,
                                BBOX_NORM_STDS=[0.1, 0.1, 0.2, 0.2]))
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    gt2 = d['gt32'][:, 0].contiguous()

    def eval_a():
        return reference_eval(d, host, thr)

    def eval_b():
        for _ in range(args.inner):
            G._ground_device(d['scores'], d['reg'], d['bbox'], d['img'], gt2, thr, counts, flag)
        torch.cuda.synchronize()

    def tgt_a():
        out = [G._targets_np(host['bbox'][b:b + 1], host['nobj'][b:b + 1], host['gt64'][b:b + 1], thr, 'kld', G._cfg_norm(cfg))
               for b in range(B)]
        res = [torch.from_numpy(np.concatenate([o[k] for o in out])).to(dev) for k in range(4)]
        torch.cuda.synchronize()
        return res

    def tgt_b():
        for _ in range(args.inner):
            G.grounding_targets(d['bbox'], d['nobj'], d['gt64'], cfg, check=False)
        torch.cuda.synchronize()

    # agreement first
    hits_ref, n_ref = eval_a()
    counts.zero_()
    G._ground_device(d['scores'], d['reg'], d['bbox'], d['img'], gt2, thr, counts, flag)
    assert counts.tolist() == [hits_ref, n_ref] and int(flag.item()) == 0, (counts.tolist(), hits_ref, n_ref)
    ta = tgt_a()
    tb = G.grounding_targets(d['bbox'], d['nobj'], d['gt64'], cfg)
    assert torch.equal(ta[0], tb['scores']) and torch.equal(ta[1], tb['scores_mask'])
    for f in (eval_a, eval_b, tgt_a, tgt_b):   # warm-up
        f()
    res = {'eval_ref_us': [], 'eval_dev_us': [], 'targets_ref_us': [], 'targets_dev_us': []}
    for _ in range(args.rounds):
        for key, f, reps in (('eval_ref_us', eval_a, 1), ('eval_dev_us', eval_b, args.inner), ('targets_ref_us', tgt_a, 1),
                             ('targets_dev_us', tgt_b, args.inner)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            res[key].append((time.perf_counter() - t0) * 1e6 / reps)
    med = {k: statistics.median(v) for k, v in res.items()}
    print('B=%d S=%d, median of %d alternating rounds (us per batch):' % (B, S, args.rounds))
    print('  eval     reference host %9.1f   device %7.1f   ratio %6.1fx' % (med['eval_ref_us'], med['eval_dev_us'],
                                                                          med['eval_ref_us'] / med['eval_dev_us']))
    print('  targets  reference host %9.1f   device %7.1f   ratio %6.1fx' % (med['targets_ref_us'], med['targets_dev_us'],
                                                                          med['targets_ref_us'] / med['targets_dev_us']))
    rec = dict(tool='vgd_eval_ab', B=B, S=S, rounds=args.rounds, inner=args.inner, median_us=med,
               eval_ratio=med['eval_ref_us'] / med['eval_dev_us'], targets_ratio=med['targets_ref_us'] / med['targets_dev_us'],
               all_us={k: [round(x, 2) for x in v] for k, v in res.items()}, device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
