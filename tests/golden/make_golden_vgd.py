"""Generate tests/golden/vgd.npz: the visual grounding targets and evaluation of the *imported reference* (the reference
checkout, available in the build container only) on deterministic batches, for mmnas_amd/grounding.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vgd.py

* targets: load_data_vgd.py proc_bbox_label (with get_sigmoid_score and proc_img_feat), compiled out of the loader with `ast`
  as make_golden._extract_functions does (the loader imports spacy / GloVe at module level), over overlaps.py bbox_overlaps
  (the pure-Python twin of bbox.pyx) and bbox_transform.py bbox_transform;
* evaluation: bbox_transform_inv, np.argmax, clip_boxes and bbox_overlaps called exactly as train_vgd.py:436-453 calls them.

Every batch stores its inputs beside the outputs (key prefix `b<k>|`), so the tests need nothing else.  Only arrays are
written -- no reference source, bytecode or pickled object.
"""
import ast
import copy
import importlib.util
import os
import sys
from types import SimpleNamespace

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MMNAS_REFERENCE', '/root/reference')

import numpy as np

S = 100          # the loader's padding (proc_img_feat(..., img_feat_pad_size=100))
MODES = ('kld', 'bce')
NORM_STD = ((0.0, 0.0, 0.0, 0.0), (0.1, 0.1, 0.2, 0.2))
NORM_ODD = ((0.01, -0.02, 0.05, -0.1), (0.1, 0.13, 0.2, 0.27))


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _NumpyFloat:
    """`np` for the loader's code: numpy 2 has no np.float (the loader's float64 alias)."""

    def __getattr__(self, k):
        return np.float64 if k == 'float' else getattr(np, k)


def load_reference():
    bt = _module(os.path.join(REF, 'mmnas', 'utils', 'bbox_transform.py'), 'ref_bbox_transform')
    ovl = _module(os.path.join(REF, 'mmnas', 'utils', 'overlaps.py'), 'ref_overlaps')
    path = os.path.join(REF, 'mmnas', 'loader', 'load_data_vgd.py')
    tree = ast.parse(open(path).read(), filename=path)
    names = {'get_sigmoid_score', 'proc_bbox_label', 'proc_img_feat'}
    picked = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in picked) == sorted(names)
    ns = {'np': _NumpyFloat(), 'copy': copy, 'bbox_overlaps': ovl.bbox_overlaps, 'bbox_transform': bt.bbox_transform}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, 'exec'), ns)
    return bt, ovl, ns


def _loader_self(ns, cfg):
    """The DataSet instance the methods see.  Compiled outside the class, `self.__C` is not name-mangled: the attribute is
    literally `__C`."""
    me = SimpleNamespace()
    setattr(me, '__C', cfg)
    me.get_sigmoid_score = lambda overlap, thr: ns['get_sigmoid_score'](me, overlap, thr)
    me.proc_img_feat = lambda feat, img_feat_pad_size: ns['proc_img_feat'](me, feat, img_feat_pad_size)
    return me


# ---- deterministic batches ---------------------------------------------------------------------------------------------------
def _random_batch(rs, B, thr, mode, norm):
    """Random proposals inside varied images, the referred box near one of them (so that IoU >= thr occurs), nobj 1..100."""
    nobj = rs.randint(1, S + 1, size=B)
    nobj[0], nobj[1 % B] = 1, S
    shape = np.stack((rs.randint(200, 801, size=B), rs.randint(200, 801, size=B)), 1).astype(np.float32)   # (h, w)
    bbox = np.zeros((B, S, 4), np.float32)
    refs = []
    for b in range(B):
        h, w = shape[b]
        n = nobj[b]
        x1 = rs.uniform(-5, 0.8 * w, n)
        y1 = rs.uniform(-5, 0.8 * h, n)
        bw = rs.uniform(0, 0.5 * w, n)
        bh = rs.uniform(0, 0.5 * h, n)
        box = np.stack((x1, y1, x1 + bw, y1 + bh), 1)
        box[::3] = np.round(box[::3])             # some integer boxes
        bbox[b, :n] = box.astype(np.float32)
        k = rs.randint(n)
        p = bbox[b, k].astype(np.float64)
        pw, ph = p[2] - p[0] + 1, p[3] - p[1] + 1
        x, y = p[0] + rs.uniform(-0.15, 0.15) * pw, p[1] + rs.uniform(-0.15, 0.15) * ph
        refs.append([round(float(x), 2), round(float(y), 2), round(float(pw * rs.uniform(0.7, 1.3)), 2),
                     round(float(ph * rs.uniform(0.7, 1.3)), 2)])
    # network outputs: log-softmax scores (full_vgd.py with kld), small deltas; half the samples pick their best proposal
    logits = rs.standard_normal((B, S)).astype(np.float32)
    logits[:, :] -= np.log(np.exp(logits.astype(np.float64)).sum(1, keepdims=True)).astype(np.float32)
    reg = (0.3 * rs.standard_normal((B, S, 4))).astype(np.float32)
    return dict(bbox=bbox, nobj=nobj.astype(np.int32), refs=refs, thr=thr, mode=mode, norm=norm, img_shape=shape,
                pred_scores=logits, pred_reg=reg, best_pick=(rs.uniform(size=B) < 0.5))


def _crafted_batch(mode, norm):
    """The edge cases, one per sample (S = 100 rows; rows past nobj are zero padding)."""
    samples = []   # (proposals, refs [x, y, w, h], img (h, w), argmax row, deltas of that row, tie rows)
    # (bbox_transform_inv with zero deltas maps [x1, y1, x2, y2] to [x1, y1, x2 + 1, y2 + 1]: the eval rows below are the
    #  target boxes shrunk by one pixel)
    # 0: a proposal equal to the referred box (IoU 1), and one that decodes to it
    samples.append(([[10, 20, 60, 60], [10, 20, 59, 59], [0, 0, 30, 30], [100, 100, 200, 150]], [10, 20, 50, 40], (480, 640), 1,
                    (0, 0, 0, 0), ()))
    # 1: IoU exactly 0.5 with integer boxes: gt [0,0,9,9], proposal [0,0,9,4]; the eval decodes [0,0,8,3] to [0,0,9,4]
    samples.append(([[0, 0, 9, 4], [0, 0, 8, 3], [50, 50, 80, 80]], [0, 0, 9, 9], (480, 640), 1, (0, 0, 0, 0), ()))
    # 2: touching boxes (iw == 0, ih == 0): no target; the eval scores the touching one
    samples.append(([[10, 0, 19, 9], [0, 10, 9, 19], [10, 10, 19, 19]], [0, 0, 9, 9], (480, 640), 0, (0, 0, 0, 0), ()))
    # 3: zero-width boxes (x2 == x1)
    samples.append(([[5, 5, 5, 9], [5, 5, 5, 5], [7, 5, 7, 9]], [5, 5, 0, 4], (480, 640), 0, (0, 0, 0, 0), ()))
    # 4: boxes outside the image and negative coordinates (clipping)
    samples.append(([[-20, -10, 30, 40], [600, 400, 700, 500], [-50, -50, -10, -10]], [0, 0, 40, 45], (480, 640), 1,
                    (0.4, 0.3, 0.2, 0.1), ()))
    # 5: no proposal at or above the threshold (scores_mask 0, transformed still filled)
    samples.append(([[0, 0, 3, 3], [300, 300, 310, 305], [100, 0, 140, 20]], [200, 200, 60, 60], (480, 640), 2, (0, 0, 0, 0), ()))
    # 6: exact score ties: rows 3 and 7 share the maximum (np.argmax: row 3)
    samples.append(([[10, 10, 50, 50], [12, 12, 48, 52], [0, 0, 60, 60], [11, 9, 49, 51], [8, 8, 52, 52], [10, 12, 50, 50],
                     [9, 11, 51, 49], [10, 10, 50, 51]], [10, 10, 40, 40], (300, 300), 3, (0.01, -0.02, 0.03, -0.04), (7,)))
    # 7: the argmax on a padded row (nobj = 5, row 50 all zero)
    samples.append(([[10, 10, 50, 50], [20, 20, 30, 30], [0, 0, 5, 5], [40, 40, 90, 90], [15, 15, 45, 45]], [10, 10, 40, 40],
                    (300, 400), 50, (0.1, 0.1, 1.5, 1.2), ()))
    # 8: |dw| about 10: a one-pixel proposal against the whole image (targets ~ log 640), deltas +-10 (a clipped whole-image box)
    samples.append(([[100, 100, 100, 100], [0, 0, 639, 479], [200, 150, 201, 151]], [0, 0, 639, 479], (480, 640), 0,
                    (0.2, -0.1, 10.0, 9.5), ()))
    # 9: IoU exactly 0.5 against a wider box: gt [0,0,19,9], proposal [0,0,9,9]; the eval decodes [0,0,8,8] to [0,0,9,9]
    samples.append(([[0, 0, 9, 9], [0, 0, 8, 8], [30, 30, 40, 40]], [0, 0, 19, 9], (100, 100), 1, (0, 0, 0, 0), ()))
    B = len(samples)
    bbox = np.zeros((B, S, 4), np.float32)
    nobj = np.zeros(B, np.int32)
    shape = np.zeros((B, 2), np.float32)
    scores = np.full((B, S), -10.0, np.float32)
    reg = np.zeros((B, S, 4), np.float32)
    refs = []
    rs = np.random.RandomState(77)
    for b, (props, ref, img, arg, delta, ties) in enumerate(samples):
        n = len(props)
        bbox[b, :n] = np.asarray(props, np.float32)
        nobj[b] = n
        shape[b] = img
        refs.append([float(v) for v in ref])
        scores[b] = (-5.0 - rs.uniform(size=S)).astype(np.float32)
        scores[b, arg] = -0.25
        for t in ties:
            scores[b, t] = -0.25
        reg[b] = (0.05 * rs.standard_normal((S, 4))).astype(np.float32)
        reg[b, arg] = np.asarray(delta, np.float32)
    return dict(bbox=bbox, nobj=nobj, refs=refs, thr=0.5, mode=mode, norm=norm, img_shape=shape, pred_scores=scores,
                pred_reg=reg, best_pick=np.zeros(B, bool))


def batches():
    rs = np.random.RandomState(20261016)
    out = [_random_batch(rs, 16, 0.5, 'kld', None), _random_batch(rs, 16, 0.5, 'kld', NORM_STD),
           _random_batch(rs, 16, 0.5, 'bce', NORM_ODD), _random_batch(rs, 16, 0.4, 'bce', None),
           _crafted_batch('kld', None), _crafted_batch('bce', NORM_STD)]
    return out


# ---- the reference on them ---------------------------------------------------------------------------------------------------
def run(bt, ovl, ns, k, c):
    cfg = SimpleNamespace(OVERLAP_THRESHOLD=c['thr'], SCORES_LOSS=c['mode'], BBOX_NORM=c['norm'] is not None,
                          BBOX_NORM_MEANS=list(c['norm'][0]) if c['norm'] else None,
                          BBOX_NORM_STDS=list(c['norm'][1]) if c['norm'] else None)
    me = _loader_self(ns, cfg)
    B = c['bbox'].shape[0]
    bbox, nobj = c['bbox'], c['nobj']
    out = {}
    gt64 = np.zeros((B, 4), np.float64)
    t_scores, t_smask = np.zeros((B, S), np.float32), np.zeros((B, 1), np.float32)
    t_bbox, t_bmask = np.zeros((B, S, 4), np.float32), np.zeros((B, S, 1), np.float32)
    for b in range(B):
        refs = {'bbox': list(c['refs'][b])}
        g = copy.deepcopy(refs['bbox'])     # load_data_vgd.py:165-168
        g[2] = g[0] + g[2]
        g[3] = g[1] + g[3]
        gt64[b] = g
        sc, sm, tb, bm = ns['proc_bbox_label'](me, refs, {'bbox': bbox[b, :nobj[b]]})
        # load_data_vgd.py:187-190: torch.from_numpy(...).float() (bbox_mask .unsqueeze(-1))
        t_scores[b], t_smask[b] = sc.astype(np.float32), sm.astype(np.float32)
        t_bbox[b], t_bmask[b, :, 0] = tb.astype(np.float32), bm.astype(np.float32)
    # eval inputs as the loader hands them over: gt [B,1,4] float32, bbox padded to 100 rows, img_shape float32
    pred_scores, pred_reg = c['pred_scores'].copy(), c['pred_reg'].copy()
    for b in np.nonzero(c['best_pick'])[0]:
        ov = ovl.bbox_overlaps(bbox[b, :nobj[b]].astype(np.float64), gt64[b:b + 1])[:, 0]
        pred_scores[b, int(np.argmax(ov))] = 0.0
    eval_gt_bbox = gt64.astype(np.float32)[:, None, :]
    eval_bbox, eval_img_shape = bbox.copy(), c['img_shape'].copy()
    # train_vgd.py:439-453
    bbox_reg = bt.bbox_transform_inv(eval_bbox.reshape(-1, 4), pred_reg.reshape(-1, 4)).reshape(-1, S, 4)
    arg_pred_scores = np.argmax(pred_scores, axis=1)
    e_box, e_iou, e_hit = np.zeros((B, 4), np.float32), np.zeros(B, np.float64), np.zeros(B, bool)
    for step_ix in range(pred_scores.shape[0]):
        cliped_bbox_reg_ix = bt.clip_boxes(bbox_reg[step_ix], eval_img_shape[step_ix])
        overlaps = ovl.bbox_overlaps(
            np.ascontiguousarray(cliped_bbox_reg_ix[arg_pred_scores[step_ix]][np.newaxis, :], dtype=np.float64),
            np.ascontiguousarray(eval_gt_bbox[step_ix], dtype=np.float64))[:, 0]
        e_box[step_ix] = cliped_bbox_reg_ix[arg_pred_scores[step_ix]]
        e_iou[step_ix] = overlaps[0]
        e_hit[step_ix] = bool(overlaps >= c['thr'])
    p = 'b%d|' % k
    out.update({p + 'bbox': bbox, p + 'nobj': nobj, p + 'gt': gt64, p + 'thr': np.float64(c['thr']),
                p + 'mode': np.int32(MODES.index(c['mode'])),
                p + 'norm': np.asarray(c['norm'], np.float64).reshape(-1) if c['norm'] else np.zeros(0, np.float64),
                p + 'img_shape': eval_img_shape, p + 'gt32': eval_gt_bbox, p + 'pred_scores': pred_scores, p + 'pred_reg': pred_reg,
                p + 't_scores': t_scores, p + 't_scores_mask': t_smask, p + 't_bbox': t_bbox, p + 't_bbox_mask': t_bmask,
                p + 't_iou': np.stack([np.pad(ovl.bbox_overlaps(bbox[b, :nobj[b]].astype(np.float64), gt64[b:b + 1])[:, 0],
                                              (0, S - nobj[b])) for b in range(B)]),
                p + 'e_idx': arg_pred_scores.astype(np.int64), p + 'e_box': e_box, p + 'e_iou': e_iou, p + 'e_hit': e_hit})
    return out


def gen_vgd():
    bt, ovl, ns = load_reference()
    out = {}
    with np.errstate(divide='ignore', invalid='ignore'):
        for k, c in enumerate(batches()):
            out.update(run(bt, ovl, ns, k, c))
    out['n_batches'] = np.int32(len(batches()))
    np.savez_compressed(os.path.join(HERE, 'vgd.npz'), **out)
    return out


if __name__ == '__main__':
    gen_vgd()
    print('wrote', os.path.join(HERE, 'vgd.npz'), os.path.getsize(os.path.join(HERE, 'vgd.npz')), 'bytes')
