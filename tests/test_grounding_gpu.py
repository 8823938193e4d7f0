"""mmnas_amd.grounding on the MI355X: mmnas_vgd_targets / mmnas_vgd_ground against the reference's own outputs
(tests/golden/vgd.npz) and against the numpy fallback on identical inputs, the device error flag, no host synchronisation in
ground_batch, GroundingEvaluator on a VGD Net_Full at the train_vgd dimensions against the reference evaluation restated on the
same network outputs, the in-place BBOX_NORM swap under FlatAdam, and device targets through harness.vgd_loss."""
import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_grounding_host import BATCHES, _cfg, ulps32

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy


def _dev(*a):
    return [T(np.ascontiguousarray(x)).to(DEV) for x in a]


def boxes_close(a, b):
    """Decoded boxes: within 4 ulp, or within 4 ulp of 1024 where x1 = ctr - w / 2 cancels to a small value (the last bits
    of the float32 exp differ between math libraries)."""
    return bool(((ulps32(a, b) <= 4) | (np.abs(a.astype(np.float64) - b) <= 4 * float(np.spacing(np.float32(1024))))).all())


@pytest.mark.parametrize('k', range(len(BATCHES)))
def test_targets_kernel_against_reference_and_fallback(k):
    from mmnas_amd.grounding import grounding_targets
    d = BATCHES[k]
    bbox, nobj, gt = _dev(d['bbox'], d['nobj'], d['gt'])
    t = {n: v.cpu().numpy() for n, v in grounding_targets(bbox, nobj, gt, d['cfg']).items()}
    f = {n: v.numpy() for n, v in grounding_targets(T(d['bbox']), T(d['nobj']), T(d['gt']), d['cfg']).items()}
    for ref in (f, {'scores': d['t_scores'], 'scores_mask': d['t_scores_mask'], 'bbox': d['t_bbox'], 'bbox_mask': d['t_bbox_mask']}):
        assert np.array_equal(t['scores_mask'], ref['scores_mask'])
        assert np.array_equal(t['bbox_mask'], ref['bbox_mask'])
        assert np.array_equal(t['scores'], ref['scores'])          # S = 100: numpy's pairwise order, bitwise
        assert int(ulps32(t['bbox'], ref['bbox']).max()) <= 1


@pytest.mark.parametrize('S', [1, 7, 129, 700, 1024])
def test_targets_kernel_long_rows_against_fallback(S):
    from mmnas_amd.grounding import grounding_targets
    rs = np.random.RandomState(S)
    B = 9
    xy = rs.uniform(0, 40, (B, S, 2))
    bbox = np.concatenate((xy, xy + rs.uniform(0, 60, (B, S, 2))), -1).astype(np.float32)
    nobj = rs.randint(1, S + 1, B).astype(np.int32)
    nobj[0] = S
    gt = np.concatenate((rs.uniform(0, 20, (B, 2)), rs.uniform(40, 80, (B, 2))), -1)
    for mode in ('kld', 'bce'):
        cfg = _cfg(SCORES_LOSS=mode, OVERLAP_THRESHOLD=0.3, BBOX_NORM=True, BBOX_NORM_MEANS=[0, 0.1, 0, 0],
                   BBOX_NORM_STDS=[0.1, 0.1, 0.2, 0.2])
        t = {n: v.cpu().numpy() for n, v in grounding_targets(*_dev(bbox, nobj, gt), cfg).items()}
        f = {n: v.numpy() for n, v in grounding_targets(T(bbox), T(nobj), T(gt), cfg).items()}
        if S > 128:
            assert t['scores_mask'].sum() > 0
        for n in ('scores_mask', 'bbox_mask', 'scores'):
            assert np.array_equal(t[n], f[n]), (mode, n)
        assert int(ulps32(t['bbox'], f['bbox']).max()) <= 1


@pytest.mark.parametrize('k', range(len(BATCHES)))
def test_ground_kernel_against_reference_and_fallback(k):
    from mmnas_amd.grounding import ground_batch
    d = BATCHES[k]
    thr = float(d['thr'])
    args = [d[n] for n in ('pred_scores', 'pred_reg', 'bbox', 'img_shape', 'gt32')]
    r = {n: v.cpu().numpy() for n, v in ground_batch(*_dev(*args), thr).items()}
    f = {n: v.numpy() for n, v in ground_batch(*(T(a) for a in args), thr).items()}
    near = (np.abs(d['e_iou'] - thr) < 1e-5) & (d['e_iou'] != thr)
    assert int(near.sum()) == 0
    for ref in (f, {'idx': d['e_idx'], 'box': d['e_box'], 'iou': d['e_iou'], 'hit': d['e_hit']}):
        assert np.array_equal(r['idx'], ref['idx'])
        assert boxes_close(r['box'], ref['box'])
        same = (r['box'] == ref['box']).all(1)
        assert np.array_equal(r['iou'][same], ref['iou'][same])     # IoU of equal boxes: bitwise
        assert np.allclose(r['iou'], ref['iou'], rtol=1e-4, atol=1e-6)
        assert np.array_equal(r['hit'], ref['hit'])


def test_ground_counts_accumulate_on_the_device():
    from mmnas_amd.grounding import _ground_device
    counts = torch.zeros(2, dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    hits = n = 0
    for d in BATCHES:
        args = _dev(*(d[k] for k in ('pred_scores', 'pred_reg', 'bbox', 'img_shape', 'gt32')))
        _ground_device(*args[:4], args[4][:, 0], float(d['thr']), counts, flag)
        hits += int(d['e_hit'].sum())
        n += len(d['e_hit'])
    assert counts.tolist() == [hits, n] and int(flag.item()) == 0


def test_device_error_flags_raise():
    from mmnas_amd.grounding import GroundingError, ground_batch, grounding_targets
    d = BATCHES[0]
    bbox, nobj, gt = _dev(d['bbox'], d['nobj'], d['gt'])
    S = bbox.shape[1]
    for bad in (0, S + 1):
        n = nobj.clone()
        n[5] = bad
        with pytest.raises(GroundingError, match='nobj'):
            grounding_targets(bbox, n, gt, _cfg())
        t = grounding_targets(bbox, n, gt, _cfg(), check=False)      # the sample's outputs are zero
        assert not t['scores'][5].any() and not t['bbox'][5].any() and not t['scores_mask'][5].any()
    g = gt.clone()
    g[2, 3] = float('inf')
    with pytest.raises(GroundingError, match='NaN or infinite'):
        grounding_targets(bbox, nobj, g, _cfg())
    args = _dev(*(d[k] for k in ('pred_scores', 'pred_reg', 'bbox', 'img_shape', 'gt32')))
    for i, v in ((0, float('nan')), (0, -float('inf')), (1, float('nan')), (1, float('inf'))):
        a = [x.clone() for x in args]
        a[i].view(-1)[123] = v
        with pytest.raises(GroundingError, match='NaN or infinite'):
            ground_batch(*a, 0.5)


def test_ground_batch_issues_no_host_sync():
    from mmnas_amd.grounding import ground_batch
    rs = np.random.RandomState(1)
    B, S = 64, 100
    d = BATCHES[0]
    bbox = np.tile(d['bbox'], (4, 1, 1))
    args = _dev(rs.standard_normal((B, S)).astype(np.float32), (0.2 * rs.standard_normal((B, S, 4))).astype(np.float32), bbox,
                np.tile(d['img_shape'], (4, 1)), np.tile(d['gt32'], (4, 1, 1)))
    ground_batch(*args, 0.5, check=False)     # (first call: library load, allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = ground_batch(*args, 0.5, check=False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    f = ground_batch(*(a.cpu() for a in args), 0.5)
    assert torch.equal(r['idx'].cpu(), f['idx'])


# ---- the evaluator on a VGD Net_Full at the train_vgd dimensions ------------------------------------------------------------------
NORM = dict(BBOX_NORM=True, BBOX_NORM_MEANS=[0.0, 0.0, 0.0, 0.0], BBOX_NORM_STDS=[0.1, 0.1, 0.2, 0.2])


def _vgd_case(HSIZE=512, B=64, seed=31):
    from mmnas.model.full_vgd import Net_Full
    c = cases.net_case('vgd', 'mmnas_vgd', seed, HSIZE=HSIZE, B=B, Sx=15, Sy=100, token_size=2000, ans_size=3129)
    net = Net_Full(c['cfg'], {'token_size': c['token_size'], 'ans_size': c['ans_size'],
                              'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)})
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    net = net.to(DEV).train()
    rs = np.random.RandomState(seed + 1)
    xy = rs.uniform(0, 300, (B, 100, 2))
    bbox = np.concatenate((xy, xy + rs.uniform(5, 200, (B, 100, 2))), -1).astype(np.float32)
    img = np.stack((rs.randint(300, 600, B), rs.randint(300, 700, B)), 1).astype(np.float32)
    gxy = rs.uniform(0, 250, (B, 2))
    gt = np.concatenate((gxy, gxy + rs.uniform(20, 250, (B, 2))), -1).astype(np.float32)[:, None, :]
    return net, c, bbox, img, gt


def _reference_eval(pred_scores, pred_reg, bbox, img_shape, gt, thr):
    """train_vgd.py:436-453 restated on the host: decode every row (bbox_transform_inv), np.argmax, clip_boxes, then
    overlaps.py bbox_overlaps in Python scalars per sample."""
    B, S = pred_scores.shape
    boxes, deltas = bbox.reshape(-1, 4), pred_reg.reshape(-1, 4)
    widths = boxes[:, 2] - boxes[:, 0] + np.float32(1.0)
    heights = boxes[:, 3] - boxes[:, 1] + np.float32(1.0)
    ctr_x = boxes[:, 0] + np.float32(0.5) * widths
    ctr_y = boxes[:, 1] + np.float32(0.5) * heights
    pcx = deltas[:, 0] * widths + ctr_x
    pcy = deltas[:, 1] * heights + ctr_y
    pw = np.exp(deltas[:, 2]) * widths
    ph = np.exp(deltas[:, 3]) * heights
    reg = np.stack((pcx - np.float32(0.5) * pw, pcy - np.float32(0.5) * ph, pcx + np.float32(0.5) * pw,
                    pcy + np.float32(0.5) * ph), 1).reshape(B, S, 4)
    arg = np.argmax(pred_scores, axis=1)
    hits, ious, out_box = 0, [], []
    for i in range(B):
        bx = reg[i].copy()
        for k, m in ((0, img_shape[i][1]), (1, img_shape[i][0]), (2, img_shape[i][1]), (3, img_shape[i][0])):
            bx[:, k] = np.maximum(np.minimum(bx[:, k], m - 1), 0)
        b = bx[arg[i]].astype(np.float64)
        q = gt[i, 0].astype(np.float64)
        box_area = (q[2] - q[0] + 1) * (q[3] - q[1] + 1)
        ov = 0.0
        iw = min(b[2], q[2]) - max(b[0], q[0]) + 1
        if iw > 0:
            ih = min(b[3], q[3]) - max(b[1], q[1]) + 1
            if ih > 0:
                ua = float((b[2] - b[0] + 1) * (b[3] - b[1] + 1) + box_area - iw * ih)
                ov = iw * ih / ua
        hits += ov >= thr
        ious.append(ov)
        out_box.append(bx[arg[i]])
    return arg, np.array(out_box), np.array(ious), int(hits)


def _reference_outputs(net, inputs):
    """The network's outputs with proj_reg rescaled the reference's way (params.data = ..., train_vgd.py:410-420)."""
    W, b = net.proj_reg.weight, net.proj_reg.bias
    w0, b0 = W.data, b.data
    std = torch.from_numpy(np.array(NORM['BBOX_NORM_STDS'])).to(DEV).float()
    mean = torch.from_numpy(np.array(NORM['BBOX_NORM_MEANS'])).to(DEV).float()
    flags = [(m, m.training) for m in net.modules()]
    net.eval()
    try:
        with torch.no_grad():
            W.data = w0 * torch.unsqueeze(std, 1)
            b.data = b0 * std + mean
            ps, pr = net(inputs)
    finally:
        W.data, b.data = w0, b0
        for m, t in flags:
            m.training = t
    return ps.cpu().numpy(), pr.cpu().numpy()


def test_evaluator_matches_the_reference_eval_at_train_vgd_dimensions():
    from mmnas_amd.grounding import GroundingEvaluator, ground_batch
    net, c, bbox, img, gt = _vgd_case()
    inputs = tuple(_dev(*c['inputs']))
    ps, pr = _reference_outputs(net, inputs)
    thr = 0.5
    arg, box, iou, hits = _reference_eval(ps, pr, bbox, img, gt, thr)
    # half the samples are given their own predicted box (plus a pixel) as the ground truth: hits on both sides of the count
    gt = gt.copy()
    gt[::2, 0] = box[::2] + np.float32(1)
    arg, box, iou, hits = _reference_eval(ps, pr, bbox, img, gt, thr)
    assert 0 < hits < len(arg)
    assert int((np.abs(iou - thr) < 1e-5).sum()) == 0
    cfg = _cfg(**NORM)
    ev = GroundingEvaluator(net, cfg)
    W, b = net.proj_reg.weight, net.proj_reg.bias
    w0, b0, ptrs = W.detach().clone(), b.detach().clone(), (W.data_ptr(), b.data_ptr())
    out = ev.update(inputs, *_dev(bbox, img, gt))
    r = ev.compute()
    assert r['count'] == len(arg) and r['hits'] == hits
    assert abs(r['accuracy'] - hits / float(len(arg)) * 100.) < 1e-12
    assert np.array_equal(out['idx'].cpu().numpy(), arg)
    assert boxes_close(out['box'].cpu().numpy(), box)
    assert torch.equal(W, w0) and torch.equal(b, b0) and (W.data_ptr(), b.data_ptr()) == ptrs
    assert net.training and all(m.training for m in net.modules())
    # the same outputs through ground_batch: the evaluator's forward is the reference's
    g = ground_batch(*_dev(ps, pr, bbox, img, gt), thr)
    assert torch.equal(g['idx'], out['idx']) and torch.equal(g['hit'], out['hit'])
    ev.update(inputs, *_dev(bbox, img, gt))
    assert ev.compute()['count'] == 2 * len(arg) and ev.compute()['hits'] == 2 * hits


def _train_step(net, opt, inputs, t):
    from mmnas_amd.harness import vgd_loss
    opt.zero_grad()
    ps, pr = net(inputs)
    loss = vgd_loss(ps, pr, t['scores'], t['scores_mask'], t['bbox'], t['bbox_mask'])
    loss.backward()
    opt.step()
    torch.cuda.synchronize()


def test_flat_adam_step_after_an_evaluator_call_is_unchanged():
    """The in-place BBOX_NORM swap leaves FlatAdam's flat buffer intact: from one optimizer state (after a real training step),
    an Adam step on a fixed gradient gives bitwise the same parameters with and without an evaluator call in between, and the
    parameters stay views into the buffer.  (A fixed gradient, because a network backward does not repeat bitwise: the
    embedding and split-K products add with atomics.)"""
    from mmnas_amd.grounding import GroundingEvaluator, grounding_targets
    from mmnas_amd.optim import FlatAdam
    B = 8
    net, c, bbox, img, gt = _vgd_case(HSIZE=128, B=B, seed=41)
    inputs = tuple(_dev(*c['inputs']))
    nobj = torch.full((B,), 100, dtype=torch.int32, device=DEV)
    t = grounding_targets(*_dev(bbox), nobj, T(gt[:, 0].astype(np.float64)).to(DEV), _cfg(**NORM))
    opt = FlatAdam(list(net.parameters()), lr=1e-3, betas=(0.9, 0.98), eps=1e-9)
    _train_step(net, opt, inputs, t)     # live moments
    snap = [x.clone() for x in (opt.flat_p, opt.m, opt.v)]
    gs = opt.global_step
    g = torch.randn(opt.fg.flat.shape, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    ev = GroundingEvaluator(net, _cfg(**NORM))
    W = net.proj_reg.weight
    res = []
    for with_eval in (False, True):
        for x, y in zip((opt.flat_p, opt.m, opt.v), snap):
            x.copy_(y)
        opt.global_step = gs
        if with_eval:
            ev.update(inputs, *_dev(bbox, img, gt))
            assert ev.compute()['count'] == B
            for x, y in zip((opt.flat_p, opt.m, opt.v), snap):
                assert torch.equal(x, y)
        for p, o in zip(opt.params, opt.fg.offsets):     # still views into the flat buffer
            assert p.data_ptr() == opt.flat_p[o:o + 1].data_ptr()
        opt.zero_grad()
        opt.fg.flat.copy_(g)
        opt.step()
        torch.cuda.synchronize()
        o = opt.fg.offsets[next(i for i, p in enumerate(opt.params) if p is W)]
        assert torch.equal(W.detach().reshape(-1), opt.flat_p[o:o + W.numel()])
        res.append(opt.flat_p.clone())
    assert not torch.equal(res[0], snap[0])
    assert torch.equal(res[0], res[1])


def test_device_targets_give_the_fallbacks_loss():
    from mmnas_amd.grounding import grounding_targets
    from mmnas_amd.harness import vgd_loss
    for d in BATCHES:
        rs = np.random.RandomState(int(d['nobj'].sum()))
        B, S = d['bbox'].shape[:2]
        logits = rs.standard_normal((B, S)).astype(np.float32)
        ps = torch.log_softmax(T(logits), -1).to(DEV)
        pr = T((0.5 * rs.standard_normal((B, S, 4))).astype(np.float32)).to(DEV)
        mode = d['cfg'].SCORES_LOSS
        td = grounding_targets(*_dev(d['bbox'], d['nobj'], d['gt']), d['cfg'])
        tf = {k: v.to(DEV) for k, v in grounding_targets(T(d['bbox']), T(d['nobj']), T(d['gt']), d['cfg']).items()}
        ld = float(vgd_loss(ps, pr, td['scores'], td['scores_mask'], td['bbox'], td['bbox_mask'], scores_loss=mode))
        lf = float(vgd_loss(ps, pr, tf['scores'], tf['scores_mask'], tf['bbox'], tf['bbox_mask'], scores_loss=mode))
        assert np.isfinite(ld) and abs(ld - lf) <= 1e-6 * abs(lf)
