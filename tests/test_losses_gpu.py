"""mmnas_amd.losses on the MI355X (csrc/losses.hip): against the reference's recorded losses (tests/golden/losses.npz,
losses64.npz), against the torch composition run in float64 on the CPU (loss and both gradients, at the project's parity bar
of 1e-3), bit-equal repeats, the reference's NaN on an empty mask, and the losses inside the harness's steps.

When MMNAS_LOSS_STATS names a file, the worst error met against float64 is written there at the end of the module
(profiles/r07_losses_error_stats.json is one such run)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import TOL, load, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy

ERR = {}     # label -> worst relative error against the float64 composition


def _note(label, e):
    print('%s: %.3e' % (label, e))
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_LOSS_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(dict(ERR, worst=max(ERR.values())), f, indent=1, sort_keys=True)


def _scalar_err(a, b):
    a, b = (float(x.detach()) if isinstance(x, torch.Tensor) else float(x) for x in (a, b))
    return abs(a - b) / abs(b)


# ---- the reference's recorded results ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('full64', [False, True], ids=['small', 'B64_production_dimensions'])
def test_vgd_loss_against_the_recorded_reference(full64):
    from mmnas_amd.losses import VgdLoss
    npz = load('losses64.npz' if full64 else 'losses.npz')
    c = cases.losses_cases(full64)[2]
    t = {k: T(v).to(DEV) for k, v in cases.vgd_targets(c, 9204).items()}
    ps, pr = T(npz['vgd|pred_scores']).to(DEV), T(npz['vgd|pred_reg']).to(DEV)
    mod = VgdLoss()
    loss = mod((ps, pr), t)
    ref = npz['vgd|loss_parts']
    parts = mod.parts.cpu().numpy()
    e = max(_scalar_err(parts[0], ref[0]), _scalar_err(parts[1], ref[1]), _scalar_err(loss, ref[2]))
    print('vgd recorded (full64=%s): parts %s loss %.8f reference %s, worst rel err %.3e' % (full64, parts, float(loss), ref, e))
    assert e < TOL
    assert parts[2] == float(t['scores_mask'].sum()) and parts[3] == float(t['bbox_mask'].sum())


@pytest.mark.parametrize('full64', [False, True], ids=['small', 'B160_production_dimensions'])
def test_triplet_bce_against_the_recorded_reference(full64):
    from mmnas_amd.losses import TripletBCELoss
    npz = load('losses64.npz' if full64 else 'losses.npz')
    sp, sc, si = (T(np.ascontiguousarray(a)).to(DEV) for a in npz['itm|scores'])
    loss = TripletBCELoss()(sp, sc, si)
    e = _scalar_err(loss, npz['itm|loss'])
    print('itm recorded (full64=%s): %.8f reference %.8f rel err %.3e' % (full64, float(loss), float(npz['itm|loss']), e))
    assert e < TOL


# ---- torch in float64 ----------------------------------------------------------------------------------------------------------
def _vgd_np(B, S, smask, bmask, seed):
    rs = np.random.RandomState(seed)
    ps = np.log(rs.dirichlet(np.ones(S), B)).astype(np.float32)
    pr = (1.5 * rs.standard_normal((B, S, 4))).astype(np.float32)        # |pred_reg - bbox| on both sides of 1
    sc = rs.dirichlet(np.ones(S), B).astype(np.float32)
    sc[rs.uniform(size=(B, S)) < 0.3] = 0                               # exact zeros: xlogy(0, 0) = 0
    bb = rs.standard_normal((B, S, 4)).astype(np.float32)
    bb[0, 0] = pr[0, 0] + np.array([1.0, -1.0, 0.999999, -1.000001], np.float32)    # at the SmoothL1 switch itself
    sm = (rs.uniform(size=(B, S) if smask == 'full' else (B, 1)) < 0.7).astype(np.float32)
    sm[0] = 1
    bm = (rs.uniform(size=(B, S, 1)) < 0.4).astype(np.float32)
    bm[0, 0] = 1
    if bmask == 'full':
        bm = bm * np.ones((1, 1, 4), np.float32)
    return ps, pr, sc, sm, bb, bm


def _vgd_vs_float64(label, arrs, **kw):
    """arrs: (pred_scores, pred_reg, scores, scores_mask, bbox, bbox_mask) float32 device tensors."""
    from mmnas_amd.harness import vgd_loss
    from mmnas_amd.losses import vgd_loss_fused
    ps, pr = (a.detach().clone().requires_grad_() for a in arrs[:2])
    loss = vgd_loss_fused(ps, pr, *arrs[2:], **kw)
    loss.backward()
    d = [a.detach().double().cpu() for a in arrs]
    d[0].requires_grad_()
    d[1].requires_grad_()
    ref = vgd_loss(*d, **kw)
    ref.backward()
    e = (_scalar_err(loss, ref), rel_err(ps.grad.cpu().numpy(), d[0].grad.numpy()), rel_err(pr.grad.cpu().numpy(), d[1].grad.numpy()))
    _note('vgd %s %s' % (label, sorted(kw.items())), max(e))
    assert np.isfinite(float(ref.detach())) and max(e) < TOL, (label, kw, e)


@pytest.mark.parametrize('mode', ['kld', 'bce'])
@pytest.mark.parametrize('smask', ['full', 'row'])
@pytest.mark.parametrize('bmask', ['full', 'region'])
def test_vgd_loss_against_float64(mode, smask, bmask):
    for B, S, seed in ((5, 7, 1), (3, 37, 2), (64, 100, 3)):
        arrs = [T(a).to(DEV) for a in _vgd_np(B, S, smask, bmask, seed)]
        label = 'B%dxS%d %s/%s' % (B, S, smask, bmask)
        _vgd_vs_float64(label, arrs, scores_loss=mode)
        _vgd_vs_float64(label, arrs, scores_loss=mode, loss_avg=False, lam=1.25)
        _vgd_vs_float64(label, arrs, scores_loss=mode, batch_size=2 * B + 1)


def test_vgd_loss_on_device_targets_against_float64():
    from mmnas_amd.grounding import grounding_targets
    from tests.test_grounding_host import BATCHES
    for k, d in enumerate(BATCHES):
        rs = np.random.RandomState(50 + k)
        B, S = d['bbox'].shape[:2]
        t = grounding_targets(*(T(np.ascontiguousarray(d[n])).to(DEV) for n in ('bbox', 'nobj', 'gt')), d['cfg'])
        assert tuple(t['scores_mask'].shape) == (B, 1) and tuple(t['bbox_mask'].shape) == (B, S, 1)
        if float(t['scores_mask'].sum()) == 0 or float(t['bbox_mask'].sum()) == 0:
            continue
        ps = torch.log_softmax(T(rs.standard_normal((B, S)).astype(np.float32)), -1).to(DEV)
        pr = T(rs.standard_normal((B, S, 4)).astype(np.float32)).to(DEV)
        _vgd_vs_float64('grounding_targets batch %d' % k, [ps, pr, t['scores'], t['scores_mask'], t['bbox'], t['bbox_mask']],
                        scores_loss=d['cfg'].SCORES_LOSS)


def _triplet_vs_float64(label, mine, ref, s, elementwise=False):
    g = [a.detach().clone().requires_grad_() for a in s]
    loss = mine(*g)
    loss.backward()
    d = [a.detach().double().cpu().requires_grad_() for a in s]
    r = ref(*d)
    r.backward()
    e = [_scalar_err(loss, r)] + [rel_err(a.grad.cpu().numpy(), b.grad.numpy()) for a, b in zip(g, d)]
    _note('itm %s' % label, max(e))
    assert max(e) < TOL, (label, e)
    if elementwise:     # every element is formed in float64 and rounded once: far inside 1e-3 of its own value
        for a, b in zip(g, d):
            assert np.allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=TOL, atol=0), label
    return loss


@pytest.mark.parametrize('reduction', ['sum', 'mean'])
def test_triplet_bce_against_float64(reduction):
    from mmnas_amd.harness import BCE_Loss
    from mmnas_amd.losses import TripletBCELoss
    cfg = SimpleNamespace(REDUCTION=reduction)
    for n, seed in ((11, 1), (160, 2), (3000, 3)):
        rs = np.random.RandomState(seed)
        s = [T(rs.uniform(0.001, 0.999, n).astype(np.float32)).to(DEV) for _ in range(3)]
        _triplet_vs_float64('bce %s n=%d' % (reduction, n), TripletBCELoss(cfg), BCE_Loss(cfg), s)
    s = [T(rs.uniform(0.001, 0.999, (4, 5)).astype(np.float32)).to(DEV) for _ in range(3)]       # any equal shape
    _triplet_vs_float64('bce %s [4,5]' % reduction, TripletBCELoss(cfg), BCE_Loss(cfg), s)
    # exactly 0 and 1 and next to them: the -100 clamp of the log and the 1e-12 clamp of the backward's denominator
    below_one = np.nextafter(np.float32(1), np.float32(0))
    edge = np.array([0.0, 1.0, 1e-30, below_one, 1e-13, 0.5, 1.0, 0.0], np.float32)
    s = [T(np.roll(edge, k)).to(DEV) for k in range(3)]
    loss = _triplet_vs_float64('bce %s edge' % reduction, TripletBCELoss(cfg), BCE_Loss(cfg), s, elementwise=True)
    assert np.isfinite(float(loss)) and float(loss) >= (100.0 if reduction == 'sum' else 100.0 / 8)


def test_triplet_margin_against_float64():
    from mmnas_amd.losses import TripletMarginLoss
    from mmnas_amd.utils.itm_loss import Margin_Loss
    rs = np.random.RandomState(8)
    for n in (13, 160):
        s = [T(rs.uniform(0, 1, n).astype(np.float32)).to(DEV) for _ in range(3)]
        cc = 0.2 + s[1].double() - s[0].double()
        assert bool((cc > 1e-3).any()) and bool((cc < -1e-3).any())          # active and inactive hinges
        _triplet_vs_float64('margin n=%d' % n, TripletMarginLoss(), Margin_Loss(), s)
    pos = T(np.array([0.9, 0.9, 0.1, 0.5], np.float32)).to(DEV)              # all inactive / all active / one of each
    negc = T(np.array([0.1, 0.95, 0.6, 0.1], np.float32)).to(DEV)
    negi = T(np.array([0.2, 0.99, 0.7, 0.6], np.float32)).to(DEV)
    _triplet_vs_float64('margin crafted', TripletMarginLoss(), Margin_Loss(), [pos, negc, negi], elementwise=True)


# ---- determinism, empty masks, autograd ----------------------------------------------------------------------------------------
def test_repeated_calls_are_bit_equal():
    from mmnas_amd.losses import TripletBCELoss, TripletMarginLoss, vgd_loss_fused
    arrs = [T(a).to(DEV) for a in _vgd_np(64, 100, 'row', 'region', 9)]
    rs = np.random.RandomState(10)
    s = [T(rs.uniform(0.001, 0.999, 160).astype(np.float32)).to(DEV) for _ in range(3)]
    runs = []
    for _ in range(3):
        out = []
        for mode in ('kld', 'bce'):
            ps, pr = (a.clone().requires_grad_() for a in arrs[:2])
            loss = vgd_loss_fused(ps, pr, *arrs[2:], scores_loss=mode)
            loss.backward()
            out += [loss.detach(), ps.grad, pr.grad]
        for fn in (TripletBCELoss(), TripletMarginLoss()):
            g = [a.clone().requires_grad_() for a in s]
            loss = fn(*g)
            loss.backward()
            out += [loss.detach()] + [a.grad for a in g]
        runs.append(out)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def test_an_empty_mask_gives_the_references_nan():
    from mmnas_amd.harness import vgd_loss
    from mmnas_amd.losses import VgdLoss
    for bmask in ('full', 'region'):
        arrs = [T(a).to(DEV) for a in _vgd_np(4, 9, 'row', bmask, 11)]
        arrs[5] = torch.zeros_like(arrs[5])
        mod = VgdLoss()
        loss = mod((arrs[0], arrs[1]), tuple(arrs[2:]))
        assert bool(torch.isnan(loss)) and bool(torch.isnan(vgd_loss(*arrs)))
        parts = mod.parts.cpu().numpy()
        assert np.isfinite(parts[0]) and np.isnan(parts[1]) and parts[3] == 0


def test_backward_twice_and_upstream_scale():
    from mmnas_amd.losses import TripletBCELoss, vgd_loss_fused
    arrs = [T(a).to(DEV) for a in _vgd_np(5, 7, 'full', 'full', 12)]
    ps, pr = (a.clone().requires_grad_() for a in arrs[:2])
    loss = vgd_loss_fused(ps, pr, *arrs[2:])
    (3.0 * loss).backward(retain_graph=True)               # the upstream scalar is a device value
    g3 = (ps.grad.clone(), pr.grad.clone())
    ps.grad = pr.grad = None
    loss.backward()                                        # a second backward works when the graph was retained ...
    assert rel_err(g3[0].cpu().numpy(), 3 * ps.grad.cpu().numpy()) < 1e-6
    assert rel_err(g3[1].cpu().numpy(), 3 * pr.grad.cpu().numpy()) < 1e-6
    with pytest.raises(RuntimeError, match='second time'):  # ... and raises torch's own clear error when it was not
        loss.backward()
    s = [torch.rand(6, device=DEV).mul_(0.9).add_(0.05).requires_grad_() for _ in range(3)]
    l2 = TripletBCELoss()(*s)
    l2.backward()
    with pytest.raises(RuntimeError, match='second time'):
        l2.backward()
    # gradients flow to the predictions only
    t = arrs[2].clone().requires_grad_()
    ps.grad = None
    vgd_loss_fused(ps, pr, t, *arrs[3:]).backward()
    assert t.grad is None and ps.grad is not None


def test_no_grad_returns_the_value_and_saves_nothing():
    from mmnas_amd.losses import TripletBCELoss, TripletMarginLoss, VgdLoss
    arrs = [T(a).to(DEV) for a in _vgd_np(64, 100, 'row', 'region', 13)]
    ps, pr = (a.clone().requires_grad_() for a in arrs[:2])
    mod = VgdLoss()
    want = mod((ps, pr), tuple(arrs[2:]))
    s = [torch.rand(160, device=DEV).requires_grad_() for _ in range(3)]
    want_t = [fn(*s) for fn in (TripletBCELoss(), TripletMarginLoss())]
    assert want.grad_fn is not None and all(w.grad_fn is not None for w in want_t)
    torch.cuda.synchronize()
    with torch.no_grad():
        before = torch.cuda.memory_allocated()
        got = mod((ps, pr), tuple(arrs[2:]))
        got_t = [fn(*s) for fn in (TripletBCELoss(), TripletMarginLoss())]
        grown = torch.cuda.memory_allocated() - before
    assert got.grad_fn is None and not got.requires_grad and torch.equal(got, want.detach())
    for a, b in zip(got_t, want_t):
        assert a.grad_fn is None and not a.requires_grad and torch.equal(a, b.detach())
    # three scalars and the parts vector stay alive (one 512-byte allocator block each); a saved gradient buffer would be 128 KB
    assert grown <= 4 * 512, grown
    # predictions that require no gradient: the same
    got = mod((ps.detach(), pr.detach()), tuple(arrs[2:]))
    assert got.grad_fn is None and torch.equal(got, want.detach())


# ---- inside the harness --------------------------------------------------------------------------------------------------------
def _build(cls, c):
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def test_train_loop_step_with_vgd_loss_matches_the_torch_composition():
    """TrainLoop(net, loss_fn=VgdLoss(cfg)).step(inputs, grounding_targets(...)) against a copy of the net stepped with
    harness.vgd_loss + backward, the loop's own hyper-parameters: the loss, every parameter's gradient and the parameters after
    one optimizer step agree at the project bar.

    The gradients carry the comparison: Adam's first step moves every element by lr * g / (|g| + 1e-9), i.e. by +-lr whatever
    the size of g, so an element whose gradient is round-off (and a network backward does not repeat bitwise: its embedding
    and split-K products add with atomics) moves by +lr in one run and -lr in the other.  With a raised lr of 1e-3 two runs
    differed by 1.6e-3 of a tensor's largest weight in exactly that way (measured, mhatt.linear_q.weight), which says nothing
    about the loss; gradients are compared against a floor of 1e-3 of the largest gradient norm instead, as the ITM step below
    and tests/test_harness_gpu.py do."""
    from mmnas.model.full_vgd import Net_Full
    from mmnas_amd.grounding import grounding_targets
    from mmnas_amd.harness import TrainLoop, vgd_loss
    from mmnas_amd.losses import VgdLoss
    B, S = 6, 20
    c = cases.net_case('vgd', 'mmnas_vgd', 77, HSIZE=128, B=B, Sx=8, Sy=S)
    c['cfg'].DROPOUT_R = 0.0
    rs = np.random.RandomState(78)
    xy = rs.uniform(0, 300, (B, S, 2))
    bbox = T(np.concatenate((xy, xy + rs.uniform(5, 200, (B, S, 2))), -1).astype(np.float32)).to(DEV)
    gt = bbox[:, 3].double()                               # the referred box is proposal 3 of every sample
    nobj = torch.full((B,), S, dtype=torch.int32, device=DEV)
    cfg = SimpleNamespace(OVERLAP_THRESHOLD=0.5, SCORES_LOSS='kld', BBOX_NORM=False, LOSS_LAMBDA=0.5, LOSS_AVG=True, BATCH_SIZE=B)
    t = grounding_targets(bbox, nobj, gt, cfg)
    assert float(t['scores_mask'].sum()) == B
    inputs = tuple(T(a).to(DEV) for a in c['inputs'])
    res = []
    for fused in (True, False):
        net = _build(Net_Full, c)
        if fused:
            loop = TrainLoop(net, loss_fn=VgdLoss(cfg))
            loss = loop.step(inputs, t)
            assert loop.loss_fn.parts is not None and tuple(loop.loss_fn.parts.shape) == (4,)
        else:
            loop = TrainLoop(net, loss_fn=lambda pred, tg: vgd_loss(pred[0], pred[1], tg['scores'], tg['scores_mask'], tg['bbox'],
                                                                   tg['bbox_mask']))
            loss = loop.step(inputs, t)
        torch.cuda.synchronize()
        res.append((float(loss), {k: p.detach().cpu().numpy().copy() for k, p in net.named_parameters()},
                    {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}))
        loop.reducer.fg.disable_sinks() if hasattr(loop.reducer.fg, 'disable_sinks') else None
    assert _scalar_err(res[0][0], res[1][0]) < TOL
    moved = 0
    for k, v in c['P'].items():
        if k not in res[0][1]:
            continue
        e = rel_err(res[0][1][k], res[1][1][k])
        assert e < TOL, (k, e)
        moved += int(not np.array_equal(res[0][1][k], v))
    assert moved > 0
    top = max(float(np.abs(g).max()) for g in res[1][2].values())
    assert top > 0
    for k, g in res[1][2].items():
        e = float(np.abs(res[0][2][k].astype(np.float64) - g).max()) / max(float(np.abs(g).max()), 1e-3 * top)
        assert e < TOL, (k, e)


def test_itm_triplet_step_with_the_fused_loss():
    from mmnas.model.full_itm import Net_Full
    from mmnas.utils.itm_loss import BCE_Loss
    from mmnas_amd.harness import itm_triplet_step
    from mmnas_amd.losses import TripletBCELoss, fused
    c, neg, _ = cases.losses_cases()
    c['cfg'].DROPOUT_R = 0.0
    pos = tuple(T(a).to(DEV) for a in c['inputs'])
    ng = tuple(T(a).to(DEV) for a in neg['inputs'])
    res = []
    for fn in (fused(BCE_Loss()), BCE_Loss()):
        net = _build(Net_Full, c)
        loss = itm_triplet_step(net, fn, pos, ng)
        res.append((float(loss), {k: float(p.grad.double().norm()) for k, p in net.named_parameters() if p.grad is not None}))
    assert isinstance(fused(BCE_Loss()), TripletBCELoss)
    assert _scalar_err(res[0][0], res[1][0]) < TOL
    assert res[0][1].keys() == res[1][1].keys() and len(res[0][1]) > 10
    top = max(res[1][1].values())
    for k, n in res[1][1].items():
        assert abs(res[0][1][k] - n) <= TOL * max(n, 1e-3 * top), (k, res[0][1][k], n)
