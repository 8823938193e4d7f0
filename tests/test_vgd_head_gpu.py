"""The fused grounding head (ops.grounding_head / ops.GroundingHeadFn, csrc/vgdhead.hip; switch MMNAS_VGD_HEAD) on the GPU:
  * the function against the reference's statements (full_vgd.py:105-114) run in float64 on the CPU -- oracle.layer_norm, the two
    linear layers, log_softmax -- both outputs and all eight gradients for a random upstream gradient on both outputs, judged with
    tests.util.rel_err at the project's 1e-3;
  * repeatability, one output unused, non-contiguous tensors, no_grad, the fallback for an unsupported shape;
  * the whole VGD network at the scripts' dimensions against the reference's own recording (tests/golden/nets_full.npz), judged
    exactly as tests/test_nets_full_gpu.py judges it, with the switch on (one ops.grounding_head call per forward) and off (none);
  * one supernet weight step of hygr_vgd.Net_Search through SearchLoop + VgdLoss with the switch on and off.

A gradient that is mathematically zero has no relative error.  Under log_softmax the scores are shift-invariant, so the gradient of
proj_scores.bias is the sum of d scores = ds - softmax * sum(ds) over the regions, which is zero: the float64 reference returns
its own round-off (1e-16) and any float32 evaluation returns float32 round-off.  The same holds for ln_b's gradient when only the
scores reach the loss (it is proj_scores.weight times that sum).  Those two entries are judged against the scale of the terms of
the sum -- sum |d scores| (times |proj_scores.weight| for ln_b) from the float64 run -- at the same 1e-3, as __graft_entry__.smoke
and tests.util.check_grad_samples floor such denominators; every other entry is judged by rel_err itself.

When MMNAS_VGD_HEAD_STATS names a file, the worst errors met per tensor are written there at the end of the module
(profiles/r10_vgd_head_error_stats.json is one such run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import TOL, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy

# (B, S, F): log_softmax over one score is 0; F below a wave and no multiple of 64; S and F off every tile size; the scripts'
# shape; more than 128 regions at the top of the F range
SHAPES = [(1, 1, 8), (3, 5, 24), (2, 37, 520), (2, 100, 1024), (1, 130, 2048)]
NAMES = ('yf', 'xp', 'ln_a', 'ln_b', 'w_scores', 'b_scores', 'w_reg', 'b_reg')
EPS = 1e-6

ERR = {}     # label -> worst error met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_VGD_HEAD_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


@functools.lru_cache(maxsize=None)
def _inputs(B, S, F):
    """Standard-normal inputs, projection weights scaled by F^-0.5, and the upstream gradients of both outputs (float32, CPU)."""
    g = torch.Generator().manual_seed(1000 * B + 10 * S + F)
    r = lambda *sh: torch.randn(*sh, generator=g)
    t = dict(yf=r(B, S, F), xp=r(B, F), ln_a=1 + 0.1 * r(F), ln_b=0.1 * r(F), w_scores=r(1, F) * F ** -0.5, b_scores=0.1 * r(1),
             w_reg=r(4, F) * F ** -0.5, b_reg=0.1 * r(4))
    return t, r(B, S), r(B, S, 4)


@functools.lru_cache(maxsize=None)
def _reference(B, S, F, logsm, use_scores=True, use_reg=True):
    """The composition in float64 on the CPU: outputs, the eight gradients (name -> array) and the cancellation scales of the two
    sums that vanish under log_softmax.  Computed once per case and shared; the arrays are read-only."""
    from oracle.mmnas_oracle import _linear, layer_norm
    t, gs, gr = _inputs(B, S, F)
    p = {k: v.detach().double().requires_grad_() for k, v in t.items()}
    xy = layer_norm(p['xp'].unsqueeze(1) + p['yf'], p['ln_a'], p['ln_b'], EPS)
    raw = _linear(xy, p['w_scores'], p['b_scores']).squeeze(-1)
    raw.retain_grad()
    scores = torch.log_softmax(raw, dim=-1) if logsm else raw
    reg = _linear(xy, p['w_reg'], p['b_reg'])
    loss = (scores * gs.double()).sum() * float(use_scores) + (reg * gr.double()).sum() * float(use_reg)
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in p.items()}
    ds = raw.grad.abs().sum()
    scale = {'b_scores': float(ds), 'ln_b': float(ds * p['w_scores'].detach().abs().max())}
    out = (scores.detach().numpy(), reg.detach().numpy())
    for a in out + tuple(grads.values()):
        a.setflags(write=False)
    return out, grads, scale


def _gpu(B, S, F, logsm, use_scores=True, use_reg=True, noncontig=False):
    from mmnas_amd import ops
    t, gs, gr = _inputs(B, S, F)
    p = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in t.items()}
    yf = p['yf']
    gs, gr = gs.to(DEV), gr.to(DEV)
    if noncontig:   # yf as a slice of a wider product, the upstream gradients as transposed / strided views
        wide = torch.zeros(B, S, F + 8, device=DEV)
        wide[..., 4:F + 4] = t['yf'].to(DEV)
        p['yf'] = wide.requires_grad_()
        yf = p['yf'][..., 4:F + 4]
        gs = gs.t().contiguous().t()
        gr = torch.stack([gr, gr], -1)[..., 0]
        assert not yf.is_contiguous() and not gr.is_contiguous() and (S == 1 or B == 1 or not gs.is_contiguous())
    scores, reg = ops.grounding_head(yf, p['xp'], p['ln_a'], p['ln_b'], EPS, p['w_scores'], p['b_scores'], p['w_reg'], p['b_reg'],
                                     log_softmax=logsm)
    outs, gout = [], []
    if use_scores:
        outs.append(scores); gout.append(gs)
    if use_reg:
        outs.append(reg); gout.append(gr)
    torch.autograd.backward(outs, gout)
    torch.cuda.synchronize()
    # (the composition behind the fallback leaves an unused parameter without a gradient: that is a zero)
    grads = {k: (np.zeros(tuple(v.shape), np.float32) if v.grad is None else v.grad.cpu().numpy()) for k, v in p.items()}
    if noncontig:
        assert not np.any(grads['yf'][..., :4]) and not np.any(grads['yf'][..., F + 4:])
        grads['yf'] = grads['yf'][..., 4:F + 4]
    return (scores.detach().cpu().numpy(), reg.detach().cpu().numpy()), grads


def _judge(label, got, ref, logsm, use_reg=True, outputs=(True, True)):
    (sc, rg), grads = got
    (rsc, rrg), rgrads, scale = ref
    errs = {}
    if outputs[0]:
        errs['scores'] = rel_err(sc, rsc)
    if outputs[1]:
        errs['reg'] = rel_err(rg, rrg)
    for k in NAMES:
        zero_sum = logsm and (k == 'b_scores' or (k == 'ln_b' and not use_reg))     # (module docstring)
        if zero_sum:
            errs['d' + k] = float(np.abs(grads[k] - rgrads[k]).max()) / max(scale[k], 1e-30) if scale[k] > 0 else float(np.abs(grads[k]).max())
        else:
            errs['d' + k] = rel_err(grads[k], rgrads[k])
    for k, e in errs.items():
        print('%s %s %.3e' % (label, k, e))
        _note(k, e)
    bad = {k: e for k, e in errs.items() if not e <= TOL}
    assert not bad, (label, bad)


# ---------------------------------------------------------------------------------------------------------------------
# the function
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('logsm', [True, False], ids=['log_softmax', 'raw_scores'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'B%d_S%d_F%d' % s)
def test_grounding_head_vs_float64_composition(shape, logsm):
    from mmnas_amd import _lib as L
    assert L.lib().mmnas_vgd_head_supported(shape[1], shape[2])
    _judge('%s logsm=%d' % (shape, logsm), _gpu(*shape, logsm), _reference(*shape, logsm), logsm)


def test_log_softmax_over_one_region_is_exactly_zero():
    (sc, _), grads = _gpu(1, 1, 8, True)
    assert sc.shape == (1, 1) and sc[0, 0] == 0.0
    assert not np.any(grads['w_scores']) and not np.any(grads['b_scores'])


@pytest.mark.parametrize('shape', [(2, 37, 520), (2, 100, 1024)], ids=lambda s: 'B%d_S%d_F%d' % s)
def test_two_calls_give_the_same_bits(shape):
    a, b = _gpu(*shape, True), _gpu(*shape, True)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    for k in NAMES:
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize('logsm', [True, False], ids=['log_softmax', 'raw_scores'])
@pytest.mark.parametrize('used', ['scores', 'reg'])
def test_only_one_output_reaches_the_loss(used, logsm):
    shape = (2, 37, 520)
    us, ur = used == 'scores', used == 'reg'
    got = _gpu(*shape, logsm, use_scores=us, use_reg=ur)
    _judge('%s only %s logsm=%d' % (shape, used, logsm), got, _reference(*shape, logsm, us, ur), logsm, use_reg=ur)
    if ur:   # nothing flows through the scores: their projection's gradients are exactly zero
        assert not np.any(got[1]['w_scores']) and not np.any(got[1]['b_scores'])


def test_non_contiguous_input_and_upstream_gradients():
    shape = (3, 5, 24)
    _judge('%s non-contiguous' % (shape,), _gpu(*shape, True, noncontig=True), _reference(*shape, True), True)
    shape = (2, 37, 520)
    got = _gpu(*shape, True, noncontig=True)
    _judge('%s non-contiguous' % (shape,), got, _reference(*shape, True), True)
    plain = _gpu(*shape, True)
    assert all(np.array_equal(x, y) for x, y in zip(got[0], plain[0]))       # the same numbers reach the kernel
    for k in NAMES:
        assert np.array_equal(got[1][k], plain[1][k]), k


@pytest.mark.parametrize('logsm', [True, False], ids=['log_softmax', 'raw_scores'])
def test_no_grad_outputs_equal_grad_mode_outputs_bitwise(logsm, monkeypatch):
    from mmnas_amd import _lib as L
    from mmnas_amd import ops
    shape = (2, 37, 520)
    t, _, _ = _inputs(*shape)
    p = {k: v.detach().clone().to(DEV).requires_grad_() for k, v in t.items()}
    args = (p['yf'], p['xp'], p['ln_a'], p['ln_b'], EPS, p['w_scores'], p['b_scores'], p['w_reg'], p['b_reg'])
    s1, r1 = ops.grounding_head(*args, log_softmax=logsm)
    assert s1.requires_grad and r1.requires_grad
    saved = []
    lib = L.lib()

    class Spy:      # the statistics pointers of the forward call: null when nothing is saved
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != 'mmnas_vgd_head_fwd':
                return fn
            return lambda *a: (saved.append((a[10], a[11])), fn(*a))[1]
    monkeypatch.setattr(L, '_lib', Spy())
    with torch.no_grad():
        s0, r0 = ops.grounding_head(*args, log_softmax=logsm)
    monkeypatch.undo()
    assert saved == [(None, None)]
    assert not s0.requires_grad and s0.grad_fn is None and r0.grad_fn is None
    assert torch.equal(s0, s1.detach()) and torch.equal(r0, r1.detach())


def test_unsupported_shape_takes_the_composition_and_meets_the_bar(monkeypatch):
    from mmnas_amd import _lib as L
    from mmnas_amd import ops
    shape = (2, 7, 1001)
    assert not L.lib().mmnas_vgd_head_supported(shape[1], shape[2])
    calls = []
    orig = ops.GroundingHeadFn.apply
    monkeypatch.setattr(ops.GroundingHeadFn, 'apply', lambda *a: (calls.append(1), orig(*a))[1])
    _judge('%s fallback' % (shape,), _gpu(*shape, True), _reference(*shape, True), True)
    assert not calls
    _gpu(3, 5, 24, True)
    assert calls == [1]          # ... and a supported shape does go through the kernels


# ---------------------------------------------------------------------------------------------------------------------
# whole networks
# ---------------------------------------------------------------------------------------------------------------------
VGD_FULL = ('full', 'vgd', 'mmnas_vgd', 512, 2, 15, 100, None)


@pytest.mark.parametrize('on,route', [(True, 'per_operator'), (True, 'chain'), (False, 'per_operator')],
                         ids=['on-per_operator', 'on-chain', 'off-per_operator'])
def test_vgd_network_at_the_scripts_dimensions_vs_reference(on, route, monkeypatch):
    """tests/golden/nets_full.npz's VGD case through tests/test_nets_full_gpu.py's own _run / _check (golden outputs, loss, every
    gradient norm, check_grad_samples), with the head fused (under plain autograd and behind the flat gradient buffer) and not."""
    from mmnas_amd import ops
    from tests.test_nets_full_gpu import _check, _run
    assert VGD_FULL in cases.FULL_CASES
    calls = []
    orig = ops.grounding_head
    monkeypatch.setattr(ops, 'grounding_head', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    prev = ops.set_vgd_head(on)
    try:
        res = _run(VGD_FULL, route, monkeypatch)
    finally:
        ops.set_vgd_head(prev)
    assert len(calls) == (1 if on else 0)        # one forward: exactly one call, or none
    _check(VGD_FULL, route, res)


def test_supernet_weight_step_with_the_fused_head_equals_the_composition():
    from mmnas.model.hygr_vgd import Net_Search
    from mmnas_amd import ops
    from mmnas_amd.harness import SearchLoop
    from mmnas_amd.losses import VgdLoss
    c = cases.net_case('vgd', None, 4711, search=True, B=3, Sx=6, Sy=9)
    c['cfg'].DROPOUT_R = 0.0
    plan = cases.search_plan(np.random.RandomState(5), None)
    flat = plan['enc'] + plan['dec']
    inp = tuple(T(a).to(DEV) for a in c['inputs'])
    tgt = {k: T(v).to(DEV) for k, v in cases.vgd_targets(c, 4712).items()}
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    calls = []
    orig = ops.GroundingHeadFn.apply
    res = []
    prev = ops.vgd_head_enabled()
    try:
        ops.GroundingHeadFn.apply = lambda *a: (calls.append(1), orig(*a))[1]
        for on in (True, False):
            torch.manual_seed(7)
            ops.manual_seed(7)
            net = Net_Search(c['cfg'], init)
            net.load_state_dict({k: T(v) for k, v in c['P'].items()})
            net = net.to(DEV).train()
            loop = SearchLoop(net, loss_fn=VgdLoss(c['cfg']))
            ops.set_vgd_head(on)
            try:
                loss = loop.weight_step(inp, tgt, optimize=False, plan=flat)
                torch.cuda.synchronize()
                res.append((float(loss.detach()), loop.reducer.fg.flat.detach().cpu().numpy().copy()))
            finally:
                loop.reducer.fg.disable_sinks()
            assert len(calls) == 1       # the first (fused) step made the one call, the second none
    finally:
        ops.GroundingHeadFn.apply = orig
        ops.set_vgd_head(prev)
    (l_on, g_on), (l_off, g_off) = res
    assert np.isfinite(l_on) and np.isfinite(g_on).all() and np.abs(g_off).max() > 0
    e_loss, e_grad = abs(l_on - l_off) / abs(l_off), rel_err(g_on, g_off)
    print('supernet weight step: loss %.3e flat gradient %.3e' % (e_loss, e_grad))
    _note('supernet_loss', e_loss)
    _note('supernet_flat_grad', e_grad)
    assert e_loss <= TOL and e_grad <= TOL
