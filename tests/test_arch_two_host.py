"""Host side of the fused ALPHA_BINARY_MODE 'two' architecture update (no GPU):
  * ops.alpha_two_step on CPU tensors -- the torch restatement of mmnas_alpha_two_step -- replays tests/golden/arch_two.npz
    (the reference's MixedOp statements + torch Adam, make_golden_arch_two.py) and the two 'mx|two|...' cases of mixed.npz;
  * harness.ArchAdam(mode='two') on a CPU supernet in lockstep with the per-module statements around torch Adam;
  * checkpoints travel between ArchAdam(mode='two') and torch.optim.Adam in both directions;
  * the argument errors of the Python layer and of the C entry (which returns before any launch).
The bound 1e-5 (tests/util.rel_err) is the project's bar for alphas between two paths (tests/test_harness_gpu.py)."""
import ctypes

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import load, rel_err

T = torch.from_numpy
TOL = 1e-5
SETTINGS = ((0.1, (0.0, 0.999), 0.0), (0.1, (0.5, 0.999), 1e-3), (1.0, (0.0, 0.999), 0.0))
MIN_GAP = 0.1


def fin(x):
    """Padding columns hold -inf on both sides: compare the rest."""
    x = np.asarray(x, np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def replay_arch_two(npz, s, dev='cpu'):
    """Feed arch_two.npz's setting `s` step by step through ops.alpha_two_step on `dev`; returns the worst error per
    quantity after asserting each against the recording."""
    from mmnas_amd import ops
    lr, b1, b2, wd = (float(x) for x in npz['s%d|hyper' % s])
    assert (lr, (b1, b2), wd) == SETTINGS[s]
    eps = float(npz['eps'])
    widths = npz['widths']
    prob = T(npz['alpha0'].copy()).to(dev)
    m, v, pg = torch.zeros_like(prob), torch.zeros_like(prob), torch.full_like(prob, 7.0)     # (prob_grad is overwritten)
    pad = np.arange(prob.shape[1])[None, :] >= widths[:, None]
    worst = {}
    for t in range(npz['pairs'].shape[0]):
        pairs = [tuple(int(x) for x in p) for p in npz['pairs'][t]]
        for k, (i, j) in enumerate(pairs):
            assert abs(float(npz['gate_grad'][t, k, i]) - float(npz['gate_grad'][t, k, j])) >= MIN_GAP
        ops.alpha_two_step(prob, T(npz['gate_grad'][t].copy()).to(dev), m, v, pg, pairs, lr, (b1, b2), eps, t + 1, weight_decay=wd)
        got = dict(prob_grad=pg, alpha=prob, exp_avg=m, exp_avg_sq=v)
        for name, ten in got.items():
            ref = npz['s%d|%s' % (s, name)][t]
            e = rel_err(fin(ten.cpu().numpy()), fin(ref))
            worst[name] = max(worst.get(name, 0.0), e)
            assert e < TOL, (s, t, name, e)
        a = prob.cpu().numpy()
        assert np.all(np.isneginf(a[pad])) and np.all(np.isfinite(a[~pad])), 'padding columns stay -inf, the others finite'
        assert not m.cpu().numpy()[pad].any() and not v.cpu().numpy()[pad].any()
    return worst


@pytest.mark.parametrize('s', [0, 1, 2])
def test_cpu_restatement_replays_the_reference_recording(s):
    npz = load('arch_two.npz')
    assert sorted(set(int(w) for w in npz['widths'])) == [2, 4, 5] and npz['pairs'].shape[0] == 6
    print('setting', s, 'worst errors', replay_arch_two(npz, s))


def test_cpu_restatement_replays_the_two_mode_cases_of_mixed_npz():
    """prob_grad against the recording; the rescale half fed the recording's stand-in optimizer step (alpha_stepped)."""
    from mmnas_amd import ops
    npz = load('mixed.npz')
    for kind in ('enc_safe', 'dec_safe'):
        tag = 'mx|two|%s|' % kind
        c = cases.mixed_case('two', kind, int(npz[tag + 'seed']))
        idx = torch.tensor([[c['act'][0], c['inact'][0]]])
        old = T(npz[tag + 'alpha_old'].copy())[None]
        grad = ops.alpha_two_pair_grad(old, T(npz[tag + 'gate_grad'].copy())[None], idx)
        assert rel_err(grad[0].numpy(), npz[tag + 'prob_grad']) < TOL
        stepped = T(npz[tag + 'alpha_stepped'].copy())[None]
        ops.alpha_two_rescale(stepped, old.gather(1, idx), idx)
        assert rel_err(stepped[0].numpy(), npz[tag + 'alpha_rescaled']) < TOL


def _build(c):
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.train()


def _plan_list(plan):
    return plan['enc'] + plan['dec']


def _gate_grads(rs, mods, plan):
    """One gate-gradient vector per node with |g_i - g_j| >= MIN_GAP on its pair (beta1 = 0: Adam moves by +-lr whatever the
    gradient's size, so a pair gradient near zero would leave the sign to float32 rounding on either side)."""
    out = []
    for m, (act, inact) in zip(mods, plan):
        while True:
            g = rs.uniform(-1.0, 1.0, m.n_choices).astype(np.float32)
            if abs(float(g[act[0]]) - float(g[inact[0]])) >= MIN_GAP:
                break
        out.append(g)
    return out


def _torch_update(net, opt, plan, grads):
    """The reference's statements (search_vqa.py:330-335) through the per-module path."""
    from mmnas.model.mixed import MixedOp
    net.set_sampled(plan)
    MixedOp.MODE = 'two'
    try:
        for m, g in zip(net.redundant_modules, grads):
            m.alpha_gate.grad = T(g.copy())
            m.alpha_prob.grad = None
        net.set_arch_param_grad()
        opt.step()
        net.rescale_updated_arch_param()
    finally:
        MixedOp.MODE = None


def _fused_update(net, opt, plan, grads):
    net.set_sampled(plan)
    for m, g in zip(net.redundant_modules, grads):
        m.alpha_gate.grad = T(g.copy())          # outside the flat block: ArchAdam copies it in
    opt.step()


def _alphas(net):
    return net._flat_alphas()[0].detach().numpy().copy()


def _grads(net):
    w = net._flat_alphas()[0].shape[1]
    return np.stack([np.pad(m.alpha_prob.grad.numpy(), (0, w - m.n_choices)) for m in net.redundant_modules])


@pytest.mark.parametrize('betas,wd', [((0.0, 0.999), 0.0), ((0.5, 0.999), 0.0), ((0.5, 0.999), 1e-3)],
                         ids=['scripts_setting', 'beta1_0.5', 'beta1_0.5_wd'])
def test_arch_adam_mode_two_in_lockstep_with_the_per_module_statements(betas, wd):
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(12)
    fused, ref = _build(c), _build(c)
    fopt = ArchAdam(fused, 0.1, betas, weight_decay=wd, mode='two')
    ref._flat_alphas()
    ropt = torch.optim.Adam(list(ref.alpha_prob_parameters()), 0.1, betas=betas, weight_decay=wd)
    mods = fused.redundant_modules
    width = fused._flat_alphas()[0].shape[1]
    pad = np.array([[j >= m.n_choices for j in range(width)] for m in mods])
    versions = [m.alpha_version for m in mods]
    seen = np.zeros(pad.shape, bool)           # columns that were in a sampled pair at an earlier step
    moved_outside = 0
    for step in range(3):
        plan = _plan_list(cases.search_plan(rs, 'two'))
        grads = _gate_grads(rs, mods, plan)
        before = _alphas(fused)
        _torch_update(ref, ropt, plan, grads)
        _fused_update(fused, fopt, plan, grads)
        a, b = _alphas(fused), _alphas(ref)
        assert rel_err(fin(a), fin(b)) < TOL, (step, 'alpha')
        assert rel_err(_grads(fused), _grads(ref)) < TOL, (step, 'alpha_prob.grad')
        assert np.all(np.isneginf(a[pad])) and np.all(np.isfinite(a[~pad]))
        in_pair = np.zeros(pad.shape, bool)
        for i, (act, inact) in enumerate(plan):
            in_pair[i, act[0]] = in_pair[i, inact[0]] = True
        outside = ~pad & ~in_pair
        if betas[0] == 0.0 and wd == 0.0:
            assert np.array_equal(a[outside], before[outside]), 'zero gradient, no momentum, no decay: no motion'
        elif wd == 0.0:
            assert np.array_equal(a[outside & ~seen], before[outside & ~seen]), 'never in a pair: no moments yet'
            stale = outside & seen
            assert np.all(a[stale] != before[stale]), 'the momentum of an earlier pair keeps moving its columns'
            moved_outside += int(stale.sum())
        seen |= in_pair
        for i, m in enumerate(mods):
            assert m.alpha_prob.grad.data_ptr() == fused._flat_grads[1][i].data_ptr()     # a row of the gradient block
    assert fopt.steps == 3 and [m.alpha_version for m in mods] == [x + 3 for x in versions]
    if betas[0] and wd == 0.0:
        assert moved_outside > 0


def test_checkpoints_travel_between_arch_adam_mode_two_and_torch_adam():
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(13)
    betas, wd = (0.5, 0.999), 1e-3
    fused, ref = _build(c), _build(c)
    fopt = ArchAdam(fused, 0.1, betas, weight_decay=wd, mode='two')
    ref._flat_alphas()
    ropt = torch.optim.Adam(list(ref.alpha_prob_parameters()), 0.1, betas=betas, weight_decay=wd)
    for _ in range(2):
        plan = _plan_list(cases.search_plan(rs, 'two'))
        grads = _gate_grads(rs, fused.redundant_modules, plan)
        _torch_update(ref, ropt, plan, grads)
        _fused_update(fused, fopt, plan, grads)
    sd_fused, sd_torch = fopt.state_dict(), ropt.state_dict()
    assert sd_fused['param_groups'][0]['weight_decay'] == wd == sd_torch['param_groups'][0]['weight_decay']
    assert sorted(sd_fused['state']) == sorted(sd_torch['state']) == list(range(30))
    for k, st in sd_torch['state'].items():
        assert float(st['step']) == float(sd_fused['state'][k]['step']) == 2.0
        for name in ('exp_avg', 'exp_avg_sq'):
            assert rel_err(sd_fused['state'][k][name].numpy(), st[name].numpy()) < TOL, (k, name)
    # the 'full' optimizer reads the same file (state_dict / load_state_dict do not depend on the mode)
    full = ArchAdam(_build(c))
    full.load_state_dict(sd_fused)
    assert full.steps == 2 and full.mode == 'full' and torch.equal(full.m, fopt.m) and torch.equal(full.v, fopt.v)
    # each side resumes from the OTHER side's file (fresh optimizers with other settings: the file's are taken) and the
    # two go on in lockstep
    fused2, ref2 = _build(c), _build(c)
    for net, src in ((fused2, ref), (ref2, fused)):
        net._flat_alphas()[0].copy_(src._flat_alphas()[0])
    fopt2 = ArchAdam(fused2, 0.7, (0.9, 0.9), mode='two')
    fopt2.load_state_dict(sd_torch)
    assert (fopt2.lr, tuple(fopt2.betas), fopt2.weight_decay, fopt2.steps, fopt2.mode) == (0.1, betas, wd, 2, 'two')
    ropt2 = torch.optim.Adam(list(ref2.alpha_prob_parameters()), 0.7)
    ropt2.load_state_dict(sd_fused)
    assert ropt2.param_groups[0]['weight_decay'] == wd and ropt2.param_groups[0]['lr'] == 0.1
    plan = _plan_list(cases.search_plan(rs, 'two'))
    grads = _gate_grads(rs, fused.redundant_modules, plan)
    _torch_update(ref2, ropt2, plan, grads)
    _fused_update(fused2, fopt2, plan, grads)
    assert rel_err(fin(_alphas(fused2)), fin(_alphas(ref2))) < TOL
    assert float(ropt2.state_dict()['state'][0]['step']) == 3.0 == float(fopt2.state_dict()['state'][0]['step'])


def _blocks(rows, width=4):
    prob = torch.zeros(rows, width)
    return prob, torch.ones(rows, width), torch.zeros(rows, width), torch.zeros(rows, width), torch.zeros(rows, width)


def test_python_layer_argument_errors():
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam
    hyper = (0.1, (0.0, 0.999), 1e-8)
    prob, gg, m, v, pg = _blocks(3)
    prob[0, 2:] = float('-inf')
    good = [(0, 1), (1, 3), (2, 0)]
    for pairs, step, what in (([(0, 0), (1, 3), (2, 0)], 1, 'i == j'), ([(0, 1), (1, 4), (2, 0)], 1, 'index >= width'),
                              ([(0, 1), (-1, 3), (2, 0)], 1, 'negative index'), ([(0, 2), (1, 3), (2, 0)], 1, 'padding column'),
                              (good, 0, 'step < 1'), (good[:2], 1, 'a pair missing')):
        before = prob.clone()
        with pytest.raises(ValueError):
            ops.alpha_two_step(prob, gg, m, v, pg, pairs, *hyper, step)
        assert torch.equal(prob, before) and not m.any() and not v.any(), what       # nothing was written
    ops.alpha_two_step(prob, gg, m, v, None, good, *hyper, 1)                        # prob_grad is optional
    big = _blocks(129)
    with pytest.raises(ValueError):
        ops.alpha_two_step(*big, [(0, 1)] * 129, *hyper, 1)
    ops.alpha_two_step(*_blocks(128), [(0, 1)] * 128, *hyper, 1)                     # the limit itself
    ops.alpha_two_step(*_blocks(0), [], *hyper, 1)                                   # no rows: nothing to do
    # ArchAdam: a node without a sampled pair, a pair outside the node's own candidates
    c = cases.net_case('vqa', None, 4343, search=True)
    net = _build(c)
    with pytest.raises(ValueError):
        ArchAdam(net, mode='three')
    opt = ArchAdam(net, mode='two')
    assert net.redundant_modules[0].active_index is None
    with pytest.raises(ValueError, match='no sampled pair'):
        opt.step()
    plan = _plan_list(cases.search_plan(np.random.RandomState(3), 'two'))
    net.set_sampled(plan)
    mods = net.redundant_modules
    assert mods[0].n_choices == 2
    alphas = _alphas(net)
    for act, inact in (([0], [2]), ([1], [1]), ([0], [])):
        mods[0].active_index, mods[0].inactive_index = act, inact
        with pytest.raises(ValueError):
            opt.step()
    plan_full = _plan_list(cases.search_plan(np.random.RandomState(3), 'full'))
    net.set_sampled(plan_full)               # a 'full' sample: the wide nodes hold three inactive candidates, no pair
    with pytest.raises(ValueError, match='no sampled pair'):
        opt.step()
    assert opt.steps == 0 and np.array_equal(fin(_alphas(net)), fin(alphas))


def test_c_entry_rejects_bad_arguments_before_any_launch():
    """Host buffers stand in for the device pointers: every call here must return from the entry's own checks (a launch
    without a device would come back as MMNAS_E_LAUNCH = -3, never as -1 / -2 / 0)."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    assert 'mmnas_alpha_two_step' in L.SYMBOLS and len(L.SYMBOLS['mmnas_alpha_two_step'][1]) == 15
    assert lib.mmnas_abi_version() == 1
    buf = [(ctypes.c_float * (129 * 4))() for _ in range(5)]
    p = [ctypes.cast(b, ctypes.c_void_p).value for b in buf]

    def call(rows, width, pairs, step):
        arr = (ctypes.c_int * max(1, len(pairs)))(*pairs)
        return lib.mmnas_alpha_two_step(p[0], p[1], p[2], p[3], p[4], rows, width, arr, 0.1, 0.0, 0.999, 1e-8, 0.0, step, None)

    assert call(129, 4, [0, 1] * 129, 1) == -1 and b'rows=129' in lib.mmnas_last_error()      # MMNAS_E_SHAPE
    assert call(2, 4, [0, 1, 2, 2], 1) == -2 and b'row 1' in lib.mmnas_last_error()           # i == j
    assert call(2, 4, [0, 4, 1, 2], 1) == -2                                                   # index == width
    assert call(2, 4, [0, 1, -1, 2], 1) == -2
    assert call(2, 4, [0, 1, 1, 2], 0) == -2                                                   # step < 1
    assert call(0, 4, [], 1) == 0                                                              # rows == 0: OK
    assert not any(any(b) for b in buf)
