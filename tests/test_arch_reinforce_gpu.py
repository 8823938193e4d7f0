"""The REINFORCE architecture update on the GPU (mmnas_alpha_reinforce_step) and SearchLoop(arch_mode='reinforce'):
  * the kernel against the float64 torch restatement on the CPU over every case of tests/arch_reinforce_cases.py (whose inputs
    are conditioned: tests/test_arch_reinforce_host.py) on prob, m, v, prob_grad, stats and baseline; padding columns;
  * repeatability bit for bit, guard bands around every buffer, prob_grad / stats / cost optional, the err flag;
  * the loop on the tiny Net_Search of tests/test_arch_two_gpu.py: against the restatement fed the same plans and the
    qualities the loop reports; no weight, gradient or flag moves; weight steps around an arch step are undisturbed.

Bound: 1e-5 (tests/util.rel_err), the project's bar for alphas between two paths.

When MMNAS_ARCH_REINFORCE_STATS names a file, the worst distance per quantity is written there at the end of the module
(profiles/r17_arch_reinforce_error_stats.json is one such run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import arch_reinforce_cases as RC
from tests.golden import cases
from tests.guardband import Arena
from tests.test_arch_two_host import SETTINGS, TOL, fin
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy
NAMES = RC.NAMES + ('baseline',)
assert TOL == 1e-5

ERR = {}     # label -> worst distance met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_ARCH_REINFORCE_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('key', RC.combos(), ids=['%dx%d-M%d-%s' % k for k in RC.combos()])
def test_kernel_vs_the_float64_restatement(key):
    c = RC.case(*key)
    pad = ~c['live']
    for s in range(len(SETTINGS)):
        got = RC.replay(c, s, torch.float32, DEV)
        ref = RC.reference(*key, s)
        for t, (g, r) in enumerate(zip(got, ref)):
            for name in NAMES:
                e = rel_err(fin(g[name]), fin(r[name]))
                _note('kernel|%s' % name, e)
                print('%r setting %d step %d %s: %.3g' % (key, s, t + 1, name, e))
                assert e < TOL, (key, s, t, name, e)
            assert g['err'] == 0
            assert np.all(np.isneginf(g['prob'][pad])) and np.all(np.isfinite(g['prob'][~pad])), 'padding columns stay -inf'
            assert not g['m'][pad].any() and not g['v'][pad].any(), 'padding moments stay untouched'
            assert not g['prob_grad'][pad].any()


@pytest.mark.parametrize('key', [(300, 3, 4, 'mul'), (128, 5, 16, 'add'), (65, 4, 4, 'none')], ids=str)
def test_same_inputs_give_the_same_bits(key):
    c = RC.case(*key)
    a, b = RC.replay(c, 1, torch.float32, DEV), RC.replay(c, 1, torch.float32, DEV)
    for x, y in zip(a, b):
        for name in NAMES:
            assert np.array_equal(x[name], y[name]), name


def _arena_call(c, t, with_pg=True, with_stats=True, with_cost=True, state=None, quality=None):
    """One update inside a guard-band arena: quality and cost are inputs, prob / m / v / baseline / err are read and written,
    prob_grad and stats are written whole (the arena pre-fills them with a NaN pattern)."""
    from mmnas_amd import ops
    rows, width, M = c['rows'], c['width'], c['M']
    form, w = RC.REWARDS[c['reward']]
    ar = Arena(DEV, capacity=4 << 20)
    zero = np.zeros((rows, width), np.float32)
    prob = ar.inout(c['a0'] if state is None else state[0], name='prob')[1]
    m = ar.inout(zero if state is None else state[1], name='m')[1]
    v = ar.inout(zero if state is None else state[2], name='v')[1]
    base = ar.inout(np.zeros(2, np.float32) if state is None else state[3], name='baseline')[1]
    err = ar.inout(np.zeros(1, np.int32), name='err')[1]
    q = ar.inp(c['quality'][t] if quality is None else quality, name='quality')[1]
    cost = ar.inp(c['cost'], name='cost')[1] if with_cost and form else None
    pg = ar.out((rows, width), name='prob_grad')[1] if with_pg else None
    st = ar.out(M + 3, name='stats')[1] if with_stats else None
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][t], q, base, 0.1, (0.5, 0.999), RC.EPS, t + 1, weight_decay=1e-3, cost=cost,
                             cost_weight=w, cost_ref=c['cost_ref'], reward_form=form or 'mul', baseline_decay=RC.DECAY, stats=st,
                             err=err, n_choices=c['n'])
    return ar, [x.clone() for x in (prob, m, v, base)], pg, st, err


@pytest.mark.parametrize('key', [(300, 3, 4, 'mul'), (65, 4, 4, 'add'), (128, 5, 16, 'mul'), (1, 2, 1, 'add')], ids=str)
def test_only_the_outputs_are_written_and_prob_grad_stats_and_cost_are_optional(key):
    c = RC.case(*key)
    ar, state, pg, st, err = _arena_call(c, 0)
    ar.check()
    assert int(err) == 0 and float(state[3][1]) == 1.0 and float(st[c['M']]) == float(state[3][0])
    for with_pg, with_stats in ((False, True), (True, False), (False, False)):
        ar, other, _, _, _ = _arena_call(c, 0, with_pg, with_stats)
        ar.check()
        for x, y in zip(state, other):
            assert torch.equal(x, y), (with_pg, with_stats)
    ar, nocost, _, st2, _ = _arena_call(c, 0, with_cost=False)                      # cost=None: R_i = Q_i
    ar.check()
    assert np.array_equal(st2[:c['M']].cpu().numpy(), c['quality'][0])
    ar, _, _, _, _ = _arena_call(c, 1, state=[x.cpu().numpy() for x in state])      # with moments and a baseline in place
    ar.check()


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_a_non_finite_quality_sets_err_and_leaves_the_device_state_alone(bad):
    c = RC.case(65, 4, 4, 'mul')
    _, state, _, _, _ = _arena_call(c, 0)
    q = c['quality'][1].copy()
    q[3] = bad
    ar, after, pg, st, err = _arena_call(c, 1, state=[x.cpu().numpy() for x in state], quality=q)
    torch.cuda.synchronize()
    assert int(err) == 1
    for x, y in zip(state, after):
        assert np.array_equal(x.cpu().numpy().view(np.int32), y.cpu().numpy().view(np.int32))
    pat = np.int32(np.array([0x7FC5A17E], np.uint32).view(np.int32)[0])
    assert (pg.cpu().numpy().view(np.int32) == pat).all() and (st.cpu().numpy().view(np.int32) == pat).all(), 'outputs stay unwritten'
    for r in ar.recs:                           # the arena's own verdict, but for "every output was written"
        if r.kind == 'out':
            r.written = None
    ar.check()


# ---- the loop ---------------------------------------------------------------------------------------------------------------------
def _build(c):
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def _plan_lists(rs, M, k):
    out = []
    for _ in range(k):
        step = []
        for _ in range(M):
            p = cases.search_plan(rs, None)
            step.append(p['enc'] + p['dec'])
        out.append(step)
    return out


@pytest.fixture(scope='module')
def setup():
    c = cases.net_case('vqa', None, 4343, search=True)
    inp = tuple(T(a).to(DEV) for a in c['inputs'])
    tgt = T(c['target']).to(DEV)
    return c, inp, tgt


@pytest.mark.parametrize('reward', ['negloss', 'soft'])
def test_search_loop_against_the_restatement_and_nothing_but_the_alphas_moves(setup, reward):
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import answering, ops
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c, inp, tgt = setup
    M = 3
    if reward == 'soft':       # (the case's targets are sparse and an untrained net scores 0 on them: dense scores tell samples apart)
        tgt = torch.rand(tgt.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    kw = dict(reward=answering.SoftAccuracyReward()) if reward == 'soft' else dict(reward_form='add')
    loop = SearchLoop(_build(c), arch_mode='reinforce', reinforce_samples=M, baseline_decay=0.9, **kw)
    net, opt = loop.net, loop.alpha_optim
    try:
        assert isinstance(opt, ArchAdam) and opt.mode == 'reinforce' and opt.quality.is_cuda and opt.quality.shape == (M,)
        plans = _plan_lists(np.random.RandomState(8), M, 3)
        n = [m.n_choices for m in net.redundant_modules]
        prob = net._flat_alphas()[0].detach().cpu().double()
        m64, v64, pg64 = torch.zeros_like(prob), torch.zeros_like(prob), torch.zeros_like(prob)
        base64, err64 = torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
        loop.weight_step(inp, tgt, optimize=False, plan=plans[0][0])      # gradients in place: the arch steps must not touch them
        torch.cuda.synchronize()
        weights = [p.detach().clone() for p in net.net_parameters()]
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters() if 'alpha_prob' not in k}
        assert sum(g is not None for g in grads.values()) > 10
        flat = loop.reducer.fg.flat.detach().clone()
        net.imgfeat_linear.eval()                                          # a flag that differs from its neighbours'
        flags = [m.training for m in net.modules()]
        for k, step_plans in enumerate(plans):
            mean = loop.arch_step(inp, tgt, plan=step_plans)
            assert MixedOp.MODE is None and isinstance(mean, torch.Tensor) and mean.is_cuda
            q = opt.quality.detach().cpu()
            assert float(mean) == pytest.approx(float(q.mean()), rel=1e-6) and bool(torch.isfinite(q).all())
            assert (q > 0).all() if reward == 'soft' else (q < 0).all()
            choice = torch.tensor([[int(p[0][0]) for p in plan] for plan in step_plans])
            assert torch.equal(opt.choice, choice)
            ops.alpha_reinforce_step(prob, m64, v64, pg64, choice, q.double(), base64, 0.1, (0.0, 0.999), 1e-8, k + 1,
                                     baseline_decay=0.9, err=err64, n_choices=n)
            got = dict(prob=net._flat_alphas()[0], m=opt.m, v=opt.v, prob_grad=net._flat_grads[1], baseline=opt.baseline)
            for name, ref in (('prob', prob), ('m', m64), ('v', v64), ('prob_grad', pg64), ('baseline', base64)):
                e = rel_err(fin(got[name].detach().cpu().numpy()), fin(ref.numpy()))
                _note('loop|%s|%s' % (reward, name), e)
                print('reward', reward, 'arch step', k, name, '%.3g' % e, 'qualities', q.tolist())
                assert e < TOL, (k, name, e)
            assert int(opt.err) == 0 and opt.steps == k + 1
        assert [m.training for m in net.modules()] == flags, 'training flags are put back'
        for w, p in zip(weights, net.net_parameters()):
            assert torch.equal(w, p.detach()), 'an arch step wrote a weight'
        for k, p in net.named_parameters():            # (alpha_prob.grad is the update's prob_grad: the one gradient it sets)
            if k in grads:
                assert (p.grad is None) == (grads[k] is None) and (p.grad is None or torch.equal(grads[k], p.grad)), k
        assert torch.equal(flat, loop.reducer.fg.flat), 'an arch step wrote the flat gradient buffer'
        with pytest.raises(ValueError, match='one per sample'):
            loop.arch_step(inp, tgt, plan=plans[0][:2])
    finally:
        MixedOp.MODE = None
        loop.reducer.fg.disable_sinks()


def test_an_exception_inside_the_reward_puts_mode_and_flags_back(setup):
    from mmnas.model.mixed import MixedOp
    from mmnas_amd.harness import SearchLoop
    c, inp, tgt = setup

    class Boom(RuntimeError):
        pass

    def reward(pred, target):
        raise Boom()

    loop = SearchLoop(_build(c), arch_mode='reinforce', reinforce_samples=2, reward=reward)
    try:
        before = loop.net._flat_alphas()[0].clone()
        MixedOp.MODE = 'two'                       # (arch_step sets None itself and must leave None)
        with pytest.raises(Boom):
            loop.arch_step(inp, tgt)
        assert MixedOp.MODE is None and all(m.training for m in loop.net.modules())
        assert torch.equal(before, loop.net._flat_alphas()[0]) and loop.alpha_optim.steps == 0
    finally:
        MixedOp.MODE = None
        loop.reducer.fg.disable_sinks()


def test_weight_steps_around_an_arch_step_are_the_weight_steps_alone(setup):
    """A weight step, a reinforce arch step, a weight step leave the weights that two weight steps alone leave.  Two runs of
    one weight step need not repeat bit for bit (the backward adds with float atomics: tests/test_sgd_gpu.py), and Adam turns
    the noise of a mathematically zero gradient into a step of full size, so two loops' weights cannot be compared to 1e-5
    whatever lies between their steps.  What decides the claim is compared instead, on ONE loop after one real weight step:
    everything the next weight step reads -- weights, Adam moments and step counts, the flat gradient buffer, the loop's own
    count -- is bitwise what it was before the arch step; the next weight step's forward loss on an injected sample (the
    sampler re-seeding of a search that draws its own) is bit for bit the loss without the arch step, and its gradients agree
    to the project's 1e-5 between two runs of one backward."""
    from mmnas.model.mixed import MixedOp
    from mmnas_amd.harness import SearchLoop
    c, inp, tgt = setup
    rs = np.random.RandomState(12)
    p1, p2 = (_plan_lists(rs, 1, 1)[0][0] for _ in range(2))
    loop = SearchLoop(_build(c), arch_mode='reinforce', reinforce_samples=2, reward_form='add')
    try:
        adam = loop.net_optim.optimizer
        loop.weight_step(inp, tgt, plan=p1)
        loss_b = loop.weight_step(inp, tgt, optimize=False, plan=p2).detach().clone()      # without an arch step in front
        grads_b = loop.reducer.fg.flat.detach().clone()
        torch.cuda.synchronize()
        state = [x.detach().clone() for x in (adam.flat_p, adam.m, adam.v, loop.reducer.fg.flat)]
        counts = (list(adam.steps), loop.net_optim._step, loop.steps)
        alphas = loop.net._flat_alphas()[0].clone()
        loop.arch_step(inp, tgt)
        torch.cuda.synchronize()
        assert not torch.equal(alphas, loop.net._flat_alphas()[0]), 'the arch step moved no alpha'
        for x, y in zip(state, (adam.flat_p, adam.m, adam.v, loop.reducer.fg.flat)):
            assert torch.equal(x, y)
        assert counts == (list(adam.steps), loop.net_optim._step, loop.steps)
        loss_a = loop.weight_step(inp, tgt, optimize=False, plan=p2).detach()
        assert torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
        e = rel_err(loop.reducer.fg.flat.cpu().numpy(), grads_b.cpu().numpy())
        _note('loop|weight_gradients_behind_an_arch_step', e)
        print('gradients of the weight step behind the arch step against the one without: %.3g' % e)
        assert e < TOL
        loop.weight_step(inp, tgt, plan=p2)
        assert bool(torch.isfinite(adam.flat_p).all()) and not torch.equal(adam.flat_p, state[0])
    finally:
        MixedOp.MODE = None
        loop.reducer.fg.disable_sinks()


def test_full_and_two_loops_built_beside_it_are_what_they_were(setup):
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c = cases.net_case('vqa', None, 77, search=True, HSIZE=64)
    for kw, mode, kind in ((dict(arch_mode='two'), None, torch.optim.Adam),
                           (dict(arch_mode='two', fused_arch_update=True), 'two', ArchAdam),
                           (dict(arch_mode='full'), 'full', ArchAdam), (dict(), 'full', ArchAdam),
                           (dict(arch_mode='reinforce'), 'reinforce', ArchAdam)):
        loop = SearchLoop(_build(c), **kw)
        try:
            assert type(loop.alpha_optim) is kind, kw
            if mode:
                assert loop.alpha_optim.mode == mode
            assert hasattr(loop.alpha_optim, 'quality') == (mode == 'reinforce')
        finally:
            loop.reducer.fg.disable_sinks()
