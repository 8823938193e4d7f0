"""The cost-aware architecture update on the GPU (mmnas_alpha_full_step_cost / mmnas_alpha_two_step_cost):
  * both kernels against the float64 torch restatement on the CPU over every case of tests/arch_cost_cases.py (whose inputs
    are conditioned: tests/test_arch_cost_host.py), padding columns, the conservation of each sampled pair's mass;
  * repeatability bit for bit, guard bands around every buffer, prob_grad / stats optional;
  * cost_weight = 0 against the entries without the term;
  * SearchLoop(cost_table=...) against a twin loop whose alphas come from the float64 restatement.

Bounds: 1e-5 (tests/util.rel_err), the project's bar for alphas between two paths; 1e-6 on a pair's logsumexp, the bar of
tests/test_arch_two_gpu.py.

When MMNAS_ARCH_COST_STATS names a file, the worst errors met are written there at the end of the module
(profiles/r14_arch_cost_error_stats.json is one such run)."""
import json
import os

import numpy as np
import pytest
import torch

from tests import arch_cost_cases as AC
from tests.golden import cases
from tests.guardband import Arena
from tests.test_arch_two_host import SETTINGS, TOL, fin
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy

ERR = {}     # label -> worst error met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_ARCH_COST_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


def _lse(prob, pairs):
    return torch.logsumexp(T(np.ascontiguousarray(prob)).gather(1, T(pairs)), dim=1)


@pytest.mark.parametrize('mode,rows,width', [(m, r, w) for m in ('full', 'two') for r, w in AC.SHAPES[m]],
                         ids=lambda x: str(x))
def test_kernel_vs_the_float64_restatement(mode, rows, width):
    for form in AC.FORMS:
        for w in AC.WEIGHTS:
            c = AC.case(mode, rows, width, form, w)
            pad = ~c['live']
            for s in range(len(SETTINGS)):
                got = AC.replay(c, s, torch.float32, DEV)
                ref = AC.reference(mode, rows, width, form, w, s)
                before = c['a0'].astype(np.float64)
                for t, (g, r) in enumerate(zip(got, ref)):
                    for name in AC.NAMES + ('stats',):
                        e = rel_err(fin(g[name]), fin(r[name]))
                        _note('kernel|%s|%s' % (mode, name), e)
                        print('%s %dx%d %s weight %g setting %d step %d %s: %.3g' % (mode, rows, width, form, w, s, t + 1, name, e))
                        assert e < TOL, (form, w, s, t, name, e)
                    assert np.all(np.isneginf(g['prob'][pad])) and np.all(np.isfinite(g['prob'][~pad])), 'padding columns stay -inf'
                    assert not g['m'][pad].any() and not g['v'][pad].any(), 'padding moments stay untouched'
                    assert not g['prob_grad'][pad].any()
                    if mode == 'two':
                        drift = float((_lse(g['prob'], c['pairs'][t]) - _lse(before, c['pairs'][t])).abs().max())
                        _note('kernel|two|pair_logsumexp_drift_abs', drift)
                        print('%s %dx%d %s weight %g setting %d step %d pair logsumexp drift: %.3g' % (mode, rows, width, form, w, s, t + 1, drift))
                        assert drift < 1e-6, (form, w, s, t, drift)
                    before = g['prob']


@pytest.mark.parametrize('mode,rows,width', [('full', 300, 3), ('two', 128, 5)], ids=lambda x: str(x))
def test_same_inputs_give_the_same_bits(mode, rows, width):
    for form in AC.FORMS:
        c = AC.case(mode, rows, width, form, 3.0)
        a, b = AC.replay(c, 1, torch.float32, DEV), AC.replay(c, 1, torch.float32, DEV)
        for x, y in zip(a, b):
            for name in AC.NAMES + ('stats',):
                assert np.array_equal(x[name], y[name]), (form, name)


def _arena_call(c, t, with_pg, with_stats, state=None):
    """One update inside a guard-band arena: gate_grad and cost are inputs, prob / m / v are read and written, prob_grad and
    stats are written whole."""
    from mmnas_amd import ops
    rows, width = c['rows'], c['width']
    ar = Arena(DEV, capacity=4 << 20)
    zero = np.zeros((rows, width), np.float32)
    prob = ar.inout(c['a0'] if state is None else state[0], name='prob')[1]
    m = ar.inout(zero if state is None else state[1], name='m')[1]
    v = ar.inout(zero if state is None else state[2], name='v')[1]
    gg = ar.inp(c['gg'][t], name='gate_grad')[1]
    cost = ar.inp(c['cost'], name='cost')[1]
    pg = ar.out((rows, width), name='prob_grad')[1] if with_pg else None
    st = ar.out(rows + 2, name='stats')[1] if with_stats else None
    pl = [tuple(int(x) for x in p) for p in c['pairs'][t]] if c['mode'] == 'two' else None
    ops.alpha_cost_step(prob, gg, m, v, pg, cost, 0.1, (0.5, 0.999), AC.EPS, t + 1, weight_decay=1e-3, cost_weight=c['weight'],
                        cost_ref=AC.COST_REF, cost_form=c['form'], pairs=pl, stats=st)
    ar.check()
    return [x.clone() for x in (prob, m, v)], pg, st


@pytest.mark.parametrize('mode,rows,width', [('full', 300, 3), ('full', 65, 4), ('two', 128, 5), ('two', 1, 2)], ids=lambda x: str(x))
def test_only_the_outputs_are_written_and_prob_grad_and_stats_are_optional(mode, rows, width):
    c = AC.case(mode, rows, width, 'log', 3.0)
    state, pg, st = _arena_call(c, 0, True, True)
    assert pg is not None and st is not None and float(st[rows]) > 0
    for with_pg, with_stats in ((False, True), (True, False), (False, False)):
        other, _, _ = _arena_call(c, 0, with_pg, with_stats)
        for x, y in zip(state, other):
            assert torch.equal(x, y), (with_pg, with_stats)
    _arena_call(c, 1, True, True, state=[x.cpu().numpy() for x in state])      # with moments in place


@pytest.mark.parametrize('mode,rows,width', [('full', 300, 3), ('full', 65, 4), ('two', 65, 4), ('two', 128, 5)], ids=lambda x: str(x))
def test_cost_weight_zero_against_the_entries_without_the_term(mode, rows, width):
    """prob, m, v and prob_grad within 1e-5 in both modes: every Adam entry forms its coefficients the same way (adam_coef)."""
    from mmnas_amd import ops
    c = AC.case(mode, rows, width, 'linear', 3.0)
    cost = T(c['cost']).to(DEV)
    bitwise = True
    for s, (lr, betas, wd) in enumerate(SETTINGS):
        new = [T(c['a0'].copy()).to(DEV)] + [torch.zeros(rows, width, device=DEV) for _ in range(3)]
        old = [x.clone() for x in new]
        for t in range(AC.STEPS):
            g = T(c['gg'][t]).to(DEV)
            pl = [tuple(int(x) for x in p) for p in c['pairs'][t]] if mode == 'two' else None
            ops.alpha_cost_step(new[0], g, *new[1:], cost, lr, betas, AC.EPS, t + 1, weight_decay=wd, cost_weight=0.0,
                                cost_ref=AC.COST_REF, cost_form='linear', pairs=pl)
            if mode == 'two':
                ops.alpha_two_step(old[0], g, *old[1:], pl, lr, betas, AC.EPS, t + 1, weight_decay=wd)
            else:
                ops.alpha_full_step(old[0], g, *old[1:], lr, betas, AC.EPS, t + 1, weight_decay=wd)
            for name, x, y in zip(AC.NAMES, new, old):
                e = rel_err(fin(x.cpu().numpy()), fin(y.cpu().numpy()))
                bitwise = bitwise and torch.equal(x, y)
                _note('weight0|%s|%s' % (mode, name), e)
                print('%s %dx%d setting %d step %d %s: %.3g' % (mode, rows, width, s, t + 1, name, e))
                assert e < TOL, (s, t, name, e)
    _note('weight0|%s|not_bitwise' % mode, 0.0 if bitwise else 1.0)
    print(mode, rows, width, 'bitwise' if bitwise else 'not bitwise')


def _build(c):
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def _plan_list(plan):
    return plan['enc'] + plan['dec']


@pytest.mark.parametrize('mode', ['full', 'two'])
def test_search_loop_with_a_cost_table_against_the_float64_restatement(mode):
    """Two arch steps with a weight step between them.  The twin loop -- same weights, same plans, no table -- runs
    arch_step(optimize=False); its gate gradients feed the float64 restatement on the CPU, whose alphas the twin then takes.
    The backward adds the gate gradients with float atomics (tests/test_arch_two_gpu.py), so right before the loop's update
    reads its gate-gradient block it takes the twin's."""
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import _lib as L
    from mmnas_amd import cost as K
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(8)
    plans = [_plan_list(cases.search_plan(rs, mode)) for _ in range(2)]
    wplan = _plan_list(cases.search_plan(rs, None))
    inp = tuple(T(a).to(DEV) for a in c['inputs']); tgt = T(c['target']).to(DEV)
    lr, betas, weight, form = 0.1, (0.0, 0.999), 1.0, 'log'
    net = _build(c)
    table = K.CostTable(enc={'self_att_64': 3.0, 'feed_forward': 1.5},
                        dec={'self_att_64': 7.0, 'rel_self_att_64': 9.0, 'guided_att_64': 5.0, 'feed_forward': 2.0}, unit='us')
    loop = SearchLoop(net, arch_mode=mode, fused_arch_update=True, alpha_lr=lr, alpha_betas=betas, cost_table=table, cost_weight=weight,
                      cost_form=form)
    twin = SearchLoop(_build(c), arch_mode=mode, fused_arch_update=True, alpha_lr=lr, alpha_betas=betas)
    lib = L.lib()
    entry = 'mmnas_alpha_two_step_cost' if mode == 'two' else 'mmnas_alpha_full_step_cost'
    real = getattr(lib, entry)
    launches = []
    try:
        opt = loop.alpha_optim
        assert isinstance(opt, ArchAdam) and opt.mode == mode and opt.cost is not None and twin.alpha_optim.cost is None
        block = table.for_net(net)
        assert torch.equal(opt.cost.cpu(), block) and opt.cost_ref == pytest.approx(table.uniform_expected(net))
        setattr(lib, entry, lambda *a: (launches.append(a[7]), real(*a))[1])
        ref = dict(prob=twin.net._flat_alphas()[0].detach().cpu().double())
        ref.update(m=torch.zeros_like(ref['prob']), v=torch.zeros_like(ref['prob']), pg=torch.zeros_like(ref['prob']),
                   stats=torch.zeros(32, dtype=torch.float64))
        step = opt.step

        def step_on_the_twins_gate_gradients():
            loop.net._flat_grads[0].copy_(twin.net._flat_grads[0])
            step()
        opt.step = step_on_the_twins_gate_gradients
        for k, plan in enumerate(plans):
            if k:      # a weight step between the arch steps: the table does not touch it
                lw, tw = loop.weight_step(inp, tgt, plan=wplan), twin.weight_step(inp, tgt, plan=wplan)
                assert torch.equal(lw.detach(), tw.detach()), (float(lw.detach()), float(tw.detach()))
            loss_t = float(twin.arch_step(inp, tgt, optimize=False, plan=plan).detach())
            loss_l = float(loop.arch_step(inp, tgt, plan=plan).detach())
            assert MixedOp.MODE is None and abs(loss_l - loss_t) < 1e-5 * abs(loss_t), (k, loss_l, loss_t)
            gg = twin.net._flat_grads[0].detach().cpu().double()
            assert float(gg.abs().max()) > 0
            pairs = [(act[0], inact[0]) for act, inact in plan] if mode == 'two' else None
            ops.alpha_cost_step(ref['prob'], gg, ref['m'], ref['v'], ref['pg'], block.double(), lr, betas, 1e-8, k + 1,
                                cost_weight=weight, cost_ref=opt.cost_ref, cost_form=form, pairs=pairs, stats=ref['stats'])
            twin.net._flat_alphas()[0].copy_(ref['prob'].float())
            for m in twin.net.redundant_modules:
                m.alpha_version += 1
            e_a = rel_err(fin(loop.net._flat_alphas()[0].detach().cpu().numpy()), fin(ref['prob'].numpy()))
            e_s = rel_err(opt.cost_stats.cpu().numpy(), ref['stats'].numpy())
            _note('loop|%s|alpha' % mode, e_a)
            _note('loop|%s|stats' % mode, e_s)
            print(mode, 'arch step', k, 'loss', loss_l, loss_t, 'alpha', e_a, 'stats', e_s, 'E', float(opt.cost_stats[-2]))
            assert e_a < TOL and e_s < TOL, (k, e_a, e_s)
            assert float(loop.net.expected_cost(block)) == pytest.approx(float(loop.net.expected_cost(opt.cost)))
        assert launches == [30, 30] and opt.steps == 2       # one launch per update, all nodes in it
        assert sorted(opt.state_dict()['param_groups'][0]) == sorted(twin.alpha_optim.state_dict()['param_groups'][0])
    finally:
        setattr(lib, entry, real)
        MixedOp.MODE = None
        for lp in (loop, twin):
            lp.reducer.fg.disable_sinks()


def test_device_float64_takes_no_silent_torch_path():
    from mmnas_amd import _lib as L
    from mmnas_amd import ops
    bufs = [torch.zeros(2, 4, device=DEV, dtype=torch.float64) for _ in range(6)]
    with pytest.raises(L.MMNasHipError):
        ops.alpha_cost_step(*bufs, 0.1, (0.0, 0.999), 1e-8, 1, cost_weight=1.0, cost_ref=2.0)
