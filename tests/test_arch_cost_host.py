"""Host side of the cost-aware architecture update (no GPU):
  * every case of tests/arch_cost_cases.py is conditioned: the float32 torch restatement alone stays within 2.5e-6 of the
    float64 one (the module's docstring says why that is asked of the inputs);
  * the restatement (ops.alpha_cost_step on CPU tensors) in float64 against an independent oracle -- torch.autograd over
    J = sum g . softmax(alpha) + R(alpha) and torch.optim.Adam(weight_decay=...) in float64, for 'two' followed by
    ops.alpha_two_rescale -- to 1e-10, and in float32 to the project's 1e-5;
  * harness.ArchAdam(cost=...) on a CPU supernet: the expected cost falls at every update when the task gradient is zero;
    cost_weight = 0 is the optimizer without a table, bit for bit;
  * mmnas_amd.cost: the flop table against bench.py's formulas, the JSON round trip, the block's order, every ValueError;
  * the argument errors of the Python layer and of the two C entries, which return before any launch."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import arch_cost_cases as AC
from tests.golden import cases
from tests.test_arch_two_host import SETTINGS, TOL, fin
from tests.util import rel_err

T = torch.from_numpy
ALL = AC.combos('full') + AC.combos('two')


@pytest.mark.parametrize('key', ALL, ids=lambda k: '%s-%dx%d-%s-%g' % k)
def test_every_case_is_conditioned(key):
    e = AC.conditioning(AC.case(*key))
    print(key, 'float32 against float64 restatement: %.3g' % e)
    assert e < AC.CONDITION, (key, e)


def _oracle(c, setting):
    """torch.autograd + torch.optim.Adam in float64, one parameter per row over its live columns (a -inf logit has no place in
    an optimizer with weight decay).  Returns per step prob, m, v, prob_grad as padded float64 arrays."""
    from mmnas_amd import ops
    lr, betas, wd = SETTINGS[setting]
    rows, width, n = c['rows'], c['width'], c['n']
    ps = [torch.nn.Parameter(T(c['a0'][r, :n[r]].copy()).double()) for r in range(rows)]
    opt = torch.optim.Adam(ps, lr, betas=betas, eps=AC.EPS, weight_decay=wd)
    cost = T(c['cost']).double()
    out = []

    def padded(rowvals, fill):
        x = np.full((rows, width), fill, np.float64)
        for r, t in enumerate(rowvals):
            x[r, :n[r]] = t.detach().numpy()
        return x

    for t in range(AC.STEPS):
        g = T(c['gg'][t]).double()
        opt.zero_grad()
        E = sum((torch.softmax(p, 0) * cost[r, :n[r]]).sum() for r, p in enumerate(ps))
        R = c['weight'] * (E - AC.COST_REF) / AC.COST_REF if c['form'] == 'linear' else c['weight'] * torch.log(E / AC.COST_REF)
        J = R
        for r, p in enumerate(ps):
            if c['mode'] == 'two':
                ij = T(c['pairs'][t, r])
                J = J + (g[r, ij] * torch.softmax(p[ij], 0)).sum()
            else:
                J = J + (g[r, :n[r]] * torch.softmax(p, 0)).sum()
        J.backward()
        grad = padded([p.grad for p in ps], 0.0)
        old = padded(ps, -np.inf)
        opt.step()
        new = T(padded(ps, -np.inf))
        if c['mode'] == 'two':
            idx = T(c['pairs'][t])
            ops.alpha_two_rescale(new, T(old).gather(1, idx), idx)
            with torch.no_grad():
                for r, p in enumerate(ps):
                    p.copy_(new[r, :n[r]])
        out.append(dict(prob=new.numpy().copy(), prob_grad=grad, m=padded([opt.state[p]['exp_avg'] for p in ps], 0.0),
                        v=padded([opt.state[p]['exp_avg_sq'] for p in ps], 0.0), E=float(E.detach()), R=float(R.detach())))
    return out


@pytest.mark.parametrize('mode', ['full', 'two'])
@pytest.mark.parametrize('rows,width', [(1, 2), (30, 5), (65, 4)], ids=lambda x: str(x))
def test_restatement_against_autograd_and_torch_adam(mode, rows, width):
    for form in AC.FORMS:
        for w in AC.WEIGHTS:
            c = AC.case(mode, rows, width, form, w)
            for s in range(len(SETTINGS)):
                want = _oracle(c, s)
                d64 = AC.distance(AC.reference(mode, rows, width, form, w, s), want)
                d32 = AC.distance(AC.replay(c, s, torch.float32), want)
                print(mode, rows, width, form, w, 'setting', s, 'float64', d64, 'float32', d32)
                assert max(d64.values()) < 1e-10, (form, w, s, d64)
                assert max(d32.values()) < TOL, (form, w, s, d32)
                for got, ref in zip(AC.reference(mode, rows, width, form, w, s), want):      # stats: E_r, E, R
                    assert abs(got['stats'][-2] - ref['E']) < 1e-10 * abs(ref['E'])
                    assert abs(got['stats'][-1] - ref['R']) < 1e-10 * max(abs(ref['R']), 1.0)
                    assert abs(got['stats'][:-2].sum() - ref['E']) < 1e-10 * abs(ref['E'])


def test_padding_stays_and_log_form_without_cost_is_inert():
    from mmnas_amd import ops
    c = AC.case('full', 30, 5, 'log', 3.0)
    for step in AC.reference('full', 30, 5, 'log', 3.0, 1):
        assert np.all(np.isneginf(step['prob'][~c['live']])) and np.all(np.isfinite(step['prob'][c['live']]))
        assert not step['m'][~c['live']].any() and not step['v'][~c['live']].any() and not step['prob_grad'][~c['live']].any()
    # E <= 0 under 'log': the cost part and R are 0 -- the update is the one without a table
    a = T(c['a0'].copy())
    g = T(c['gg'][0])
    outs = []
    for zero_cost in (True, False):
        prob, m, v, pg, st = a.clone(), torch.zeros_like(a), torch.zeros_like(a), torch.zeros_like(a), torch.ones(32)
        ops.alpha_cost_step(prob, g, m, v, pg, torch.zeros_like(a) if zero_cost else T(c['cost']), 0.1, (0.0, 0.999), AC.EPS, 1,
                            cost_weight=3.0 if zero_cost else 0.0, cost_ref=2.0, cost_form='log', stats=st)
        outs.append((prob, m, v, pg))
        if zero_cost:
            assert not st.any()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def _build(c):
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.train()


def _plan_list(plan):
    return plan['enc'] + plan['dec']


def _random_block(net, rs):
    width = net._flat_alphas()[0].shape[1]
    block = torch.zeros(len(net.redundant_modules), width)
    for i, m in enumerate(net.redundant_modules):
        block[i, :m.n_choices] = T(rs.uniform(0.5, 4.0, m.n_choices).astype(np.float32))
    return block


@pytest.mark.parametrize('mode', ['full', 'two'])
@pytest.mark.parametrize('form', AC.FORMS)
def test_expected_cost_falls_on_a_host_supernet_when_the_task_gradient_is_zero(mode, form):
    from mmnas_amd import cost as K
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(21)
    net = _build(c)
    block = K.flop_cost_table(net, 5, 7) if form == 'linear' else _random_block(net, rs)
    opt = ArchAdam(net, 0.1, (0.0, 0.999), mode=mode, cost=block, cost_weight=1.0, cost_form=form)
    n_choices = [m.n_choices for m in net.redundant_modules]
    assert opt.cost_ref == pytest.approx(K.uniform_expected(block, n_choices)) and opt.cost_stats.shape == (32,)
    seen = [float(net.expected_cost(block))]
    for k in range(8):
        net.set_sampled(_plan_list(cases.search_plan(rs, mode)))
        for m in net.redundant_modules:
            m.alpha_gate.grad = torch.zeros(m.n_choices)
        opt.step()
        assert float(opt.cost_stats[-2]) == pytest.approx(seen[-1], rel=1e-5)      # E of the alphas before the update
        seen.append(float(net.expected_cost(block)))
        print(mode, form, 'update', k, 'E', seen[-1], 'R', float(opt.cost_stats[-1]))
        assert seen[-1] < seen[-2], (k, seen)
    assert isinstance(net.expected_cost(block), torch.Tensor) and net.expected_cost(block).dim() == 0
    pick = net._flat_alphas()[0].argmax(dim=1)
    assert net.genotype_cost(block) == pytest.approx(float(sum(block[i, int(j)] for i, j in enumerate(pick))))
    assert isinstance(net.genotype_cost(block), float)


@pytest.mark.parametrize('mode', ['full', 'two'])
def test_cost_weight_zero_is_the_optimizer_without_a_table_bit_for_bit(mode, monkeypatch):
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    plain, zero = _build(c), _build(c)
    popt = ArchAdam(plain, 0.1, (0.5, 0.999), weight_decay=1e-3, mode=mode)
    zopt = ArchAdam(zero, 0.1, (0.5, 0.999), weight_decay=1e-3, mode=mode, cost=_random_block(zero, np.random.RandomState(2)),
                    cost_weight=0.0, cost_form='log')
    assert zopt.cost is None and zopt.cost_stats is None
    monkeypatch.setattr(ops, 'alpha_cost_step', lambda *a, **k: pytest.fail('the cost entry was called'))
    if mode == 'full':      # (ops.alpha_full_step has no host branch: 'full' without a table runs on the device only)
        called = []
        monkeypatch.setattr(ops, 'alpha_full_step', lambda *a, **k: called.append(a))
        for opt, net in ((popt, plain), (zopt, zero)):
            net.begin_arch_step()
            opt.step()
        assert len(called) == 2 and all(len(a) == len(called[0]) for a in called)
        assert all(x is y or x == y for x, y in zip(called[0][5:], called[1][5:]))
        return
    rs = np.random.RandomState(5)
    for _ in range(3):
        plan = _plan_list(cases.search_plan(rs, 'two'))
        grads = [rs.uniform(-1, 1, m.n_choices).astype(np.float32) for m in plain.redundant_modules]
        for net, opt in ((plain, popt), (zero, zopt)):
            net.set_sampled(plan)
            for m, g in zip(net.redundant_modules, grads):
                m.alpha_gate.grad = T(g.copy())
            opt.step()
        assert torch.equal(plain._flat_alphas()[0], zero._flat_alphas()[0])
        assert torch.equal(popt.m, zopt.m) and torch.equal(popt.v, zopt.v)
    assert popt.state_dict().keys() == zopt.state_dict().keys()
    assert popt.state_dict()['param_groups'] == zopt.state_dict()['param_groups']      # configuration, not state


def test_flop_table_is_benchs_formula_for_the_shipped_names():
    from mmnas_amd import cost as K
    from mmnas_amd.utils.ops_adapter import OpsAdapter
    spec = importlib.util.spec_from_file_location(
        'bench', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)      # (the library itself does not import the benchmark)
    for d in (128, 256, 512):
        cfg = cases.small_cfg(HSIZE=d)
        for Sx, Sy in ((14, 100), (5, 7)):
            for kind in ('enc', 'dec'):
                for name in ('self_att_64', 'rel_self_att_64', 'guided_att_64', 'feed_forward', 'none'):
                    assert K.op_flops(name, cfg, Sx, Sy, kind) == bench.op_flops_fwd(name, 1, Sx, Sy, d, kind), (name, d, kind)
    cfg = cases.small_cfg(HSIZE=256)
    names = sorted(OpsAdapter().OPS)
    assert len(names) == 41
    flops = {n: K.op_flops(n, cfg, 14, 100, 'dec') for n in names}
    assert all(isinstance(f, int) and f >= 0 for f in flops.values())
    assert [n for n, f in flops.items() if f == 0] == ['gelu', 'leakyrelu', 'none', 'relu', 'skip_connect']
    assert flops['self_att_64_2'] > flops['self_att_64'] and flops['feed_forward_8'] == 2 * flops['feed_forward']
    assert flops['std_conv_7'] > flops['std_conv_3'] > flops['sep_conv_3']
    with pytest.raises(ValueError):
        K.op_flops('self_att', cfg, 14, 100, 'dec')
    with pytest.raises(ValueError):
        K.op_flops('feed_forward', cfg, 14, 100, 'mid')


def test_cost_tables(tmp_path):
    from mmnas_amd import cost as K
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c = cases.net_case('vqa', None, 4343, search=True)
    net = _build(c)
    mods = net.redundant_modules
    kinds = K.node_kinds(net)
    assert kinds == ['enc'] * 12 + ['dec'] * 18
    flop = K.flop_cost_table(net, 5, 7)
    assert flop.shape == (30, 4) and flop.dtype == torch.float32
    for i, m in enumerate(mods):
        want = [K.op_flops(n, c['cfg'], 5, 7, kinds[i]) / 1e6 for n in m.Used_OPS]
        assert flop[i, :m.n_choices].tolist() == pytest.approx(want) and not flop[i, m.n_choices:].any()
    # a table: JSON round trip and the block's order (rows = redundant_modules, columns = the node's Used_OPS)
    tab = K.CostTable(enc={'self_att_64': 3.0, 'feed_forward': 1.5, 'none': 0.0},
                      dec={'self_att_64': 7.0, 'rel_self_att_64': 9.0, 'guided_att_64': 5.0, 'feed_forward': 2.0, 'none': 0},
                      unit='us', meta={'batch': 64, 'shapes': {'Sx': 14}})
    path = str(tmp_path / 'table.json')
    tab.to_json(path)
    back = K.CostTable.from_json(path)
    assert (back.enc, back.dec, back.unit, back.meta) == (tab.enc, tab.dec, tab.unit, tab.meta)
    block = back.for_net(net)
    assert block.shape == (30, 4) and block.dtype == torch.float32
    for i, m in enumerate(mods):
        src = tab.enc if kinds[i] == 'enc' else tab.dec
        assert block[i, :m.n_choices].tolist() == [src[n] for n in m.Used_OPS] and not block[i, m.n_choices:].any()
    assert back.uniform_expected(net) == pytest.approx(12 * (3.0 + 1.5) / 2 + 18 * (7.0 + 9.0 + 5.0 + 2.0) / 4)
    assert ArchAdam(net, cost=back, cost_weight=0.5).cost_ref == pytest.approx(back.uniform_expected(net))
    # every ValueError
    with pytest.raises(ValueError, match='guided_att_64'):
        K.CostTable(enc=tab.enc, dec={k: v for k, v in tab.dec.items() if k != 'guided_att_64'}).for_net(net)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            K.CostTable(enc=dict(tab.enc, feed_forward=bad), dec=tab.dec)
    zeros = K.CostTable(enc={k: 0.0 for k in tab.enc}, dec={k: 0.0 for k in tab.dec})
    assert not zeros.for_net(net).any()                      # 'linear' takes it
    with pytest.raises(ValueError, match='log'):
        zeros.for_net(net, cost_form='log')
    with pytest.raises(ValueError, match='log'):
        ArchAdam(net, cost=zeros, cost_weight=1.0, cost_form='log', cost_ref=1.0)
    with pytest.raises(ValueError, match='cost_ref'):
        ArchAdam(net, cost=zeros, cost_weight=1.0)           # the default reference of a table of zeros is 0
    for kw in (dict(cost_form='quadratic'), dict(cost_weight=-1.0), dict(cost_ref=0.0), dict(cost_ref=float('inf'))):
        with pytest.raises(ValueError):
            ArchAdam(net, **dict(dict(cost=tab, cost_weight=1.0), **kw))
    with pytest.raises(ValueError):
        ArchAdam(net, cost=block[:, :3], cost_weight=1.0)    # not the alpha block's shape
    neg = block.clone()
    neg[3, 1] = -1.0
    with pytest.raises(ValueError):
        ArchAdam(net, cost=neg, cost_weight=1.0)
    pad = block.clone()
    pad[0, 3] = 1.0                                          # node 0 has two candidates
    with pytest.raises(ValueError, match='padding'):
        ArchAdam(net, cost=pad, cost_weight=1.0)
    # the per-node torch-Adam path of 'two' does not carry the term
    with pytest.raises(ValueError, match='fused_arch_update'):
        SearchLoop(net, arch_mode='two', cost_table=tab, cost_weight=1.0, fused_arch_update=False)
    with pytest.raises(ValueError, match='fused_arch_update'):
        SearchLoop(net, arch_mode='two', cost_table=tab)


def _blocks(rows, width=4):
    return (torch.zeros(rows, width), torch.ones(rows, width), torch.zeros(rows, width), torch.zeros(rows, width),
            torch.zeros(rows, width), torch.ones(rows, width))


def test_python_layer_argument_errors():
    from mmnas_amd import ops
    hyper = (0.1, (0.0, 0.999), 1e-8)
    prob, gg, m, v, pg, cost = _blocks(3)
    prob[0, 2:] = float('-inf')
    cost[0, 2:] = 0
    good = [(0, 1), (1, 3), (2, 0)]
    ok = dict(cost_weight=1.0, cost_ref=2.0, cost_form='linear')
    for step, kw, what in ((1, dict(ok, cost_form='cubic'), 'form'), (1, dict(ok, cost_ref=0.0), 'ref 0'),
                           (1, dict(ok, cost_ref=float('nan')), 'ref nan'), (1, dict(ok, cost_weight=-0.5), 'weight < 0'),
                           (0, ok, 'step < 1'), (1, dict(ok, pairs=good[:2]), 'a pair missing'),
                           (1, dict(ok, pairs=[(0, 0), (1, 3), (2, 0)]), 'i == j'), (1, dict(ok, pairs=[(0, 1), (1, 4), (2, 0)]), 'index'),
                           (1, dict(ok, pairs=[(0, 2), (1, 3), (2, 0)]), 'padding column'),
                           (1, dict(ok, stats=torch.zeros(4)), 'stats size')):
        before = prob.clone()
        with pytest.raises(ValueError):
            ops.alpha_cost_step(prob, gg, m, v, pg, cost, *hyper, step, **kw)
        assert torch.equal(prob, before) and not m.any() and not v.any(), what       # nothing was written
    with pytest.raises(ValueError):
        ops.alpha_cost_step(prob, gg, m, v, pg, cost[:, :3], *hyper, 1, **ok)
    with pytest.raises(ValueError):
        ops.alpha_cost_step(prob, gg, m, v, pg, None, *hyper, 1, **ok)
    ops.alpha_cost_step(prob, gg, m, v, None, cost, *hyper, 1, pairs=good, **ok)     # prob_grad and stats are optional
    with pytest.raises(ValueError):
        ops.alpha_cost_step(*_blocks(129), *hyper, 1, pairs=[(0, 1)] * 129, **ok)
    ops.alpha_cost_step(*_blocks(128), *hyper, 1, pairs=[(0, 1)] * 128, **ok)        # the limit itself
    ops.alpha_cost_step(*_blocks(129), *hyper, 1, **ok)                              # 'full' has none
    st = torch.ones(2)
    ops.alpha_cost_step(*_blocks(0), *hyper, 1, stats=st, **ok)                      # no rows: E = 0
    assert st.tolist() == [0.0, -1.0]


def test_c_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for the device pointers: every call here must return from the entry's own checks (a launch
    without a device would come back as MMNAS_E_LAUNCH = -3, never as -1 / -2)."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    assert len(L.SYMBOLS['mmnas_alpha_full_step_cost'][1]) == 19 and len(L.SYMBOLS['mmnas_alpha_two_step_cost'][1]) == 20
    buf = [(ctypes.c_float * (130 * 4 + 2))() for _ in range(7)]
    p = [ctypes.cast(b, ctypes.c_void_p).value for b in buf]
    base = dict(rows=2, width=4, pairs=[0, 1, 1, 2], weight=1.0, ref=2.0, form=0, step=1, null=None)

    def call(two, **over):
        a = dict(base, **over)
        ptrs = [None if i == a['null'] else x for i, x in enumerate(p)]
        tail = (0.1, 0.0, 0.999, 1e-8, 0.0, a['weight'], a['ref'], a['form'], a['step'], None)
        if two:
            arr = (ctypes.c_int * max(1, len(a['pairs'])))(*a['pairs']) if a['pairs'] is not None else None
            return lib.mmnas_alpha_two_step_cost(*ptrs, a['rows'], a['width'], arr, *tail)
        return lib.mmnas_alpha_full_step_cost(*ptrs, a['rows'], a['width'], *tail)

    for two, who in ((False, b'mmnas_alpha_full_step_cost'), (True, b'mmnas_alpha_two_step_cost')):
        for over in (dict(form=2), dict(form=-1), dict(ref=0.0), dict(ref=-2.0), dict(ref=float('inf')), dict(ref=float('nan')),
                     dict(weight=-1.0), dict(step=0), dict(width=0), dict(rows=-1),
                     dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=5)):
            rc = call(two, **over)
            assert rc == (-1 if two and 'rows' in over else -2), (two, over, rc)
            assert who in lib.mmnas_last_error(), (over, lib.mmnas_last_error())
    assert call(True, width=1, pairs=[0, 0, 0, 0]) == -2 and b'width=1' in lib.mmnas_last_error()
    assert call(True, rows=129, pairs=[0, 1] * 129) == -1 and b'rows=129' in lib.mmnas_last_error()      # MMNAS_E_SHAPE
    assert call(True, pairs=[0, 1, 2, 2]) == -2 and b'row 1' in lib.mmnas_last_error()                   # i == j
    assert call(True, pairs=[0, 4, 1, 2]) == -2 and call(True, pairs=[0, 1, -1, 2]) == -2
    assert call(True, pairs=None) == -2
    assert not any(any(b) for b in buf)
