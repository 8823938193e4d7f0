"""Host side of the REINFORCE architecture update (no GPU):
  * every case of tests/arch_reinforce_cases.py is conditioned: the float32 torch restatement alone stays within 2.5e-6 of
    the float64 one;
  * the float64 restatement (ops.alpha_reinforce_step on CPU tensors) against an independent oracle -- torch.autograd over
    -(1 / M) sum_i A_i sum_r log_softmax(alpha_r)[a_ir] with A detached, then torch.optim.Adam(weight_decay=...) -- to 1e-10;
  * the baseline rule, the err flag, the padding, a toy search that learns;
  * harness.ArchAdam(mode='reinforce') checkpoints, also into torch.optim.Adam and the other modes;
  * the argument errors of the C entry (before any launch) and of the Python layer;
  * two gloo processes on different shards keep bit-identical alphas, equal to one process fed the mean of their rewards."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import arch_reinforce_cases as RC
from tests.golden import cases
from tests.test_arch_two_host import SETTINGS

T = torch.from_numpy
ALL = RC.combos()
IDS = ['%dx%d-M%d-%s' % k for k in ALL]


@pytest.mark.parametrize('key', ALL, ids=IDS)
def test_every_case_is_conditioned(key):
    e = RC.conditioning(RC.case(*key))
    print(key, 'float32 against float64 restatement: %.3g' % e)
    assert e < RC.CONDITION, (key, e)


def test_the_case_table_covers_what_the_issue_lists():
    assert RC.DROPPED == ()
    assert {(k[0], k[1]) for k in ALL} == {(1, 2), (30, 5), (65, 4), (128, 5), (300, 3)}
    assert {k[2] for k in ALL if k[:2] == (30, 5)} == {1, 4, 16} and {k[2] for k in ALL if k[:2] == (128, 5)} == {1, 4, 16}
    assert {k[2] for k in ALL if k[:2] == (300, 3)} == {1, 4}
    assert RC.REWARDS == {'none': (None, 0.0), 'mul': ('mul', -0.07), 'add': ('add', -0.3)} and RC.DECAY == 0.9 and RC.STEPS == 4
    c = RC.case(65, 4, 4, 'mul')
    assert float(c['quality'].min()) > 0.3 and float(c['quality'].max()) < 0.7
    assert np.isneginf(c['a0'][~c['live']]).all() and (~c['live']).any()
    assert not c['cost'][np.arange(65), c['n'] - 1].any() and (c['choice'] < c['n'][None, None, :]).all()


def _oracle(c, setting, baseline0):
    """torch.autograd + torch.optim.Adam in float64, one parameter per row over its live columns.  The rewards and the
    baseline are restated here in plain Python floats."""
    lr, betas, wd = SETTINGS[setting]
    rows, width, n, M = c['rows'], c['width'], c['n'], c['M']
    form, w = RC.REWARDS[c['reward']]
    ps = [torch.nn.Parameter(T(c['a0'][r, :n[r]].copy()).double()) for r in range(rows)]
    opt = torch.optim.Adam(ps, lr, betas=betas, eps=RC.EPS, weight_decay=wd)
    cost = c['cost'].astype(np.float64)
    base, out = baseline0, []

    def padded(rowvals, fill):
        x = np.full((rows, width), fill, np.float64)
        for r, t in enumerate(rowvals):
            x[r, :n[r]] = t.detach().numpy()
        return x

    for t in range(RC.STEPS):
        R = []
        for i in range(M):
            q = float(c['quality'][t, i])
            C = float(sum(cost[r, c['choice'][t, i, r]] for r in range(rows)))
            if form is None or C <= 0:
                R.append(q)
            elif form == 'mul':
                R.append(q * (C / c['cost_ref']) ** w)
            else:
                R.append(q + w * np.log(C / c['cost_ref']))
        rbar = sum(R) / M
        b = rbar if base is None else base
        A = [x - b for x in R]
        opt.zero_grad()
        J = 0.0
        for i in range(M):
            J = J + A[i] * sum(torch.log_softmax(p, 0)[c['choice'][t, i, r]] for r, p in enumerate(ps))
        (-J / M).backward()
        grad = padded([p.grad for p in ps], 0.0)
        opt.step()
        base = rbar if base is None else RC.DECAY * base + (1 - RC.DECAY) * rbar
        out.append(dict(prob=padded(ps, -np.inf), prob_grad=grad, m=padded([opt.state[p]['exp_avg'] for p in ps], 0.0),
                        v=padded([opt.state[p]['exp_avg_sq'] for p in ps], 0.0), stats=np.array(R + [rbar, b, base]),
                        baseline=np.array([base, 1.0])))
    return out


def _distance(got, ref):
    """tests/util.rel_err per quantity with the denominator floored at 1e-6.  Where every sample of the first update took the
    same column of a row, the true gradient there is sum_i A_i = 0 and both sides hold float64 rounding noise (1e-17) or an
    exact zero: a ratio of two such numbers says nothing, their difference against 1e-6 * 1e-10 still has to vanish."""
    out = {}
    for k in RC.NAMES + ('baseline',):
        out[k] = 0.0
        for g, r in zip(got, ref):
            g, r = RC.fin(g[k]), RC.fin(r[k])
            assert g.shape == r.shape
            out[k] = max(out[k], float(np.max(np.abs(g - r)) / max(np.max(np.abs(r)), 1e-6)))
    return out


@pytest.mark.parametrize('rows,width,M', [(1, 2, 1), (1, 2, 4), (30, 5, 4), (30, 5, 16), (65, 4, 1), (65, 4, 4)], ids=str)
def test_float64_restatement_against_autograd_and_torch_adam(rows, width, M):
    """Every setting from an initialised baseline (0.5: the EMA rule at all four steps), and from a fresh baseline (the first
    update uses Rbar) under the setting with weight decay.  A fresh baseline under beta1 = 0 without weight decay is left
    out, and this is why: the first update then has sum_i A_i = 0 up to float64 rounding, a column no sample took receives
    g = p * noise / M ~ 1e-18 on both sides -- from two different summation orders -- and Adam's first step turns it into
    lr * g / (|g| + 1e-8) ~ lr * 1e-10, the bound itself at lr 0.1 and 1.0.  The comparison would measure that noise.  With
    weight decay the column's gradient is wd * alpha and the noise drowns; with an initialised baseline sum_i A_i is not 0."""
    for reward in RC.REWARDS:
        c = RC.case(rows, width, M, reward)
        for s, b0 in [(s, 0.5) for s in range(len(SETTINGS))] + [(1, None)]:
            assert b0 is not None or SETTINGS[s][2] > 0
            want = _oracle(c, s, b0)
            got = RC.reference(rows, width, M, reward, s) if b0 is None else RC.replay(c, s, torch.float64, baseline0=b0)
            d = _distance(got, want)
            print(rows, width, M, reward, 'setting', s, 'baseline', b0, d)
            assert max(d.values()) < 1e-10, (reward, s, b0, d)


def _state(rows=5, width=4, dtype=torch.float64, seed=3):
    c = RC.generate(rows, width, 4, seed)
    prob = T(c['a0'].copy()).to(dtype)
    return c, prob, torch.zeros_like(prob), torch.zeros_like(prob), torch.full_like(prob, 7.0)


def test_baseline_rule_and_a_single_sample_moves_nothing_at_step_one():
    from mmnas_amd import ops
    c, prob, m, v, pg = _state()
    base, err = torch.zeros(2, dtype=torch.float64), torch.zeros(1, dtype=torch.int32)
    stats = torch.zeros(7, dtype=torch.float64)
    q = T(c['quality'].astype(np.float64))
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], q[0], base, 0.1, (0.0, 0.999), 1e-8, 1, baseline_decay=0.9, stats=stats,
                             err=err)
    rbar = float(stats[4])
    assert rbar == pytest.approx(float(q[0].mean()), rel=1e-15) and stats[5] == stats[4] and stats[6] == stats[4]      # first: b = Rbar
    assert base.tolist() == [float(stats[4]), 1.0] and torch.equal(stats[:4], q[0])
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][1], q[1], base, 0.1, (0.0, 0.999), 1e-8, 2, baseline_decay=0.9, stats=stats,
                             err=err)
    r2 = float(q[1].mean())
    assert float(stats[5]) == rbar and float(stats[6]) == pytest.approx(0.9 * rbar + 0.1 * r2, rel=1e-14)     # later: the EMA
    assert float(base[0]) == float(stats[6]) and int(err) == 0
    # M = 1 at step 1: A = R - R = 0, the alphas stay bit for bit (documented: the rule, not a defect)
    c, prob, m, v, pg = _state(dtype=torch.float32)
    before = prob.clone()
    base, err = torch.zeros(2), torch.zeros(1, dtype=torch.int32)
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0][:1], T(c['quality'][0][:1]), base, 1.0, (0.0, 0.999), 1e-8, 1, err=err)
    assert torch.equal(prob, before) and not pg.any() and not m.any() and float(base[0]) == float(c['quality'][0][0])
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][1][:1], T(c['quality'][1][:1]), base, 1.0, (0.0, 0.999), 1e-8, 2, err=err)
    assert not torch.equal(prob, before)


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), -float('inf')])
def test_a_non_finite_quality_sets_err_and_writes_nothing(bad):
    from mmnas_amd import ops
    c, prob, m, v, pg = _state(dtype=torch.float32)
    base, err, stats = torch.tensor([0.4, 1.0]), torch.zeros(1, dtype=torch.int32), torch.full((7,), 7.0)
    m.fill_(0.25)
    v.fill_(0.5)
    keep = [x.clone() for x in (prob, m, v, pg, base, stats)]
    q = T(c['quality'][0].copy())
    q[2] = bad
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], q, base, 0.1, (0.5, 0.999), 1e-8, 3, stats=stats, err=err,
                             cost=T(c['cost']), cost_weight=-0.07, cost_ref=7.5)
    assert int(err) == 1
    for x, k in zip((prob, m, v, pg, base, stats), keep):
        assert torch.equal(x, k) or (torch.equal(torch.isnan(x), torch.isnan(k)) and torch.equal(fin_t(x), fin_t(k)))
    # a reward that overflows although every quality is finite
    err.zero_()
    big = torch.full((4,), 3e38)
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], big, base, 0.1, (0.5, 0.999), 1e-8, 3, err=err, cost=T(c['cost']),
                             cost_weight=8.0, cost_ref=0.01)
    assert int(err) == 1 and torch.equal(fin_t(prob), fin_t(keep[0])) and torch.equal(base, keep[4])


def fin_t(x):
    return torch.where(torch.isfinite(x), x, torch.zeros_like(x))


def test_padding_stays():
    for key in ((65, 4, 4, 'add'), (300, 3, 4, 'mul')):
        c = RC.case(*key)
        for step in RC.replay(c, 1, torch.float32):
            pad = ~c['live']
            assert pad.any() and np.isneginf(step['prob'][pad]).all() and np.isfinite(step['prob'][~pad]).all()
            assert not step['m'][pad].any() and not step['v'][pad].any() and not step['prob_grad'][pad].any()
            assert step['err'] == 0


def test_it_learns_the_best_architecture_of_a_toy_table():
    """2 x 3 block, a fixed reward per architecture with (1, 2) the best, a seeded sampler, M = 4, 300 updates."""
    from mmnas_amd import ops
    table = torch.tensor([[0.2, 0.3, 0.1], [0.3, 0.4, 0.9], [0.1, 0.4, 0.2]])          # table[a_0][a_1]: 0.9 at (1, 2)
    prob, m, v = torch.zeros(2, 3), torch.zeros(2, 3), torch.zeros(2, 3)
    base, err = torch.zeros(2), torch.zeros(1, dtype=torch.int32)
    gen = torch.Generator().manual_seed(17)
    for step in range(1, 301):
        p = torch.softmax(prob, dim=1)
        ch = torch.multinomial(p, 4, replacement=True, generator=gen).t().contiguous()      # [M, rows]
        q = table[ch[:, 0], ch[:, 1]]
        ops.alpha_reinforce_step(prob, m, v, None, ch, q, base, 0.05, (0.0, 0.999), 1e-8, step, baseline_decay=0.9, err=err)
    p = torch.softmax(prob, dim=1)
    print('probabilities after 300 updates', p.tolist(), 'baseline', base.tolist())
    assert int(err) == 0 and float(p[0, 1] * p[1, 2]) > 0.9, p


def _build(c):
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.train()


def _drive(opt, rs, k):
    n = opt.n_choices
    for _ in range(k):
        opt.choice.copy_(T(np.stack([rs.randint(0, n) for _ in range(opt.n_samples)])))
        opt.quality.copy_(T(rs.uniform(0.3, 0.7, opt.n_samples).astype(np.float32)))
        opt.step()


def test_arch_adam_reinforce_checkpoints(tmp_path):
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(2)
    net = _build(c)
    opt = ArchAdam(net, 0.1, (0.5, 0.999), weight_decay=1e-3, mode='reinforce', n_samples=4, baseline_decay=0.9)
    versions = [m.alpha_version for m in net.redundant_modules]
    _drive(opt, rs, 3)
    assert [m.alpha_version for m in net.redundant_modules] == [x + 3 for x in versions] and int(opt.err) == 0
    assert net.redundant_modules[0].alpha_prob.grad is not None
    sd = opt.state_dict()
    assert set(sd) == {'state', 'param_groups', 'reinforce'} and sd['reinforce']['initialised'] is True
    torch.save(sd, tmp_path / 'alpha.pt')
    sd = torch.load(tmp_path / 'alpha.pt')
    # round trip: moments, step count and baseline bit for bit
    other = ArchAdam(_build(c), mode='reinforce', n_samples=4)
    other.load_state_dict(sd)
    assert torch.equal(other.m, opt.m) and torch.equal(other.v, opt.v) and other.steps == 3 and torch.equal(other.baseline, opt.baseline)
    assert other.betas == (0.5, 0.999) and other.weight_decay == 1e-3
    # a file without the key: a fresh baseline
    plain = {k: v for k, v in sd.items() if k != 'reinforce'}
    other.load_state_dict(plain)
    assert other.baseline.tolist() == [0.0, 0.0] and other.steps == 3 and torch.equal(other.m, opt.m)
    # a file with the key loads into torch Adam (which ignores it) and into the other modes
    net2 = _build(c)
    net2._flat_alphas()
    adam = torch.optim.Adam(list(net2.alpha_prob_parameters()), 0.1)
    adam.load_state_dict(sd)
    assert 'reinforce' not in adam.state_dict()
    st = adam.state_dict()['state']
    for i, m in enumerate(net2.redundant_modules):
        assert torch.equal(st[i]['exp_avg'], opt.m[i, :m.n_choices]) and float(st[i]['step']) == 3.0
    two = ArchAdam(_build(c), mode='two')
    two.load_state_dict(sd)
    assert torch.equal(two.m, opt.m) and torch.equal(two.v, opt.v) and two.steps == 3 and 'reinforce' not in two.state_dict()
    # and the other way: a 'two' checkpoint into the reinforce mode
    other.load_state_dict(two.state_dict())
    assert other.baseline.tolist() == [0.0, 0.0] and torch.equal(other.m, opt.m)


def test_arch_adam_reinforce_prices_the_sampled_architecture_with_a_negative_weight():
    from mmnas_amd import cost as K
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam
    c = cases.net_case('vqa', None, 4343, search=True)
    net = _build(c)
    block = K.flop_cost_table(net, 5, 7)
    n = [m.n_choices for m in net.redundant_modules]
    opt = ArchAdam(net, mode='reinforce', n_samples=2, cost=block, cost_weight=-0.07, reward_form='mul')
    assert opt.cost_ref == pytest.approx(K.uniform_expected(block, n))            # the default: the uniform expected cost
    rs = np.random.RandomState(4)
    _drive(opt, rs, 1)
    R = ops.alpha_reinforce_rewards(opt.quality, opt.choice, opt.cost, -0.07, opt.cost_ref, 'mul')
    assert torch.equal(opt.reinforce_stats[:2], R) and not torch.equal(R, opt.quality)
    with pytest.raises(ValueError):                                                # 'full' / 'two' keep their validation
        ArchAdam(_build(c), mode='full', cost=block, cost_weight=-0.07)


def test_c_entry_rejects_bad_arguments_before_any_launch():
    """Host buffers stand in for the device pointers: every call here must return from the entry's own checks (a launch
    without a device would come back as MMNAS_E_LAUNCH = -3, never as -1 / -2)."""
    from mmnas_amd import _lib as L
    lib = L.lib()
    assert len(L.SYMBOLS['mmnas_alpha_reinforce_step'][1]) == 25
    names = ('prob', 'm', 'v', 'prob_grad', 'quality', 'cost', 'baseline', 'stats', 'err')
    buf = {k: (ctypes.c_float * 4096)() for k in names}
    base = dict(rows=2, width=4, M=2, choice=[0, 1, 2, 0], n=[4, 3], weight=-0.07, ref=2.0, form=0, decay=0.9, step=1, null=())

    def call(**over):
        a = dict(base, **over)
        p = {k: (None if k in a['null'] else ctypes.cast(b, ctypes.c_void_p).value) for k, b in buf.items()}
        ch = None if a['choice'] is None else (ctypes.c_ubyte * max(1, len(a['choice'])))(*a['choice'])
        n = None if a['n'] is None else (ctypes.c_int * max(1, len(a['n'])))(*a['n'])
        return lib.mmnas_alpha_reinforce_step(p['prob'], p['m'], p['v'], p['prob_grad'], a['rows'], a['width'], ch, n, a['M'],
                                              p['quality'], p['cost'], a['weight'], a['ref'], a['form'], p['baseline'], a['decay'],
                                              p['stats'], p['err'], 0.1, 0.0, 0.999, 1e-8, 0.0, a['step'], None)

    for over in (dict(form=2), dict(form=-1), dict(ref=0.0), dict(ref=-2.0), dict(ref=float('inf')), dict(ref=float('nan')),
                 dict(weight=float('inf')), dict(weight=float('nan')), dict(decay=1.0), dict(decay=-0.1), dict(decay=float('nan')),
                 dict(M=0), dict(step=0), dict(width=0), dict(rows=-1), dict(choice=None), dict(n=None),
                 dict(null=('prob',)), dict(null=('m',)), dict(null=('v',)), dict(null=('quality',)), dict(null=('baseline',)),
                 dict(null=('err',)),
                 dict(choice=[0, 3, 2, 0]),            # row 1 has three live columns
                 dict(choice=[0, 1, 4, 0]),            # outside the block
                 dict(n=[4, 0]), dict(n=[5, 3])):
        rc = call(**over)
        assert rc == -2, (over, rc, lib.mmnas_last_error())
        assert b'mmnas_alpha_reinforce_step' in lib.mmnas_last_error(), (over, lib.mmnas_last_error())
    # MMNAS_E_SHAPE: past the argument block.  300 x 4 and 128 x 16 are inside it: with an index out of range, which is looked
    # at after the limits, they come back as MMNAS_E_ARG from the index check
    assert call(rows=769, M=4, choice=[0] * 3076, n=[4] * 769) == -1 and b'3076' in lib.mmnas_last_error()
    assert call(rows=1, M=257, choice=[0] * 257, n=[4]) == -1
    assert call(width=257, n=[257, 3]) == -1
    for rows, M in ((300, 4), (128, 16), (3072, 1), (12, 256)):
        assert call(rows=rows, M=M, choice=[0] * (rows * M - 1) + [4], n=[4] * rows) == -2, (rows, M)
        assert b'candidate 4 outside' in lib.mmnas_last_error()
    # a weight of either sign and the nullable three pass every check before the index check
    assert call(weight=0.07, choice=[0, 1, 2, 3]) == -2 and b'candidate 3 outside' in lib.mmnas_last_error()
    assert call(null=('prob_grad', 'cost', 'stats'), choice=[0, 1, 2, 3]) == -2 and b'candidate 3 outside' in lib.mmnas_last_error()
    assert not any(any(b) for b in buf.values())


def test_python_layer_argument_errors():
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam, NegLossReward, SearchLoop, reinforce_arch_step
    c, prob, m, v, pg = _state(dtype=torch.float32)
    base, err, q = torch.zeros(2), torch.zeros(1, dtype=torch.int32), T(c['quality'][0])
    good = dict(lr=0.1, betas=(0.0, 0.999), eps=1e-8, step=1, err=err)
    ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], q, base, **good)
    for over in (dict(reward_form='linear'), dict(cost_ref=0.0), dict(cost_ref=float('nan')), dict(cost_weight=float('inf')),
                 dict(baseline_decay=1.0), dict(baseline_decay=-0.5), dict(step=0), dict(err=None), dict(stats=torch.zeros(6)),
                 dict(cost=torch.zeros(5, 3))):
        with pytest.raises(ValueError):
            ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], q, base, **dict(good, **over))
    bad = c['choice'][0].copy()
    bad[0, 1] = c['n'][1]                       # the first padding column of row 1 (or past the block)
    for ch in (bad, -np.ones_like(bad), c['choice'][0][:, :3], np.zeros((0, 5), np.int64)):
        with pytest.raises(ValueError):
            ops.alpha_reinforce_step(prob, m, v, pg, ch, q[:len(ch)], base, **good)
    with pytest.raises(ValueError):
        ops.alpha_reinforce_step(prob, m, v, pg, c['choice'][0], q[:3], base, **good)
    # the loop's checks come before it builds anything (a toy module stands in for the supernet)
    net = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match='reinforce_samples'):
        SearchLoop(net, arch_mode='reinforce', reinforce_samples=0)
    for reward in (None, NegLossReward(torch.nn.MSELoss())):
        with pytest.raises(ValueError, match='rewards cost'):
            SearchLoop(net, arch_mode='reinforce', reward=reward, reward_form='mul', cost_table=torch.ones(2, 2), cost_weight=-0.07)
    with pytest.raises(ValueError, match="'full' or 'two'"):
        SearchLoop(net, arch_mode='three')
    sn = _build(cases.net_case('vqa', None, 4343, search=True))
    with pytest.raises(ValueError, match='n_samples'):
        ArchAdam(sn, mode='reinforce', n_samples=0)
    opt = ArchAdam(sn, mode='reinforce', n_samples=3)
    with pytest.raises(ValueError, match='one per sample'):
        reinforce_arch_step(sn, opt, lambda p, t: p, None, None, plan=[[], []])
    loss = torch.nn.MSELoss(reduction='sum')
    r = NegLossReward(loss, scale=0.25)(torch.ones(4), torch.zeros(4))
    assert float(r) == -1.0


# ---- two gloo processes ------------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    """Stands in for the supernet's forward, which has no CPU path: the real Net_Search owns the alphas, the sampler and the
    sampled indices; the prediction depends on the sample through a fixed table."""

    def __init__(self, net):
        super().__init__()
        self.net = net
        g = torch.Generator().manual_seed(5)
        self.table = torch.rand(len(net.redundant_modules), 8, generator=g)

    def forward(self, x):
        s = sum(self.table[i, m.active_index[0]] for i, m in enumerate(self.net.redundant_modules))
        return x * s / len(self.net.redundant_modules)


class _ToySupernet:
    """reinforce_arch_step's view of a network: the supernet's own sampling and alpha block, the toy's forward."""

    def __init__(self, net):
        self.net, self.toy = net, _Toy(net)

    def __getattr__(self, k):
        return getattr(self.__dict__['net'], k)

    def __call__(self, x):
        return self.toy(x)


def _reward(pred, target):
    return 1.0 / (1.0 + ((pred - target) ** 2).mean())


def _shard(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return torch.randn(6, 5, generator=g), torch.randn(6, 5, generator=g)


def _three_steps(reducer, shards):
    from mmnas_amd.model import mixed
    from mmnas_amd.harness import ArchAdam, reinforce_arch_step
    net = _ToySupernet(_build(cases.net_case('vqa', None, 3, search=True, HSIZE=64)))
    opt = ArchAdam(net, 0.1, (0.0, 0.999), mode='reinforce', n_samples=4, baseline_decay=0.9)
    mixed.seed_arch_sampler(888)
    qs = []
    for _ in range(3):
        if len(shards) == 1:
            reinforce_arch_step(net, opt, _reward, *shards[0], reducer=reducer)
        else:       # one process fed the mean of the ranks' qualities: same samples on every shard, then one update
            state = mixed._sampler.get_state()
            per = []
            for x, t in shards:
                mixed._sampler.set_state(state)
                reinforce_arch_step(net, opt, _reward, x, t, optimize=False)
                per.append(opt.quality.clone())
            opt.quality.copy_((per[0] + per[1]) * 0.5)
            opt.step()
        qs.append(opt.quality.clone())
    return net._flat_alphas()[0].clone(), opt.baseline.clone(), qs


def _w_reinforce(rank):
    from mmnas_amd import dp
    net = _build(cases.net_case('vqa', None, 3, search=True, HSIZE=64))
    red = dp.SupernetReducer(net)
    assert red.comm
    alphas, base, qs = _three_steps(red, [_shard(rank)])
    both = [torch.zeros_like(alphas) for _ in range(2)]
    dist.all_gather(both, alphas)
    assert torch.equal(both[0], both[1]), 'the ranks\' alphas differ'
    bases = [torch.zeros_like(base) for _ in range(2)]
    dist.all_gather(bases, base)
    assert torch.equal(bases[0], bases[1])
    want_a, want_b, want_q = _three_steps(None, [_shard(0), _shard(1)])
    assert torch.equal(alphas, want_a) and torch.equal(base, want_b), (alphas - want_a).abs().max()
    assert all(torch.equal(a, b) for a, b in zip(qs, want_q))
    fresh = _build(cases.net_case('vqa', None, 3, search=True, HSIZE=64))._flat_alphas()[0]
    assert not torch.equal(alphas, fresh), 'three updates moved nothing'


def _entry(rank, port):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=2)
    try:
        _w_reinforce(rank)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_on_different_shards_keep_identical_alphas():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_entry, args=(port,), nprocs=2, join=True)
