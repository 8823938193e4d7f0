"""The NET_OPTIM = 'sgd' path on the GPU:
  * mmnas_sgd_step against torch.optim.SGD + clip_grad_norm_ run in float64 on the CPU over the same tensors;
  * optim.FlatSGD: 'zero' / 'skip' handling of absent gradients, checkpoints in torch.optim.SGD's own format both ways;
  * tests/golden/traj_sgd.npz -- the reference's own loop with its 'sgd' branch (make_golden_sgd.py) -- replayed through
    SearchLoop(net_optim='sgd') = SupernetReducer + FlatSGD + CosineSchedule + ArchAdam with alpha weight decay;
  * SearchLoop's new keywords at their defaults change nothing.

When MMNAS_SGD_STATS names a file, the worst errors met are written there at the end of the module
(profiles/r08_sgd_error_stats.json is one such run)."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.golden.cases_sgd import SGD_HYPER, SGD_WEIGHT_PLANS
from tests.util import TOL, esample, load, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy

ERR = {}     # label -> worst error met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_SGD_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
# (n, element offset of p / g / buf inside their allocations): the float4 body alone, body + a tail of 1, 2, 3 elements,
# a misaligned start (all three pointers; the gradient alone), n < 4
SIZES = ((1 << 16, (0, 0, 0)), (4096 + 1, (0, 0, 0)), (4096 + 2, (0, 0, 0)), ((1 << 16) + 3, (0, 0, 0)), (1027, (1, 1, 1)),
         (4100, (0, 3, 0)), (3, (0, 0, 0)), (1, (0, 0, 0)), (2, (1, 0, 0)))
GRID = [dict(momentum=m, weight_decay=wd, clip=cl, nesterov=False, dampening=0.0)
        for m, wd, cl in itertools.product((0.0, 0.9), (0.0, 1e-4), (None, 'above', 'below'))]
GRID.append(dict(momentum=0.9, weight_decay=1e-4, clip='above', nesterov=True, dampening=0.0))
GRID.append(dict(momentum=0.9, weight_decay=1e-4, clip='above', nesterov=False, dampening=0.1))


@pytest.mark.parametrize('hp', GRID, ids=lambda h: 'm%g_wd%g_clip-%s%s%s' % (h['momentum'], h['weight_decay'], h['clip'],
                                                                              '_nesterov' if h['nesterov'] else '',
                                                                              '_damp%g' % h['dampening'] if h['dampening'] else ''))
def test_sgd_step_kernel_vs_torch_sgd_in_float64(hp):
    from mmnas_amd import _lib as L
    lib = L.lib()
    g = torch.Generator().manual_seed(11)
    lr, mom = 0.05, hp['momentum']
    for n, (op, og, ob) in SIZES:
        p0 = torch.randn(n, generator=g)
        P, G, B = (torch.zeros(n + 8, device=DEV) for _ in range(3))
        p, gr, buf = P[op:op + n], G[og:og + n], B[ob:ob + n]
        p.copy_(p0)
        ref = torch.nn.Parameter(p0.double())
        ropt = torch.optim.SGD([ref], lr, momentum=mom, dampening=hp['dampening'], weight_decay=hp['weight_decay'],
                               nesterov=hp['nesterov'])
        sumsq = torch.zeros(1, device=DEV)
        for step in range(5):
            grad = torch.randn(n, generator=g) * (0.5 + step)
            gr.copy_(grad)
            ref.grad = grad.double()
            sumsq_ptr, max_norm = None, 0.0
            if hp['clip']:
                norm = float(grad.double().norm())
                max_norm = norm * (0.5 if hp['clip'] == 'above' else 2.0)       # the norm lies above / below max_norm
                torch.nn.utils.clip_grad_norm_([ref], max_norm)
                sumsq.zero_()
                L.check(lib.mmnas_sumsq(L.fptr(gr), n, L.fptr(sumsq), L.stream()))
                sumsq_ptr = L.fptr(sumsq)
            ropt.step()
            L.check(lib.mmnas_sgd_step(L.fptr(p), L.fptr(gr), L.fptr(buf) if mom else None, n, lr, mom, hp['dampening'],
                                       hp['weight_decay'], int(hp['nesterov']), int(step == 0), sumsq_ptr, max_norm, L.stream()))
            ep = rel_err(p.cpu().numpy(), ref.detach().numpy())
            _note('kernel|param', ep)
            assert ep < TOL, (n, step, 'param', ep)
            if mom:
                eb = rel_err(buf.cpu().numpy(), ropt.state[ref]['momentum_buffer'].numpy())
                _note('kernel|momentum_buffer', eb)
                assert eb < TOL, (n, step, 'buf', eb)
            else:
                assert not bool(B.any()), 'momentum == 0 must not touch the buffer'
        # nothing outside [0, n) was written
        for whole, o in ((P, op), (B, ob)):
            assert not bool(whole[:o].any()) and not bool(whole[o + n:].any()), (n, 'out-of-range write')
    print('worst so far', ERR)


def test_sgd_step_zero_buffer_is_torchs_first_step_without_dampening():
    """dampening == 0: a zero-filled buffer with first == 0 gives bit for bit what first == 1 gives (FlatSGD relies on
    neither; a caller of the C entry may)."""
    from mmnas_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    n = 4099
    p0, gr = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    out = []
    for first in (0, 1):
        p, buf = p0.clone(), torch.zeros(n, device=DEV)
        L.check(L.lib().mmnas_sgd_step(L.fptr(p), L.fptr(gr), L.fptr(buf), n, 0.05, 0.9, 0.0, 1e-4, 0, first, None, 0.0, L.stream()))
        out.append((p, buf))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------------------------------
# FlatSGD
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(33, 17), (5,), (64, 64), (7, 3)]


def _feed(ps, ref, grads, mode):
    """Hand `grads` (index -> tensor) to both sides; the others get None here and, on the torch side, zeros ('zero' mode:
    the reference loop's `0 * sum` lines) or None ('skip')."""
    for i in range(len(ps)):
        if i in grads:
            if ps[i].grad is None:
                ps[i].grad = grads[i].to(DEV)                     # a stray gradient outside the flat buffer
            else:
                ps[i].grad.copy_(grads[i].to(DEV))
            ref[i].grad = grads[i].double()
        else:
            ps[i].grad = None
            ref[i].grad = torch.zeros_like(ref[i]) if mode == 'zero' else None


@pytest.mark.parametrize('mode', ['zero', 'skip'])
def test_flat_sgd_absent_gradients(mode):
    """'zero' is torch SGD fed explicit zero gradients -- a parameter without a gradient keeps moving on its momentum
    buffer and under weight decay; 'skip' is torch SGD fed None -- parameter and buffer stay bit for bit as they were."""
    from mmnas_amd.optim import FlatSGD
    g = torch.Generator().manual_seed(1)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    ref = [torch.nn.Parameter(t.clone().double()) for t in init]
    opt = FlatSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-4, absent_grads=mode)
    ropt = torch.optim.SGD(ref, lr=0.05, momentum=0.9, weight_decay=1e-4)
    assert opt.state_dict()['state'] == {}
    for step in range(5):
        live = [0, 1, 2, 3] if step == 0 else ([0, 2] if step % 2 else [1, 2, 3])
        if mode == 'skip' and step == 0:
            live = [0, 1, 2]              # parameter 3 meets its first gradient later than the others: its own first step
        opt.zero_grad()
        grads = {i: torch.randn(SHAPES[i], generator=g) for i in live}
        _feed(ps, ref, grads, mode)
        before = [(p.detach().clone(), opt.buf[o:o + p.numel()].clone()) for p, o in zip(ps, opt.fg.offsets)]
        tot = float(torch.sqrt(sum((gr.double() ** 2).sum() for gr in grads.values())))
        torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], 0.5)
        opt.step(max_norm=0.5)
        ropt.step()
        assert abs(opt.grad_norm() - tot) < 1e-4 * tot
        for i in range(4):
            e = rel_err(ps[i].detach().cpu().numpy(), ref[i].detach().numpy())
            _note('flat_sgd|%s|param' % mode, e)
            assert e < TOL, (mode, step, i, e)
            o, n = opt.fg.offsets[i], ps[i].numel()
            if i in live or mode == 'zero':
                if step > 0 and i not in live:
                    assert not torch.equal(ps[i].detach(), before[i][0]), 'zero mode: the parameter keeps moving'
                eb = rel_err(opt.buf[o:o + n].cpu().numpy(), ropt.state[ref[i]]['momentum_buffer'].reshape(-1).numpy())
                _note('flat_sgd|%s|momentum_buffer' % mode, eb)
                assert eb < TOL, (mode, step, i, eb)
            else:
                assert torch.equal(ps[i].detach(), before[i][0]) and torch.equal(opt.buf[o:o + n], before[i][1]), (step, i)
        assert set(opt.state_dict()['state']) == {i for i, r in enumerate(ref) if 'momentum_buffer' in ropt.state[r]}


def test_flat_sgd_checkpoints_interchange_with_torch_sgd():
    from mmnas_amd.optim import CosineSchedule, FlatSGD
    g = torch.Generator().manual_seed(2)
    init = [torch.randn(s, generator=g) for s in SHAPES]
    hp = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)

    def grads():
        return [torch.randn(s, generator=g) for s in SHAPES]

    ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
    opt = FlatSGD(ps, **hp)
    want_keys = set(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], **hp).state_dict()['param_groups'][0])
    assert set(opt.state_dict()['param_groups'][0]) == want_keys
    for _ in range(2):
        opt.zero_grad()
        for p, gr in zip(ps, grads()):
            p.grad.copy_(gr.to(DEV))
        opt.step()
    # (a) FlatSGD -> torch SGD over clones
    sd = opt.state_dict()
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    topt = torch.optim.SGD(clones, lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]['momentum'] == 0.9 and topt.param_groups[0]['lr'] == 0.05
    assert set(topt.state_dict()['param_groups'][0]) == want_keys
    gs = grads()
    opt.zero_grad()
    for p, c, gr in zip(ps, clones, gs):
        p.grad.copy_(gr.to(DEV))
        c.grad = gr.clone()
    opt.step()
    topt.step()
    for p, c in zip(ps, clones):
        e = rel_err(p.detach().cpu().numpy(), c.detach().numpy())
        _note('checkpoint|to_torch', e)
        assert e < TOL
    # (b) torch SGD -> a fresh FlatSGD built with other settings; with a schedule attached 'initial_lr' travels too
    torch.optim.lr_scheduler.CosineAnnealingLR(topt, 10, eta_min=0.001)
    tsd = topt.state_dict()
    assert tsd['param_groups'][0]['initial_lr'] == 0.05
    ps2 = [torch.nn.Parameter(c.detach().clone().to(DEV)) for c in clones]
    opt2 = FlatSGD(ps2, lr=1.0, momentum=0.5, weight_decay=0.0)
    opt2.load_state_dict(tsd)
    assert (opt2.momentum, opt2.weight_decay, opt2.param_groups[0]['lr'], opt2.param_groups[0]['initial_lr']) == (0.9, 1e-4, 0.05, 0.05)
    assert set(opt2.state_dict()['param_groups'][0]) == set(tsd['param_groups'][0])
    CosineSchedule(opt2, 10, eta_min=0.001, last_epoch=3)            # resumes: 'initial_lr' is there
    gs = grads()
    opt2.zero_grad()
    for p, c, gr in zip(ps2, clones, gs):
        p.grad.copy_(gr.to(DEV))
        c.grad = gr.clone()
    opt2.step()
    topt.step()
    for p, c in zip(ps2, clones):
        e = rel_err(p.detach().cpu().numpy(), c.detach().numpy())
        _note('checkpoint|from_torch', e)
        assert e < TOL
    # a file with buffers for some parameters only cannot be a 'zero'-mode loop's
    part = opt.state_dict()
    del part['state'][1]
    with pytest.raises(ValueError, match="absent_grads='skip'"):
        opt2.load_state_dict(part)
    opt3 = FlatSGD([torch.nn.Parameter(c.detach().clone().to(DEV)) for c in clones], absent_grads='skip', **hp)
    opt3.load_state_dict(part)
    assert opt3.has_buf == [True, False, True, True]


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own loop, 'sgd' branch
# ---------------------------------------------------------------------------------------------------------------------
def _build(cls, c):
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def _plan_list(plan):
    return plan['enc'] + plan['dec']


def _alphas(net):
    return np.stack([np.pad(m.alpha_prob.detach().cpu().numpy(), (0, 4 - m.n_choices)) for m in net.redundant_modules])


def test_sgd_trajectory_vs_reference_loop():
    """tests/golden/traj_sgd.npz replayed: scheduler step, w1, w2, scheduler step, w3, 'full' arch step with alpha weight
    decay, the forward loss of a further weight step.

    Parameter motion is compared per tensor at 2e-3 -- the whole-step gradient tolerance of test_harness_gpu.py, in its form
    `2e-3 * n + 1e-5 * top` (top: the snapshot's largest per-tensor motion) -- as |  ||mine - P0|| - ||gold - P0||  | for every
    tensor outside test_oracle_golden2's SHIFT_INVARIANT / NEAR_INVARIANT lists, and as the norm of the DIFFERENCE
    ||mine - gold|| for the tensors the golden stores in full (cases.TRAJ_FULL_KEYS) and for the strided samples of every
    tensor's motion (the floor scaled to the sample's share of the tensor).  SGD's motion is linear in the gradient: no
    allowance for stray coordinates, as check_trajectory needs for Adam, is made.

    The floor `1e-5 * top` is test_harness_gpu.py's.  It is 1.45e-7 / 3.4e-7 / 5.1e-7 at w1 / w2 / w3 in this golden, the
    size of one fp32 rounding of a parameter near 1 (2^-23 = 1.2e-7): both sides store fp32 parameters, so motion below
    that is not resolved by either.  It is the larger term -- the check is looser than 2e-3 relative -- for 439 / 364 / 268
    of the 635 compared tensors (median motion 5e-5 / 1.5e-4 / 3.3e-4), and exceeds the whole motion of one tensor at w1
    and w2 (4.9e-8, 1.4e-7), which is thereby unchecked there; the strided samples and the full tensors carry the same
    floor.  The large movers, where a wrong rate, momentum or decay shows, are held at 2e-3."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd.harness import SearchLoop
    from mmnas_amd.optim import CosineSchedule, FlatSGD
    from tests.test_oracle_golden2 import NEAR_INVARIANT, SHIFT_INVARIANT
    npz = load('traj_sgd.npz')
    c, c2, plans = cases.traj_setup()
    H = SGD_HYPER
    net = _build(Net_Search, c)
    loop = SearchLoop(net, net_lr=H['net_lr'], clip=H['clip'], alpha_lr=H['alpha_lr'], alpha_betas=H['alpha_betas'],
                      net_optim='sgd', net_momentum=H['net_momentum'], net_weight_decay=H['net_weight_decay'],
                      net_lr_min=H['net_lr_min'], max_epoch=H['max_epoch'], alpha_weight_decay=H['alpha_weight_decay'])
    try:
        assert isinstance(loop.net_optim, FlatSGD) and isinstance(loop.lr_scheduler, CosineSchedule)
        assert loop.net_optim.absent_grads == 'zero'
        inp = tuple(T(a).to(DEV) for a in c['inputs']); tgt = T(c['target']).to(DEV)
        inp2 = tuple(T(a).to(DEV) for a in c2['inputs']); tgt2 = T(c2['target']).to(DEV)
        net_keys = [k for k, _ in net.named_parameters() if 'alpha' not in k]
        named = dict(net.named_parameters())
        P0 = {k: T(c['P'][k]).double() for k in net_keys}
        losses, gnorms, lrs, snaps = [], [], [], {}
        w = [plans[i] for i in SGD_WEIGHT_PLANS]

        def weight_step(i):
            lrs.append(loop.net_optim.param_groups[0]['lr'])
            losses.append(float(loop.weight_step(inp, tgt, plan=_plan_list(w[i])).detach()))
            gnorms.append(loop.net_optim.grad_norm())
            snaps['w%d' % (i + 1)] = {k: named[k].detach().cpu().clone() for k in net_keys}

        loop.begin_epoch(0)
        weight_step(0)
        weight_step(1)
        loop.begin_epoch(1)
        weight_step(2)
        losses.append(float(loop.arch_step(inp2, tgt2, plan=_plan_list(plans[2])).detach()))
        gg, pg = net._flat_grads
        gate_grads, prob_grads, alpha_after = gg.cpu().numpy(), pg.cpu().numpy(), _alphas(net)
        snaps['a'] = {k: named[k].detach().cpu().clone() for k in net_keys}
        losses.append(float(loop.weight_step(inp, tgt, optimize=False, plan=_plan_list(w[3])).detach()))
    finally:
        loop.reducer.fg.disable_sinks()

    print('losses', losses, 'golden', npz['traj|losses'])
    print('grad norms', gnorms, 'golden', npz['traj|grad_norms'])
    print('lr', lrs, 'golden', npz['traj|lr'])
    e_alpha = rel_err(alpha_after, npz['traj|arch|alpha_after'])
    e_gate, e_prob = rel_err(gate_grads, npz['traj|arch|gate_grads']), rel_err(prob_grads, npz['traj|arch|prob_grads'])
    _note('traj|loss', max(abs(a - b) / abs(b) for a, b in zip(losses, npz['traj|losses'])))
    _note('traj|grad_norm', rel_err(np.array(gnorms), npz['traj|grad_norms']))
    _note('traj|gate_grads', e_gate); _note('traj|prob_grads', e_prob); _note('traj|alpha_after', e_alpha)
    # measure the motion before anything is asserted
    worst = {'delta_norm': (0.0, None), 'full_tensor': (0.0, None), 'delta_sample': (0.0, None)}
    fails = []
    for tag in ('w1', 'w2', 'w3', 'a'):
        keys = [str(k) for k in npz['traj|%s|keys' % tag]]
        dn, off, ds = npz['traj|%s|delta_norm' % tag], npz['traj|%s|delta_off' % tag], npz['traj|%s|delta_sample' % tag]
        assert set(keys) == set(snaps[tag])
        top = float(dn.max())
        for i, k in enumerate(keys):
            if k in SHIFT_INVARIANT or k in NEAR_INVARIANT:
                continue
            delta = snaps[tag][k].double() - P0[k]
            n = float(dn[i])
            checks = [('delta_norm', abs(float(delta.norm()) - n), 2e-3 * n + 1e-5 * top)]
            want = ds[off[i]:off[i + 1]].astype(np.float64)
            share = np.sqrt(want.size / delta.numel())
            checks.append(('delta_sample', float(np.linalg.norm(esample(delta.numpy()).astype(np.float64) - want)),
                           2e-3 * float(np.linalg.norm(want)) + 1e-5 * top * share))
            if k in cases.TRAJ_FULL_KEYS:
                gold = T(npz['traj|%s|P:%s' % (tag, k)])
                checks.append(('full_tensor', float((snaps[tag][k].double() - gold.double()).norm()),
                               2e-3 * float((gold.double() - P0[k]).norm()) + 1e-5 * top))
            for what, err, bound in checks:
                if err / bound > worst[what][0]:
                    worst[what] = (err / bound, '%s %s' % (tag, k))
                if err > bound:
                    fails.append((what, tag, k, err, bound))
    for what, (frac, where) in worst.items():
        print('motion: worst %s at %.3f of its bound (%s)' % (what, frac, where))
        _note('traj|motion|%s|worst_fraction_of_bound' % what, frac)

    for i, (a, b) in enumerate(zip(losses, npz['traj|losses'])):
        assert abs(a - b) <= 2e-4 * abs(b), ('loss', i, a, b)
    assert len(losses) == len(npz['traj|losses']) == 5
    assert rel_err(np.array(gnorms), npz['traj|grad_norms']) < 1e-3
    assert e_gate < 1e-3 and e_prob < 1e-3 and e_alpha < 1e-3, (e_gate, e_prob, e_alpha)
    assert np.abs(lrs - npz['traj|lr']).max() < 1e-12, (lrs, npz['traj|lr'])
    assert not fails, (len(fails), fails[:8])
    for k in snaps['a']:           # the arch step leaves the network weights alone
        assert torch.equal(snaps['a'][k], snaps['w3'][k]), k


def test_alpha_weight_decay_full_and_two_modes_match_torch_adam():
    """ALPHA_WEIGHT_DECAY: mode 'full' folds torch Adam's wd * alpha into the fused alpha update (mmnas_alpha_full_step_wd),
    mode 'two' hands it to torch Adam; ArchAdam's checkpoint reports and reads it."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam, SearchLoop
    g = torch.Generator().manual_seed(9)
    rows, width, wd = 30, 4, 1e-3
    a = torch.randn(rows, width, generator=g)
    a[:12, 2:] = float('-inf')
    prob = a.clone().to(DEV)
    m = torch.zeros_like(prob); v = torch.zeros_like(prob); pg = torch.zeros_like(prob)
    ps = [torch.nn.Parameter(a[i, :(2 if i < 12 else 4)].clone().double()) for i in range(rows)]
    opt = torch.optim.Adam(ps, 0.1, betas=(0.0, 0.999), weight_decay=wd)
    for step in (1, 2, 3):
        gg = torch.randn(rows, width, generator=g) * 1e-2          # small gradients: the decay term is a visible share
        gg[:12, 2:] = 0
        for i, p in enumerate(ps):
            gi = gg[i, :p.numel()].double()
            pr = torch.softmax(p.detach(), 0)
            p.grad = pr * (gi - (gi * pr).sum())
        opt.step()
        ops.alpha_full_step(prob, gg.to(DEV), m, v, pg, 0.1, (0.0, 0.999), 1e-8, step, weight_decay=wd)
        for i, p in enumerate(ps):
            n = p.numel()
            assert rel_err(pg[i, :n].cpu().numpy(), p.grad.numpy()) < 1e-5          # alpha_prob.grad stays undecayed
            e = rel_err(prob[i, :n].cpu().numpy(), p.detach().numpy())
            _note('alpha_wd|full', e)
            assert e < 1e-5
            assert bool(torch.all(torch.isinf(prob[i, n:]))), 'padding columns must stay -inf'
    c = cases.net_case('vqa', None, 77, search=True, HSIZE=64)
    for mode in ('full', 'two'):
        net = _build(Net_Search, c)
        loop = SearchLoop(net, arch_mode=mode, alpha_weight_decay=wd)
        try:
            sd = loop.alpha_optim.state_dict()
            assert sd['param_groups'][0]['weight_decay'] == wd
            if mode == 'full':
                fresh = ArchAdam(net)
                assert fresh.state_dict()['param_groups'][0]['weight_decay'] == 0
                fresh.load_state_dict(sd)
                assert fresh.weight_decay == wd
        finally:
            loop.reducer.fg.disable_sinks()


# the native entries the new keywords can reach: the weight optimizers, their clip scalar, the alpha update
REACHED = ('mmnas_sumsq', 'mmnas_adam_step', 'mmnas_sgd_step', 'mmnas_alpha_full_step', 'mmnas_alpha_full_step_wd')


def test_search_loop_new_keywords_at_their_defaults_change_nothing():
    """Two loops in one process, the new keywords absent and spelled at their defaults: both take the FlatAdam path and
    agree bit for bit -- losses, parameters, Adam moments, alphas -- on two weight steps + one arch step of traj_setup().

    The loops run in lockstep, because two runs of ONE configuration need not repeat bit for bit: the network backward
    (embedding, split-K products, column sums, relation bias) and the clip scalar (mmnas_sumsq) add with float atomics,
    whose order the hardware picks (test_grounding_gpu.py::test_flat_adam_step_after_an_evaluator_call_is_unchanged says
    the same of the backward).  What the atomics decide is therefore made common: after each backward the second loop
    takes the first's gradient buffer, and its clip scalar is overwritten with the first's before its Adam launch reads
    it.  Every loop still runs its own forward, its own backward and its own update through its own optimizer objects.
    Asserted bit for bit, unconditionally: each step's forward loss (both loops hold identical parameters when it is
    computed), parameters and both Adam moments after each weight step, alphas, alpha moments and alpha_prob.grad after
    the arch step, the network weights across the arch step.  Asserted exactly as well: which optimizer entries of the
    library each loop calls, in which order, with which scalar arguments."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd import _lib as L
    from mmnas_amd.harness import ArchAdam, SearchLoop
    from mmnas_amd.optim import FlatAdam, WarmupOptimizer
    c, c2, plans = cases.traj_setup()
    H = cases.TRAJ_HYPER
    base = dict(net_lr=H['net_lr'], net_betas=H['net_betas'], net_eps=H['net_eps'], clip=H['clip'], epoch_steps=H['epoch_steps'],
                warmup=True, alpha_lr=H['alpha_lr'], alpha_betas=H['alpha_betas'])
    spelled = dict(net_optim='wadam', net_momentum=0.9, net_weight_decay=0.0, net_lr_min=0.0005, max_epoch=None, start_epoch=0,
                   alpha_weight_decay=0.0)
    inp = tuple(T(a).to(DEV) for a in c['inputs']); tgt = T(c['target']).to(DEV)
    inp2 = tuple(T(a).to(DEV) for a in c2['inputs']); tgt2 = T(c2['target']).to(DEV)
    lib = L.lib()
    real = {name: getattr(lib, name) for name in REACHED}
    calls = ([], [])                 # per loop: (entry, its arguments that are no pointers)
    who = [0]
    opts, clip_scalars = [], []

    def spy(name):
        types = L.SYMBOLS[name][1]

        def call(*args):
            calls[who[0]].append((name, tuple(a for a, t in zip(args, types) if t is not L._fp)))
            rc = real[name](*args)
            if name == 'mmnas_sumsq' and who[0] == 1:             # one clip scalar for both updates (same stream: lands
                clip_scalars.append((opts[0]._sumsq.clone(), opts[1]._sumsq.clone()))     # before the Adam launch)
                opts[1]._sumsq.copy_(opts[0]._sumsq)
            return rc
        return call

    def on(k, fn, *a, **kw):
        who[0] = k
        return fn(*a, **kw)

    loops = []
    try:
        for name in REACHED:
            setattr(lib, name, spy(name))
        for extra in ({}, spelled):
            loop = SearchLoop(_build(Net_Search, c), **base, **extra)
            loops.append(loop)
            assert isinstance(loop.net_optim, WarmupOptimizer) and isinstance(loop.net_optim.optimizer, FlatAdam)
            assert loop.net_optim.optimizer.weight_decay == 0.0 and loop.lr_scheduler is None
            assert isinstance(loop.alpha_optim, ArchAdam) and loop.alpha_optim.weight_decay == 0
            loop.begin_epoch(0)                                   # 'wadam': nothing to do
        A, B = loops
        oa, ob = A.net_optim.optimizer, B.net_optim.optimizer
        opts.extend((oa, ob))
        assert torch.equal(oa.flat_p, ob.flat_p)
        losses = ([], [])
        for i in (0, 1):
            for k, loop in enumerate(loops):
                losses[k].append(float(on(k, loop.weight_step, inp, tgt, optimize=False, plan=_plan_list(plans[i])).detach()))
            for loop in loops:
                loop.reducer.fg.adopt_strays()                    # (the step would do it; nothing may land after the copy)
            B.reducer.fg.flat.copy_(A.reducer.fg.flat)            # one backward's gradients for both updates
            for k, loop in enumerate(loops):
                on(k, loop._net_step)
            torch.cuda.synchronize()
            assert A.net_optim._step == B.net_optim._step == i + 1
            assert A.net_optim.optimizer.param_groups[0]['lr'] == B.net_optim.optimizer.param_groups[0]['lr']
            assert len(clip_scalars) == i + 1 and torch.equal(oa._sumsq, ob._sumsq)
            print('weight step', i, 'losses', losses[0][-1], losses[1][-1], 'own clip scalars', [float(x) for x in clip_scalars[-1]])
            assert losses[0][-1] == losses[1][-1], (i, losses)
            for what in ('flat_p', 'm', 'v'):
                assert torch.equal(getattr(oa, what), getattr(ob, what)), (i, what)
        before = [o.flat_p.clone() for o in (oa, ob)]
        for k, loop in enumerate(loops):
            losses[k].append(float(on(k, loop.arch_step, inp2, tgt2, optimize=False, plan=_plan_list(plans[2])).detach()))
        for ma, mb in zip(A.net.redundant_modules, B.net.redundant_modules):
            assert (ma.alpha_gate.grad is None) == (mb.alpha_gate.grad is None)
            if ma.alpha_gate.grad is not None:
                mb.alpha_gate.grad.copy_(ma.alpha_gate.grad)      # one backward's gate gradients for both updates
        for k, loop in enumerate(loops):
            on(k, loop.alpha_optim.step)
        torch.cuda.synchronize()
        print('losses', losses[0], losses[1])
        assert losses[0] == losses[1], losses
        assert torch.equal(A.net._flat_alphas()[0], B.net._flat_alphas()[0])
        assert torch.equal(A.alpha_optim.m, B.alpha_optim.m) and torch.equal(A.alpha_optim.v, B.alpha_optim.v)
        assert torch.equal(A.net._flat_grads[1], B.net._flat_grads[1])
        assert A.alpha_optim.steps == B.alpha_optim.steps == 1
        for o, b in zip((oa, ob), before):
            assert torch.equal(o.flat_p, b), 'the arch step moved network weights'
        # the same entries in the same order with the same scalars; the parent's entries, with no decay
        assert calls[0] == calls[1], (calls[0], calls[1])
        assert [n for n, _ in calls[0]] == ['mmnas_sumsq', 'mmnas_adam_step'] * 2 + ['mmnas_alpha_full_step']
        for n, scalars in calls[0]:
            if n == 'mmnas_adam_step':
                assert scalars[5] == 0.0, scalars                 # (n, lr, beta1, beta2, eps, weight_decay, max_norm, step)
    finally:
        for name in REACHED:
            setattr(lib, name, real[name])
        for loop in loops:
            loop.reducer.fg.disable_sinks()


def test_begin_epoch_checks_its_epoch_and_a_replaced_net_optim_is_the_one_stepped():
    """begin_epoch(epoch) raises for an epoch skipped or begun twice (fresh and resumed schedules count differently, as
    CosineAnnealingLR's do); weight_step steps whatever `loop.net_optim` is when it runs."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd.harness import SearchLoop
    c = cases.net_case('vqa', None, 77, search=True, HSIZE=64)
    for start in (0, 4):
        loop = SearchLoop(_build(Net_Search, c), net_optim='sgd', net_lr=0.05, max_epoch=10, start_epoch=start)
        try:
            loop.begin_epoch(start)
            first = loop.net_optim.param_groups[0]['lr']
            with pytest.raises(ValueError):
                loop.begin_epoch(start)            # begun twice
            with pytest.raises(ValueError):
                loop.begin_epoch(start + 2)        # one skipped
            assert loop.net_optim.param_groups[0]['lr'] == first, 'a refused call must not move the schedule'
            loop.begin_epoch(start + 1)
            loop.begin_epoch()                     # no epoch given: nothing to check
            assert loop.net_optim.param_groups[0]['lr'] < first
            if start == 0:
                class Counting:
                    n = 0

                    def step(self):
                        self.n += 1
                loop.net_optim = Counting()
                loop._net_step()
                assert loop.net_optim.n == 1
        finally:
            loop.reducer.fg.disable_sinks()
