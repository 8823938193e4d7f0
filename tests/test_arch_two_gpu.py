"""The fused ALPHA_BINARY_MODE 'two' architecture update on the GPU:
  * mmnas_alpha_two_step against its torch restatement run in float64 on the CPU over the same inputs (ops.alpha_two_step
    takes CPU tensors through that restatement), with the conservation of each pair's probability mass, repeatability and
    the entry's edge cases;
  * tests/golden/arch_two.npz -- the reference's own statements (make_golden_arch_two.py) -- replayed through the kernel;
  * SearchLoop(arch_mode='two', fused_arch_update=True) in lockstep with the torch-Adam loop; the default stays torch Adam.

Bounds: 1e-5 (tests/util.rel_err) is the project's bar for alphas between two paths (tests/test_harness_gpu.py); the gate
gradients keep |g_i - g_j| >= 0.1 on every sampled pair, because with beta1 = 0 Adam moves by +-lr whatever the gradient's
size and a pair gradient near zero would leave the sign to float32 rounding.

When MMNAS_ARCH_TWO_STATS names a file, the worst errors met are written there at the end of the module
(profiles/r09_arch_two_error_stats.json is one such run)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_arch_two_host import MIN_GAP, SETTINGS, TOL, fin, replay_arch_two
from tests.util import load, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy
EPS = 1e-8

ERR = {}     # label -> worst error met


def _note(label, e):
    ERR[label] = max(ERR.get(label, 0.0), float(e))


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_ARCH_TWO_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


def _case(rows, width, steps, seed):
    """Ragged rows (n_choices in 2..width, the rest -inf), per step one pair per row inside its n_choices and gate
    gradients with |g_i - g_j| >= MIN_GAP on the pair."""
    rs = np.random.RandomState(seed)
    n = rs.randint(2, width + 1, size=rows)
    n[0] = width                                            # the block's width is used
    a = (0.5 * rs.standard_normal((rows, width))).astype(np.float32)
    a[np.arange(width)[None, :] >= n[:, None]] = -np.inf
    pairs = np.zeros((steps, rows, 2), np.int64)
    gg = np.zeros((steps, rows, width), np.float32)
    for t in range(steps):
        for r in range(rows):
            i, j = (int(x) for x in rs.choice(n[r], size=2, replace=False))
            while True:
                g = rs.uniform(-1.0, 1.0, n[r]).astype(np.float32)
                if abs(float(g[i]) - float(g[j])) >= MIN_GAP:
                    break
            pairs[t, r] = (i, j)
            gg[t, r, :n[r]] = g
    return n, a, pairs, gg


def _pair_lse(prob, pairs):
    idx = torch.as_tensor(pairs)
    return torch.logsumexp(prob.detach().cpu().double().gather(1, idx), dim=1)


# 1 x 2; the supernet's own block; a last row alone in a second 64-thread workgroup; the entry's limit
SHAPES = ((1, 2), (30, 5), (65, 4), (128, 5))


@pytest.mark.parametrize('rows,width', SHAPES, ids=lambda x: str(x))
def test_kernel_vs_the_float64_restatement_and_pair_mass_conservation(rows, width):
    from mmnas_amd import ops
    steps = 4
    n, a0, pairs, gg = _case(rows, width, steps, 100 + rows)
    pad = np.arange(width)[None, :] >= n[:, None]
    for s, (lr, betas, wd) in enumerate(SETTINGS):
        # one spare row behind the block on the device: the kernel must leave it alone
        whole = [torch.zeros(rows + 1, width, device=DEV) for _ in range(4)]
        prob, m, v, pg = (w[:rows] for w in whole)
        prob.copy_(T(a0))
        whole[0][rows] = 3.0
        whole[3][rows] = 3.0
        ref = dict(alpha=T(a0).double(), m=torch.zeros(rows, width, dtype=torch.float64),
                   v=torch.zeros(rows, width, dtype=torch.float64), prob_grad=torch.zeros(rows, width, dtype=torch.float64))
        for t in range(steps):
            pl = [tuple(int(x) for x in p) for p in pairs[t]]
            lse_before = _pair_lse(prob, pairs[t])
            ops.alpha_two_step(prob, T(gg[t]).to(DEV), m, v, pg, pl, lr, betas, EPS, t + 1, weight_decay=wd)
            ops.alpha_two_step(ref['alpha'], T(gg[t]).double(), ref['m'], ref['v'], ref['prob_grad'], pl, lr, betas, EPS, t + 1,
                               weight_decay=wd)
            got = dict(alpha=prob, m=m, v=v, prob_grad=pg)
            for name in ('alpha', 'm', 'v', 'prob_grad'):
                e = rel_err(fin(got[name].cpu().numpy()), fin(ref[name].numpy()))
                _note('kernel|%s' % name, e)
                print('rows %d width %d setting %d step %d %s: %.3g' % (rows, width, s, t + 1, name, e))
                assert e < TOL, (rows, width, s, t, name, e)
            drift = float((_pair_lse(prob, pairs[t]) - lse_before).abs().max())
            _note('kernel|pair_logsumexp_drift_abs', drift)
            print('rows %d width %d setting %d step %d pair logsumexp drift: %.3g' % (rows, width, s, t + 1, drift))
            assert drift < 1e-6, (rows, width, s, t, drift)
            a = prob.cpu().numpy()
            assert np.all(np.isneginf(a[pad])) and np.all(np.isfinite(a[~pad])), 'padding columns stay -inf'
            assert not m.cpu().numpy()[pad].any() and not v.cpu().numpy()[pad].any(), 'padding moments stay untouched'
            outside = ~pad
            outside[np.arange(rows), pairs[t, :, 0]] = False
            outside[np.arange(rows), pairs[t, :, 1]] = False
            assert not pg.cpu().numpy()[outside].any(), 'the gradient is zero outside the pair'
        for k, w in enumerate(whole):
            assert bool((w[rows] == (3.0 if k in (0, 3) else 0.0)).all()), 'a row behind the block was written'


def test_same_inputs_give_the_same_bits_and_prob_grad_is_optional():
    from mmnas_amd import ops
    rows, width = 65, 4
    _, a0, pairs, gg = _case(rows, width, 1, 7)
    pl = [tuple(int(x) for x in p) for p in pairs[0]]
    g = T(gg[0]).to(DEV)
    out = []
    for with_pg in (True, True, False):
        prob, m, v = T(a0.copy()).to(DEV), torch.zeros(rows, width, device=DEV), torch.zeros(rows, width, device=DEV)
        pg = torch.full((rows, width), 5.0, device=DEV) if with_pg else None      # (written, not accumulated)
        ops.alpha_two_step(prob, g, m, v, pg, pl, 0.1, (0.5, 0.999), EPS, 3, weight_decay=1e-3)
        out.append((prob, m, v, pg))
    for k in range(3):
        assert torch.equal(out[0][k], out[1][k]) and torch.equal(out[0][k], out[2][k]), k
    assert torch.equal(out[0][3], out[1][3]) and out[2][3] is None
    assert float(out[0][3].abs().max()) < 5.0


def test_entry_edge_cases_launch_nothing():
    from mmnas_amd import _lib as L
    from mmnas_amd import ops
    lib = L.lib()
    rows, width = 129, 4
    bufs = [torch.full((rows, width), 2.0, device=DEV) for _ in range(5)]
    arr = (ctypes.c_int * (2 * rows))(*([0, 1] * rows))

    def call(n_rows, pair_arr, step=1):
        return lib.mmnas_alpha_two_step(*[L.fptr(b) for b in bufs], n_rows, width, pair_arr, 0.1, 0.0, 0.999, EPS, 0.0, step, L.stream())

    assert call(129, arr) == -1 and b'rows=129' in lib.mmnas_last_error()          # MMNAS_E_SHAPE
    assert call(0, arr) == 0 and call(0, None) == 0                                # rows == 0: OK
    bad = (ctypes.c_int * 4)(0, 1, 2, 2)
    assert call(2, bad) == -2 and call(2, arr, step=0) == -2                       # i == j; step < 1
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == 2.0).all()), 'a refused call wrote to a buffer'
    with pytest.raises(ValueError):
        ops.alpha_two_step(*bufs, [(0, 1)] * rows, 0.1, (0.0, 0.999), EPS, 1)
    empty = [torch.zeros(0, width, device=DEV) for _ in range(5)]
    ops.alpha_two_step(*empty, [], 0.1, (0.0, 0.999), EPS, 1)
    with pytest.raises(L.MMNasHipError):                                           # float64 on the device: no silent torch path
        ops.alpha_two_step(*[b[:2].double() for b in bufs], [(0, 1)] * 2, 0.1, (0.0, 0.999), EPS, 1)


@pytest.mark.parametrize('s', [0, 1, 2])
def test_kernel_replays_the_reference_recording(s):
    worst = replay_arch_two(load('arch_two.npz'), s, dev=DEV)
    for name, e in worst.items():
        _note('golden|%s' % name, e)
    print('setting', s, 'worst errors', worst)


def _build(cls, c):
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def _plan_list(plan):
    return plan['enc'] + plan['dec']


def _alphas(net):
    return net._flat_alphas()[0].detach().cpu().numpy()


def _alpha_grads(net):
    w = net._flat_alphas()[0].shape[1]
    return np.stack([np.pad(m.alpha_prob.grad.cpu().numpy(), (0, w - m.n_choices)) for m in net.redundant_modules])


def test_search_loop_fused_update_in_lockstep_with_the_torch_adam_loop():
    """Two arch steps with different pairs.  Each loop runs its own forward, backward and update through arch_step(); the
    backward adds the gate gradients with float atomics (tests/test_sgd_gpu.py says why two runs need not repeat bit for
    bit), so right before the fused update reads its gate-gradient block it takes the torch loop's."""
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import _lib as L
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c = cases.net_case('vqa', None, 4343, search=True)
    rs = np.random.RandomState(8)
    plans = [_plan_list(cases.search_plan(rs, 'two')) for _ in range(2)]
    assert plans[0] != plans[1]
    inp = tuple(T(a).to(DEV) for a in c['inputs']); tgt = T(c['target']).to(DEV)
    fused = SearchLoop(_build(Net_Search, c), arch_mode='two', fused_arch_update=True)
    ref = SearchLoop(_build(Net_Search, c), arch_mode='two')
    lib = L.lib()
    real = lib.mmnas_alpha_two_step
    launches = []
    try:
        assert isinstance(fused.alpha_optim, ArchAdam) and fused.alpha_optim.mode == 'two'
        assert isinstance(ref.alpha_optim, torch.optim.Adam)
        lib.mmnas_alpha_two_step = lambda *a: (launches.append(a[5]), real(*a))[1]
        fused.net.reset_binary_gates()                        # fills the sampling cache from the initial alphas
        cached = fused.net._probs_cache[1].clone()
        initial = _alphas(fused.net).copy()
        step = fused.alpha_optim.step

        def step_on_the_torch_loops_gate_gradients():
            fused.net._flat_grads[0].copy_(ref.net._flat_grads[0])
            step()
        fused.alpha_optim.step = step_on_the_torch_loops_gate_gradients
        for k, plan in enumerate(plans):
            loss_r = float(ref.arch_step(inp, tgt, plan=plan).detach())
            loss_f = float(fused.arch_step(inp, tgt, plan=plan).detach())
            assert MixedOp.MODE is None
            assert abs(loss_f - loss_r) < 1e-5 * abs(loss_r), (k, loss_f, loss_r)
            gg = ref.net._flat_grads[0].cpu().numpy()
            assert float(np.abs(gg).max()) > 0
            e_a = rel_err(fin(_alphas(fused.net)), fin(_alphas(ref.net)))
            e_g = rel_err(_alpha_grads(fused.net), _alpha_grads(ref.net))
            _note('loop|alpha', e_a)
            _note('loop|alpha_prob.grad', e_g)
            print('arch step', k, 'loss', loss_f, loss_r, 'alpha', e_a, 'alpha_prob.grad', e_g)
            assert e_a < 1e-5 and e_g < 1e-4, (k, e_a, e_g)
        assert launches == [30, 30] and fused.alpha_optim.steps == 2       # one launch per update, all nodes in it
        for m in fused.net.redundant_modules:
            assert m._two_snapshot is None                                 # the per-node statements did not run
        assert float(np.abs(fin(_alphas(fused.net)) - fin(initial)).max()) > 0.05       # the alphas did move
        # the next sampling sees the new alphas: the update dropped the cached probabilities
        fused.net.reset_binary_gates()
        now = fused.net._probs_cache[1]
        assert torch.equal(now, torch.softmax(fused.net._flat_alphas()[0].detach(), dim=1).cpu())
        assert not torch.equal(now, cached)
    finally:
        lib.mmnas_alpha_two_step = real
        MixedOp.MODE = None
        for loop in (fused, ref):
            loop.reducer.fg.disable_sinks()


def test_default_keeps_torch_adam_and_full_mode_ignores_the_keyword():
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas_amd.harness import ArchAdam, SearchLoop
    c = cases.net_case('vqa', None, 77, search=True, HSIZE=64)
    for kw, mode, kind in ((dict(arch_mode='two'), None, torch.optim.Adam),
                           (dict(arch_mode='two', fused_arch_update=False), None, torch.optim.Adam),
                           (dict(arch_mode='two', fused_arch_update=True, alpha_weight_decay=1e-3), 'two', ArchAdam),
                           (dict(arch_mode='full', fused_arch_update=True), 'full', ArchAdam),
                           (dict(), 'full', ArchAdam)):
        loop = SearchLoop(_build(Net_Search, c), **kw)
        try:
            assert type(loop.alpha_optim) is kind, kw
            if mode:
                assert loop.alpha_optim.mode == mode
            if kw.get('alpha_weight_decay'):
                assert loop.alpha_optim.weight_decay == 1e-3
        finally:
            loop.reducer.fg.disable_sinks()
