"""The ragged language stream (ops.set_unpad_x: LSTM, encoder, guided keys and attflat_x on the valid tokens only) against the
padded run of the same net, weights and inputs.  The padding tokens follow the valid ones, are masked as keys in every encoder
self-attention and every guided attention and dropped by attflat_x's mask, so logits and every parameter gradient must agree to
the bars the ragged decoder stream is held to (tests/test_chain_gpu.py::_same): outputs rel_err < 2e-6, parameter gradients
within 4e-5 (supernets) / 1e-4 (Net_Full) of the parameter's largest entry, relation-path keys at REL_PATH_SELF_TOL, floors of
1e-3 / 3e-3 of the net's largest gradient.

MMNAS_UNPAD_X_STATS=<file> writes the worst error per case there (profiles/r15_unpad_x_error_stats.json is one such run)."""
import atexit
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import REL_PATH_SELF_TOL, is_rel_path, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy
LENS = (1, 5, 16, 17, 20)       # B = 5 under Sx = 23: T' = 20, packed
STATS = {}


@atexit.register
def _write_stats():
    path = os.environ.get('MMNAS_UNPAD_X_STATS')
    if path and STATS:
        with open(path, 'w') as f:
            json.dump(STATS, f, indent=1, sort_keys=True)


def _case(task, arch, search, lengths, Sx, Sy, HSIZE, pad_regions, hole=None):
    B = len(lengths)
    c = cases.net_case(task, arch, 4243, search=search, B=B, Sx=Sx, Sy=Sy, HSIZE=HSIZE)
    frcn, bbox, y_rel, ques, x_rel = c['inputs']
    rs = np.random.RandomState(77)
    ques = rs.randint(1, c['token_size'], size=(B, Sx)).astype(np.int64)
    x_rel = rs.standard_normal((B, Sx, Sx, 3)).astype(np.float32)
    for b, n in enumerate(lengths):
        ques[b, n:] = 0
        x_rel[b, n:] = 0
        x_rel[b, :, n:] = 0
    if hole is not None:
        ques[hole] = 0
    if not pad_regions:      # ITM: every image carries all its regions
        frcn = np.maximum(rs.standard_normal(frcn.shape), 0).astype(np.float32)
        frcn[..., 0] += 0.05
        y_rel = rs.standard_normal(y_rel.shape).astype(np.float32)
    c['inputs'] = (frcn, bbox, y_rel, ques, x_rel)
    return c


def _run(task, arch, search, on, lengths=LENS, Sx=23, Sy=9, mode=None, plan=None, unpad=False, HSIZE=128, dropout=0.0,
         pad_regions=None, hole=None, count_small=False):
    """One forward + backward through the flat gradient buffer -> (outputs, gradients by name, what the chain was handed:
    one dict(packed, T, ragged_y) per BackboneFn call, the LSTM's step counts, launches of the one-launch operators)."""
    from mmnas_amd import _lib as L, dp, ops
    from mmnas.model.mixed import MixedOp
    if pad_regions is None:
        pad_regions = task != 'itm'
    c = _case(task, arch, search, lengths, Sx, Sy, HSIZE, pad_regions, hole)
    c['cfg'].DROPOUT_R = dropout
    mod = importlib.import_module('mmnas.model.%s_%s' % ('hygr' if search else 'full', task))
    cls = mod.Net_Search if search else mod.Net_Full
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    net = net.to(DEV).train()
    inp = tuple(T(a).to(DEV) for a in c['inputs'])
    tgt = T(c['target']).to(DEV)
    seen, steps = [], []
    o_apply, o_lstm = ops.BackboneFn.apply, ops.lstm
    # the language side's description is the APPENDED argument: a trailing ops.Ragged behind the parameter tensors
    ops.BackboneFn.apply = lambda *a: (seen.append(dict(packed=isinstance(a[-1], ops.Ragged), T=int(a[2].shape[-1]), ragged_y=a[10] is not None)),
                                       o_apply(*a))[1]
    ops.lstm = lambda x, m: (steps.append(int(x.shape[1])), o_lstm(x, m))[1]
    prev_x, prev_y = ops.set_unpad_x(on), ops.set_unpad(unpad)
    red, small = None, None
    arr = (L.ProfStat * len(L.K_NAMES))()
    if count_small:
        L.check(L.lib().mmnas_prof_enable(1))
    try:
        ops.manual_seed(99)
        if search:
            MixedOp.MODE = mode
            net.set_sampled(plan)
            red = dp.SupernetReducer(net)
            if mode is None:
                red.begin_weight_step()
            else:
                net.begin_arch_step()
                red.fg.zero()
                red.fg.attach()
        else:
            red = dp.GradReducer(list(net.parameters()))
            red.begin_step()
        pred = net(inp)
        if task == 'vgd':
            loss = (pred[0] * tgt).sum() + 0.5 * (pred[1] ** 2).sum()
            out = torch.cat([pred[0].reshape(-1), pred[1].reshape(-1)])
        elif task == 'itm':
            loss = torch.nn.functional.binary_cross_entropy(pred, tgt, reduction='sum')
            out = pred
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, tgt, reduction='sum')
            out = pred
        loss.backward()
        torch.cuda.synchronize()
        if count_small:
            L.check(L.lib().mmnas_prof_collect(arr))
            small = int(arr[L.K_NAMES.index('small_ops')].launches)
        grads = {k: (p.grad.detach().cpu().numpy().copy() if p.grad is not None else None) for k, p in net.named_parameters()}
        return out.detach().cpu().numpy(), grads, dict(chain=seen, lstm=steps, small=small)
    finally:
        if count_small:
            L.lib().mmnas_prof_enable(0)
        MixedOp.MODE = None
        ops.BackboneFn.apply, ops.lstm = o_apply, o_lstm
        ops.set_unpad_x(prev_x)
        ops.set_unpad(prev_y)
        if red is not None:
            red.fg.disable_sinks()


def _same(tag, a, b, gtol=4e-5):
    """tests/test_chain_gpu.py::_same with every figure recorded before it is asserted."""
    out_a, g_a, _ = a
    out_b, g_b, _ = b
    e_out = rel_err(out_a, out_b)
    top = max(float(np.abs(g).max()) for g in g_b.values() if g is not None)
    worst, worst_key, fails = 0.0, None, []
    for k in g_b:
        if g_b[k] is None:
            assert g_a[k] is None or not np.any(g_a[k]), k
            continue
        assert g_a[k] is not None, k
        diff = float(np.abs(g_a[k] - g_b[k]).max())
        t = max(gtol, REL_PATH_SELF_TOL) if is_rel_path(k) else gtol
        floor = (3e-3 if is_rel_path(k) else 1e-3) * top
        ratio = diff / (t * max(float(np.abs(g_b[k]).max()), floor))
        if ratio > worst:
            worst, worst_key = ratio, k
        if ratio > 1:
            fails.append((k, diff, float(np.abs(g_b[k]).max())))
    STATS[tag] = dict(out_rel_err=e_out, out_bar=2e-6, worst_grad_over_bar=worst, worst_grad_key=worst_key, gtol=gtol)
    print('unpad_x %s: out rel_err %.2e (bar 2e-6), worst gradient %.3f of its bar (%s)' % (tag, e_out, worst, worst_key))
    assert e_out < 2e-6
    assert not fails, fails


def _engaged(info, how, T, ragged_y=False, calls=1):
    assert info['lstm'] == [T], info
    assert info['chain'] == [dict(packed=how == 'packed', T=T, ragged_y=ragged_y)] * calls, info


def _pair(tag, task, arch, search, how, Tp, gtol, **kw):
    Sx = kw.get('Sx', 23)
    padded = _run(task, arch, search, False, **kw)
    ragged = _run(task, arch, search, True, **kw)
    _engaged(padded[2], 'dense', Sx, kw.get('unpad', False))
    _engaged(ragged[2], how, Tp, kw.get('unpad', False))
    _same(tag, ragged, padded, gtol)
    return ragged, padded


def _plan_with_guided(mode):
    """The first cases.search_plan whose evaluated decoder candidates include a guided operator (index 2 of the decoder's
    candidate list) -- 'full' evaluates every candidate anyway."""
    for seed in range(1, 50):
        pl = cases.search_plan(np.random.RandomState(seed), mode)
        if any(2 in act or (mode == 'two' and 2 in inact) for act, inact in pl['dec']):
            return pl['enc'] + pl['dec']
    raise AssertionError('no plan with a guided operator')


# ---------------------------------------------------------------------------------------- 1. + 2. packed, whole nets
@pytest.mark.parametrize('task,arch', [('itm', 'mmnas_itm'), ('vqa', 'mmnas_vqa'), ('vqa', 'mcan')])
def test_net_full_packed(task, arch):
    """Net_Full, B = 5, Sx = 23, lengths (1, 5, 16, 17, 20): T' = 20, packed.  ITM: 9 regions without region padding (the case
    the ragged decoder stream never takes)."""
    _pair('full_%s_%s' % (task, arch), task, arch, False, 'packed', 20, 1e-4)


@pytest.mark.parametrize('mode', [None, 'full', 'two'])
@pytest.mark.parametrize('task', ['itm', 'vqa'])
def test_net_search_packed(task, mode):
    """Net_Search weight step (MODE None) and architecture steps (MODE 'full' / 'two': the mixed chain's node buffers and
    node_mix launches on packed rows); the gate gradients are the alpha_gate parameters' gradients, compared by name."""
    plan = _plan_with_guided(mode)
    ragged, _ = _pair('search_%s_%s' % (task, mode), task, None, True, 'packed', 20, 4e-5, mode=mode, plan=plan)
    if mode is not None:
        assert any('alpha_gate' in k and g is not None and np.any(g) for k, g in ragged[1].items())


# ---------------------------------------------------------------------------------------- 3. - 6. edges of the plan
def test_single_sample_single_token():
    """B = 1 with one token: T' = 1, trimmed and dense."""
    _pair('one_token', 'itm', 'mmnas_itm', False, 'trim', 1, 1e-4, lengths=(1,))


@pytest.mark.parametrize('task,arch,search', [('itm', 'mmnas_itm', False), ('vqa', None, True)])
def test_longest_packed_stream(task, arch, search):
    """B = 2 with lengths (128, 3) under Sx = 128: T' = 128, the largest packed stream (65..128 keys: the bf16 cores)."""
    plan = _plan_with_guided(None) if search else None
    _pair('longest_%s' % task, task, arch, search, 'packed', 128, 4e-5 if search else 1e-4, lengths=(128, 3), Sx=128, plan=plan)


def test_trimmed_without_padding_stays_dense():
    """B = 3 with lengths (17, 17, 17) under Sx = 23: T' = 17, nothing to pack."""
    _pair('trim_17', 'itm', 'mmnas_itm', False, 'trim', 17, 1e-4, lengths=(17, 17, 17))


def test_short_stream_keeps_the_one_launch_operators():
    """T' = 14 (HSIZE 256: the one-launch short-sequence operators' width): trimmed, dense, and SelfAtt on the language stream
    still runs as one launch -- as many launches of that class as the padded run of the same net at 14 tokens."""
    plan = _plan_with_guided(None)
    assert any(act == [0] for act, _ in plan[:12])        # a sampled SelfAtt on the language stream
    kw = dict(lengths=(14, 3, 9), mode=None, plan=plan, HSIZE=256, count_small=True)
    ragged, _ = _pair('short_14', 'vqa', None, True, 'trim', 14, 4e-5, **kw)
    at14 = _run('vqa', None, True, False, Sx=14, **kw)
    assert ragged[2]['small'] == at14[2]['small'] > 0, (ragged[2]['small'], at14[2]['small'])


# ---------------------------------------------------------------------------------------- 7. + 8. with the other stream / task
def test_both_streams_ragged():
    """VQA with set_unpad and set_unpad_x: packed queries (y_off) against packed keys (x_off), both head sides packed."""
    plan = _plan_with_guided(None)
    _pair('both_search', 'vqa', None, True, 'packed', 20, 4e-5, mode=None, plan=plan, unpad=True)
    _pair('both_full', 'vqa', 'mmnas_vqa', False, 'packed', 20, 1e-4, unpad=True)


def test_vgd_trims_and_never_packs():
    """VGD's head is not the native one: trimmed to T' = 20, never packed; scores and regression equal the padded run's."""
    _pair('vgd', 'vgd', 'mmnas_vgd', False, 'trim', 20, 1e-4, Sy=11)


# ---------------------------------------------------------------------------------------- 9. refusals
def test_refusals_are_bitwise_the_switch_off(monkeypatch):
    """A zero token inside a question and the side stream: today's path, bit for bit.  MMNAS_CHAIN=0 (the per-operator path,
    out of scope for packing) trims only."""
    def bits(a, b, tag):      # (the outputs, bit for bit; the gradients to the bars: float atomics order some of their sums per run)
        assert np.array_equal(a[0], b[0])
        _same('refusal_' + tag, a, b, 1e-4)

    off = _run('itm', 'mmnas_itm', False, False, hole=(2, 3))
    on = _run('itm', 'mmnas_itm', False, True, hole=(2, 3))
    _engaged(on[2], 'dense', 23)
    bits(on, off, 'zero_token')
    monkeypatch.setenv('MMNAS_SIDE_STREAM', '1')
    off = _run('itm', 'mmnas_itm', False, False)
    on = _run('itm', 'mmnas_itm', False, True)
    _engaged(on[2], 'dense', 23)
    bits(on, off, 'side_stream')
    monkeypatch.setenv('MMNAS_SIDE_STREAM', '0')
    monkeypatch.setenv('MMNAS_CHAIN', '0')
    off = _run('itm', 'mmnas_itm', False, False)
    on = _run('itm', 'mmnas_itm', False, True)
    assert on[2]['chain'] == [] and on[2]['lstm'] == [20] and off[2]['lstm'] == [23]
    print('unpad_x chain0: outputs rel_err %.3e against the switch off' % rel_err(on[0], off[0]))
    assert np.array_equal(on[0], off[0])
    _same('chain0_trim', on, off, 1e-4)


# ---------------------------------------------------------------------------------------- 10. dropout
def test_dropout_is_reproducible_on_the_packed_stream():
    """Dropout 0.1: two runs from the same ops.manual_seed give identical bits and finite values.  The draws differ from the
    padded run's -- the dropout index of a packed row is its packed position, as on the ragged decoder stream -- so the
    padded run is no reference here."""
    a = _run('itm', 'mmnas_itm', False, True, dropout=0.1)
    b = _run('itm', 'mmnas_itm', False, True, dropout=0.1)
    _engaged(a[2], 'packed', 20)
    assert np.array_equal(a[0], b[0]) and np.isfinite(a[0]).all()
    for k, g in a[1].items():
        if g is not None:
            assert np.isfinite(g).all(), k
    nodrop = _run('itm', 'mmnas_itm', False, True)
    assert not np.array_equal(a[0], nodrop[0])             # (dropout was on)


# ---------------------------------------------------------------------------------------- 11. guard bands
from tests.test_guardband_gpu import planned  # noqa: E402,F401  (tests/guardband.py's Arena behind ops._bytes / ops._ws_floats)


def test_packed_chain_stays_inside_its_planned_arena(planned):
    """A chain with x_off and the head over packed language rows, their arenas handed out at EXACTLY the planned size between
    poisoned bands: every band intact, and the results those of the allocator's blocks -- bit for bit, but for the embedding
    table's gradient, whose rows of repeated tokens are summed by float atomics in an order of the run's own."""
    from mmnas_amd import ops
    arena, state = planned

    def run():
        out, grads, info = _run('itm', 'mmnas_itm', False, True)
        _engaged(info, 'packed', 20)
        return dict(grads, out=out)

    plain = run()
    state['on'] = True
    try:
        got = run()
        ops.join_side_stream()
        arena.check()
    finally:
        state['on'] = False
    sites = [('_bytes', 'BackboneFnBackward', 'forward'), ('_bytes', 'HeadFnBackward', 'forward')]
    assert not set(sites) - set(state['sites']), state['sites']
    assert set(got) == set(plain)
    for k in plain:
        if plain[k] is None:
            assert got[k] is None, k
        elif k == 'embedding.weight':
            assert rel_err(got[k], plain[k]) < 1e-6, k
        else:
            assert np.array_equal(got[k], plain[k]), (k, float(np.abs(got[k] - plain[k]).max()))
