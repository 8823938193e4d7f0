"""The ragged streams (ops.set_unpad: decoder / image rows; ops.set_unpad_x: language rows) on nets whose attention operators have
heads of 16, 32, 128 and 256 -- the head sizes whose packed attention cores run the general backward kernels (attention.hip:
mha_bwd_q_kernel / mha_bwd_kv_kernel over q_off / k_off) and whose relation operators run mmnas_rel_fused_*_ragged and the hoisted
relmulti launch at H = 1, 2, 8, 16 heads.  Whole nets, ragged against the padded run of the same net, weights and inputs, in the manner
of tests/test_chain_gpu.py::_run_unpad / _same and tests/test_unpad_x_gpu.py::_pair, at their bars: logits rel_err < 2e-6, every
parameter gradient within 4e-5 (supernets) / 1e-4 (Net_Full) of the parameter's largest entry, relation-path keys at
REL_PATH_SELF_TOL, floors of 1e-3 / 3e-3 of the net's largest gradient.  HSIZE = 256 (every head size divides it), dropout 0.

The supernets are built over a patched search space (the registry's candidate lists are an OpsAdapter instance's dict):
  enc: self_att_32, self_att_128, feed_forward;  dec: self_att_16, rel_self_att_32, guided_att_128, guided_att_256
('none' closes the 'enc' / 'dec' lists as in the registry; the cells are built from the '_safe' lists without it).  The alpha prior of
Net_Search.init_arch names operators of the stock space, so it is patched to names of this one (the plans are injected: the alphas
do not choose anything here).

MMNAS_PACKED_HEADS_STATS=<file> writes the worst error per case there (profiles/r16_packed_heads_error_stats.json is one such run)."""
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
HSIZE = 256
TOKENS = (20, 17, 9, 3, 1)       # Sx = 20: the longest fills the stream (T' = 20 > 16: packed, not the one-launch operators)
REGIONS = (23, 1, 12, 17, 5)     # Sy = 23
STATS = {}

GENOTYPE = {
    'enc': [['self_att_128'], ['feed_forward'], ['self_att_16'], ['feed_forward'], ['self_att_128'], ['self_att_16']],
    'dec': [['self_att_32'], ['guided_att_128'], ['feed_forward'], ['rel_self_att_16'], ['self_att_256'], ['guided_att_128'],
            ['rel_self_att_16'], ['feed_forward'], ['self_att_32'], ['self_att_256']],
}
ENC = ['self_att_32', 'self_att_128', 'feed_forward', 'none']
DEC = ['self_att_16', 'rel_self_att_32', 'guided_att_128', 'guided_att_256', 'none']
PRIOR = {'enc': ['self_att_32', 'feed_forward'] * 6, 'dec': ['rel_self_att_32', 'guided_att_128', 'guided_att_256'] * 6}


@atexit.register
def _write_stats():
    path = os.environ.get('MMNAS_PACKED_HEADS_STATS')
    if path and STATS:
        with open(path, 'w') as f:
            json.dump(STATS, f, indent=1, sort_keys=True)


@pytest.fixture
def space(monkeypatch):
    """The patched search space, in both OpsAdapter instances the model code reads (mixed.py builds the candidates, nets.py
    initialises the alphas and names genotypes)."""
    from mmnas_amd.model import mixed, nets
    for ad in (mixed.OPS_ADAPTER, nets.OPS_ADAPTER):
        monkeypatch.setitem(ad.Used_OPS, 'enc', list(ENC))
        monkeypatch.setitem(ad.Used_OPS, 'dec', list(DEC))
        monkeypatch.setitem(ad.Used_OPS, 'enc_safe', ENC[:-1])
        monkeypatch.setitem(ad.Used_OPS, 'dec_safe', DEC[:-1])
    monkeypatch.setattr(nets, '_PRIOR', PRIOR)


def _inputs(cfg, task, tokens, regions, Sx, Sy, token_size, ans_size):
    B = len(tokens)
    rs = np.random.RandomState(4244)
    frcn, bbox, y_rel, _, _ = cases.net_inputs(rs, cfg, B, Sx, Sy, token_size)
    frcn = np.maximum(rs.standard_normal(frcn.shape), 0).astype(np.float32)
    frcn[..., 0] += 0.05                                   # (no valid row is all zero)
    y_rel = rs.standard_normal(y_rel.shape).astype(np.float32)
    ques = rs.randint(1, token_size, size=(B, Sx)).astype(np.int64)
    x_rel = rs.standard_normal((B, Sx, Sx, 3)).astype(np.float32)
    for b, n in enumerate(tokens):
        ques[b, n:] = 0
        x_rel[b, n:] = 0
        x_rel[b, :, n:] = 0
    if regions is not None:
        for b, n in enumerate(regions):
            frcn[b, n:] = 0
            y_rel[b, n:] = 0
            y_rel[b, :, n:] = 0
    if task == 'itm':
        target = (rs.uniform(size=(B,)) < 0.5).astype(np.float32)
    else:
        target = (rs.uniform(size=(B, ans_size)) * (rs.uniform(size=(B, ans_size)) < 0.2)).astype(np.float32)
    return (frcn, bbox, y_rel, ques, x_rel), target, rs.standard_normal((token_size, cfg.WORD_EMBED_SIZE)).astype(np.float32) * 0.5


def _run(task, search, unpad_x, unpad_y, mode=None, plan=None, tokens=TOKENS, regions=REGIONS, Sx=20, Sy=23):
    """One forward + backward through the flat gradient buffer -> (outputs, gradients by name, what the chain was handed: one
    dict(packed_x, ragged_y) per BackboneFn call).  The weights are the modules' own initialisation under a fixed seed."""
    from mmnas_amd import dp, ops
    from mmnas.model.mixed import MixedOp
    token_size, ans_size = 40, 13
    cfg = cases.small_cfg(HSIZE=HSIZE)
    cfg.DROPOUT_R = 0.0
    if not search:
        cfg.GENOTYPE = GENOTYPE
    inputs, target, emb = _inputs(cfg, task, tokens, regions, Sx, Sy, token_size, ans_size)
    mod = importlib.import_module('mmnas.model.%s_%s' % ('hygr' if search else 'full', task))
    torch.manual_seed(20261021)
    net = (mod.Net_Search if search else mod.Net_Full)(cfg, {'token_size': token_size, 'ans_size': ans_size, 'pretrained_emb': emb})
    net = net.to(DEV).train()
    inp = tuple(T(a).to(DEV) for a in inputs)
    tgt = T(target).to(DEV)
    seen = []
    o_apply = ops.BackboneFn.apply
    # (the language side's description is the appended argument: a trailing ops.Ragged behind the parameter tensors; argument 10
    #  is the decoder side's)
    ops.BackboneFn.apply = lambda *a: (seen.append(dict(packed_x=isinstance(a[-1], ops.Ragged), ragged_y=a[10] is not None)), o_apply(*a))[1]
    prev_x, prev_y = ops.set_unpad_x(unpad_x), ops.set_unpad(unpad_y)
    red = None
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
        if task == 'itm':
            loss = torch.nn.functional.binary_cross_entropy(pred, tgt, reduction='sum')
        else:
            loss = torch.nn.functional.binary_cross_entropy_with_logits(pred, tgt, reduction='sum')
        loss.backward()
        torch.cuda.synchronize()
        grads = {k: (p.grad.detach().cpu().numpy().copy() if p.grad is not None else None) for k, p in net.named_parameters()}
        return pred.detach().cpu().numpy(), grads, seen
    finally:
        MixedOp.MODE = None
        ops.BackboneFn.apply = o_apply
        ops.set_unpad_x(prev_x)
        ops.set_unpad(prev_y)
        if red is not None:
            red.fg.disable_sinks()


def _same(tag, a, b, gtol):
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
        if not ratio <= worst:
            worst, worst_key = ratio, k
        if not ratio <= 1:
            fails.append((k, diff, float(np.abs(g_b[k]).max())))
    STATS[tag] = dict(out_rel_err=e_out, out_bar=2e-6, worst_grad_over_bar=worst, worst_grad_key=worst_key, gtol=gtol)
    print('ragged heads %s: out rel_err %.2e (bar 2e-6), worst gradient %.3f of its bar (%s)' % (tag, e_out, worst, worst_key))
    assert e_out < 2e-6
    assert not fails, fails


def _pair(tag, task, search, unpad_x, unpad_y, gtol, **kw):
    padded = _run(task, search, False, False, **kw)
    ragged = _run(task, search, unpad_x, unpad_y, **kw)
    assert padded[2] == [dict(packed_x=False, ragged_y=False)], padded[2]
    assert ragged[2] == [dict(packed_x=unpad_x, ragged_y=unpad_y)], ragged[2]      # the chain ran, and ran ragged
    _same(tag, ragged, padded, gtol)
    return ragged


def _plan(mode):
    """Injected (active, inactive) lists per node over the patched space (3 encoder, 4 decoder candidates).  MODE None / 'full':
    every attention candidate is the sampled one of some node.  MODE 'two': the nodes walk over all ordered candidate pairs, so
    candidates of different head sizes share a node (self_att_32 / self_att_128; self_att_16 / guided_att_256; ...)."""
    plan = []
    for n_nodes, n in ((12, 3), (18, 4)):
        pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
        for k in range(n_nodes):
            if mode == 'two':
                i, j = pairs[k % len(pairs)]
                plan.append(([i], [j]))
            else:
                a = k % n
                plan.append(([a], [i for i in range(n) if i != a]))
    return plan


# ---------------------------------------------------------------------------------------- Net_Full
@pytest.mark.parametrize('unpad_x,unpad_y', [(False, True), (True, False), (True, True)], ids=['decoder', 'language', 'both'])
def test_net_full_vqa(unpad_x, unpad_y):
    """Decoder side: self_att_32 (H = 8), guided_att_128 (H = 2), rel_self_att_16 (H = 16), self_att_256 (H = 1); encoder side:
    self_att_128 and self_att_16.  B = 5, 23 regions with counts (23, 1, 12, 17, 5), 20 tokens with counts (20, 17, 9, 3, 1)."""
    assert {n[0] for n in GENOTYPE['dec']} >= {'self_att_32', 'guided_att_128', 'rel_self_att_16', 'self_att_256'}
    assert {n[0] for n in GENOTYPE['enc']} >= {'self_att_128', 'self_att_16'}
    _pair('full_vqa_%s' % ('both' if unpad_x and unpad_y else 'language' if unpad_x else 'decoder'), 'vqa', False, unpad_x, unpad_y, 1e-4)


def test_net_full_itm_language_stream():
    """ITM: 9 regions, every image carries them all (the ragged decoder stream never takes this case); the language stream packs."""
    _pair('full_itm_language', 'itm', False, True, False, 1e-4, regions=None, Sy=9)


# ---------------------------------------------------------------------------------------- Net_Search
@pytest.mark.parametrize('mode', [None, 'full', 'two'])
def test_net_search_vqa_decoder_stream(mode, space):
    """Weight step (MODE None) and architecture steps: 'full' evaluates every candidate of every node (gate gradients compared by
    name: the alpha_gate parameters' gradients), 'two' a pair per node -- pairs of different head sizes among them."""
    plan = _plan(mode)
    if mode == 'two':
        assert ([0], [1]) in plan[:12] and ([0], [3]) in plan[12:]      # self_att_32 / self_att_128;  self_att_16 / guided_att_256
    else:
        assert {a[0] for a, _ in plan[:12]} >= {0, 1} and {a[0] for a, _ in plan[12:]} == {0, 1, 2, 3}
    ragged = _pair('search_vqa_decoder_%s' % mode, 'vqa', True, False, True, 4e-5, mode=mode, plan=plan)
    if mode is not None:
        assert any('alpha_gate' in k and g is not None and np.any(g) for k, g in ragged[1].items())


@pytest.mark.parametrize('mode', [None, 'full'])
def test_net_search_vqa_both_streams(mode, space):
    ragged = _pair('search_vqa_both_%s' % mode, 'vqa', True, True, True, 4e-5, mode=mode, plan=_plan(mode))
    if mode is not None:
        assert any('alpha_gate' in k and g is not None and np.any(g) for k, g in ragged[1].items())
