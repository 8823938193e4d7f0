"""retrieval.SupernetItmScorer on the MI355X: factored scoring of the ITM supernet under injected architectures against full
network forwards of the same net (eval mode, MixedOp.MODE None, the same plan) and against the float64 oracle; score_matrix
under the chosen architecture; stale caches; the unused_modules_off() state; the net's state; and mining as search_itm.py does
it (search_itm.py:278-294, 313-333) against the reference statements on the naive scores.

Nets: HSIZE 128, 7 tokens, 9 regions, 5 images and 7 captions with ragged live lengths including a one-region image and a
one-token caption; pair_batch 4 and encode_batch 3, so every kind of batch is chunked and padded."""
import functools

import numpy as np
import pytest
import torch

from tests import supernet_plans as SP
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy


@functools.lru_cache(maxsize=None)
def _case(seed=9950):
    c, images, captions = SP.retrieval_case(seed)
    return c, images, captions, tuple(T(a).to(DEV) for a in images), tuple(T(a).to(DEV) for a in captions)


@functools.lru_cache(maxsize=None)
def _net(plan_name, seed=9950):
    """One net per plan (a plan's swapped-in candidate stays in its slot)."""
    net = SP.build_supernet(_case(seed)[0], DEV).eval()
    if plan_name is not None:
        SP.install(net, SP.PLANS[plan_name])
    return net


def _naive(net, img, cap, img_idx, cap_idx):
    """net(gathered inputs): eval mode, MODE None, the installed plan."""
    from mmnas.model.mixed import MixedOp
    assert MixedOp.MODE is None and not net.training
    with torch.no_grad():
        return net((img[0][img_idx], img[1][img_idx], img[2][img_idx], cap[0][cap_idx], cap[1][cap_idx]))


def _all_pairs(n_img, n_cap):
    return (torch.arange(n_img, device=DEV).repeat_interleave(n_cap), torch.arange(n_cap, device=DEV).repeat(n_img))


def _first(t, n):
    return tuple(a[:n] for a in t)


@pytest.mark.parametrize('name', list(SP.PLANS))
def test_score_pairs_matches_the_net_and_the_oracle(name):
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = _net(name)
    sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
    assert (sc.prefix_nodes, sc.guided_ops, sc.pair_nodes) == SP.implied_split(SP.PLANS[name])
    ii, ci = _all_pairs(SP.N_IMG, SP.N_CAP)
    imgs, caps = sc.encode_images(*img), sc.encode_captions(*cap)
    assert imgs.arch == caps.arch == sc.arch
    assert (caps.kv is None) == (name == 'no_guided')
    logit = sc.score_pairs(imgs, caps, ii, ci, logits=True)
    score = sc.score_pairs(imgs, caps, ii, ci)
    want = _naive(net, img, cap, ii, ci).double()
    want_logit = torch.log(want) - torch.log1p(-want)
    e_logit = rel_err(logit.cpu().numpy(), want_logit.cpu().numpy())
    e_score = rel_err(score.cpu().numpy(), want.cpu().numpy())
    oracle = SP.oracle_scores(c, SP.PLANS[name], _first(images, SP.N_IMG), _first(captions, SP.N_CAP), ii.cpu().numpy(), ci.cpu().numpy())
    e_oracle = rel_err(score.cpu().numpy(), oracle)
    print('%s: score_pairs vs net() logits %.3e scores %.3e; scores vs float64 oracle %.3e' % (name, e_logit, e_score, e_oracle))
    assert e_logit <= 1e-4 and e_score <= 1e-4
    assert e_oracle <= 1e-3


def test_score_matrix_under_the_chosen_architecture():
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = _net(None)
    net.set_chosen_op_active()
    want = torch.zeros(SP.N_IMG, SP.N_CAP, device=DEV)
    for i in range(SP.N_IMG):                      # the evaluation's loop of forwards: one image against every caption
        ii = torch.full((SP.N_CAP,), i, device=DEV)
        want[i] = _naive(net, img, cap, ii, torch.arange(SP.N_CAP, device=DEV))
    sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
    small = sc.score_matrix(img, cap, caption_chunk=3)
    e = rel_err(small.cpu().numpy(), want.cpu().numpy())
    print('score_matrix (chosen architecture) vs the loop of forwards: %.3e' % e)
    assert e <= 1e-4
    # at one pair_batch an entry does not depend on how the work was chunked or sharded
    assert torch.equal(sc.score_matrix(img, cap), small)
    assert torch.equal(sc.score_matrix(img, cap, rows=(0, 2), caption_chunk=5) + sc.score_matrix(img, cap, rows=(2, 5)), small)
    assert torch.equal(sc.score_matrix(sc.encode_images(*img), sc.encode_captions(*cap)), small)


def test_score_matrix_is_bitwise_the_same_across_pair_batch_4_and_1024():
    """M = 36 rows per product against M = 9216: the scorer schedules its products on whole output tiles, whose K sum has one
    order whatever M (the automatic schedule's stream-K runs gave the two matrices 1.2e-7 apart)."""
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = _net(None)
    net.set_chosen_op_active()
    small = SupernetItmScorer(net, pair_batch=4, encode_batch=3).score_matrix(img, cap, caption_chunk=3)
    large = SupernetItmScorer(net, pair_batch=1024, encode_batch=3).score_matrix(img, cap)
    print('score_matrix, pair_batch 4 against 1024: largest difference %.3e (relative %.3e)' %
          (float((small - large).abs().max()), rel_err(small.cpu().numpy(), large.cpu().numpy())))
    assert torch.equal(small, large)


def test_stale_caches_raise_and_fresh_ones_score():
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = _net(None)
    SP.install(net, SP.PRIOR)
    sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
    imgs, caps = sc.encode_images(*img), sc.encode_captions(*cap)
    old = sc.arch
    SP.install(net, SP.NO_GUIDED)                  # a re-sample
    ii, ci = _all_pairs(SP.N_IMG, SP.N_CAP)
    with pytest.raises(ValueError, match='architecture'):
        sc.score_pairs(imgs, caps, ii, ci)
    with pytest.raises(ValueError, match='architecture'):
        sc.score_matrix(imgs, caps)
    with pytest.raises(ValueError, match='architecture'):
        sc.score_pairs(sc.encode_images(*img), caps, ii, ci)          # one fresh, one stale
    assert sc.arch != old and sc.guided_ops == []
    got = sc.score_pairs(sc.encode_images(*img), sc.encode_captions(*cap), ii, ci)
    e = rel_err(got.cpu().numpy(), _naive(net, img, cap, ii, ci).cpu().numpy())
    assert e <= 1e-4, e


def test_scoring_inside_unused_modules_off_gives_the_same_bits():
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = _net('prior')
    sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
    outside = sc.score_matrix(img, cap)
    net.unused_modules_off()
    try:
        assert sum(op is None for m in net.redundant_modules for op in m.candidate_ops) == 12 * 1 + 18 * 3
        inside = SupernetItmScorer(net, pair_batch=4, encode_batch=3).score_matrix(img, cap)
        again = sc.score_matrix(img, cap)
    finally:
        net.unused_modules_back()
    assert torch.equal(inside, outside) and torch.equal(again, outside)
    assert all(op is not None for m in net.redundant_modules for op in m.candidate_ops)


def test_the_net_is_left_as_it_was():
    from mmnas.model.mixed import MixedOp
    from mmnas_amd.retrieval import SupernetItmScorer
    c, images, captions, img, cap = _case()
    img, cap = _first(img, SP.N_IMG), _first(cap, SP.N_CAP)
    net = SP.build_supernet(c, DEV)
    SP.install(net, SP.GUIDED_FIRST)
    net.train()
    net.attflat_y.eval()                           # a mixed state is restored module by module
    p0 = net.proj.weight
    p0.grad = torch.full_like(p0, 0.25)
    gates = [m.alpha_gate.detach().clone() for m in net.redundant_modules]
    alphas = [m.alpha_prob.detach().clone() for m in net.redundant_modules]
    index = [(list(m.active_index), list(m.inactive_index)) for m in net.redundant_modules]
    import os
    knob = os.environ.get('MMNAS_GEMM_SK')
    MixedOp.MODE = 'two'
    try:
        sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
        m1 = sc.score_matrix(img, cap, caption_chunk=3)
        assert MixedOp.MODE == 'two'
        m2 = sc.score_matrix(sc.encode_images(*img), sc.encode_captions(*cap))
        assert MixedOp.MODE == 'two'
    finally:
        MixedOp.MODE = None
    assert torch.equal(m1, m2)
    assert os.environ.get('MMNAS_GEMM_SK') == knob          # the products' schedule is the caller's again
    assert net.training and not net.attflat_y.training and net.attflat_x.training
    assert all(m.training and all(op.training for op in m.candidate_ops) for m in net.redundant_modules)
    assert torch.equal(p0.grad, torch.full_like(p0, 0.25))
    assert all(p.grad is None for n, p in net.named_parameters() if n != 'proj.weight')
    for m, g, a, (act, inact) in zip(net.redundant_modules, gates, alphas, index):
        assert torch.equal(m.alpha_gate.detach(), g) and torch.equal(m.alpha_prob.detach(), a)
        assert m.active_index == act and m.inactive_index == inact


@pytest.mark.parametrize('anchor', ['image', 'caption'])
def test_mining_equals_the_reference_statements_on_the_naive_scores(anchor):
    """5 anchors x 6 candidates, hard_size 3.  The case and the draw were picked on the CPU with the float64 oracle so that every
    anchor's four best candidates are at least 1e-2 apart (supernet_plans.MINING_*): asserted here before the comparison."""
    from mmnas_amd import retrieval
    from mmnas_amd.retrieval import SupernetItmScorer
    seed, plan = SP.MINING_CASE_SEED, SP.MINING_PLAN
    c, images, captions, img, cap = _case(seed)
    net = _net(plan, seed)
    hard = 3
    anchors, cand = SP.mining_draw(anchor)
    own, other = anchors.repeat_interleave(cand.shape[1]), cand.reshape(-1)
    ii, ci = (own, other) if anchor == 'image' else (other, own)
    oracle = SP.oracle_scores(c, SP.PLANS[plan], images, captions, ii.numpy(), ci.numpy()).reshape(cand.shape)
    top4 = -np.sort(-oracle, axis=1)[:, :4]
    gap = float((-np.diff(top4, axis=1)).min())
    print('mining (%s anchors): smallest gap among the four best oracle scores %.3e' % (anchor, gap))
    assert gap >= 1e-2
    # the reference statements (search_itm.py:289-293 / 328-332) on the naive scores
    scores = _naive(net, img, cap, ii.to(DEV), ci.to(DEV)).view(-1, cand.shape[1])
    arg_scores = torch.argsort(scores, dim=-1, descending=True)[:, :hard]
    arg_scores_bi = torch.arange(arg_scores.size(0)).unsqueeze(1).expand_as(arg_scores)
    want = cand[arg_scores_bi, arg_scores.cpu()]
    sc = SupernetItmScorer(net, pair_batch=4, encode_batch=3)
    imgs, caps = sc.encode_images(*img), sc.encode_captions(*cap)
    got = retrieval.mine_hard_negatives(sc, imgs, caps, anchors, cand, hard, anchor=anchor)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, hard)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want, T(np.take_along_axis(cand.numpy(), np.argsort(-oracle, axis=1)[:, :hard], axis=1)))


@pytest.mark.parametrize('anchor', ['image', 'caption'])
def test_mining_takes_the_fixed_network_scorer_too(anchor):
    """mine_hard_negatives over an ItmScorer (train_itm.py's mining pass): the selection step on the scorer's own pair scores."""
    from mmnas.model.full_itm import Net_Full
    from mmnas_amd import retrieval
    from tests.golden import cases
    c = cases.net_case('itm', 'mmnas_itm', 9902, HSIZE=128, B=7, Sx=7, Sy=9)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Full(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    net = net.to(DEV).eval()
    x = tuple(T(a).to(DEV) for a in c['inputs'])
    sc = retrieval.ItmScorer(net, pair_batch=4, encode_batch=3)
    imgs, caps = sc.encode_images(*x[:3]), sc.encode_captions(x[3], x[4])
    assert imgs.arch is None and caps.arch is None
    anchors, cand = SP.mining_draw(anchor)
    own, other = anchors.repeat_interleave(cand.shape[1]), cand.reshape(-1)
    scores = sc.score_pairs(imgs, caps, own, other) if anchor == 'image' else sc.score_pairs(imgs, caps, other, own)
    got = retrieval.mine_hard_negatives(sc, imgs, caps, anchors, cand, 3, anchor=anchor)
    assert torch.equal(got, retrieval.hard_negative_indices(scores, cand, 3)) and tuple(got.shape) == (5, 3)
    with pytest.raises(ValueError, match="'image' or 'caption'"):
        retrieval.mine_hard_negatives(sc, imgs, caps, anchors, cand, 3, anchor='both')
