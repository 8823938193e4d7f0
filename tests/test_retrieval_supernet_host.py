"""CPU checks of the ITM search additions: the planner of retrieval.SupernetItmScorer under injected architectures (split,
re-planning, refusals), gather_mined's reordering against the reference's statements (search_itm.py:296-305), and the batched
triplet of the harness (triplet_batch's field order, BatchedTriplet against the three-argument losses)."""
import numpy as np
import pytest
import torch

from tests import supernet_plans as SP
from tests.golden import cases


def _supernet():
    c = cases.net_case('itm', None, 11, search=True, HSIZE=64, B=1, Sx=5, Sy=6)
    return SP.build_supernet(c)


@pytest.mark.parametrize('name', list(SP.PLANS))
def test_planner_follows_the_installed_architecture(name):
    from mmnas_amd.retrieval import SupernetItmScorer
    plan = SP.PLANS[name]
    net = _supernet()
    SP.install(net, plan)
    sc = SupernetItmScorer(net)
    prefix, guided, pair = SP.implied_split(plan)
    assert sc.prefix_nodes == prefix and sc.guided_ops == guided and sc.pair_nodes == pair
    assert len(prefix) + len(guided) + len(pair) == 18
    assert sc.arch == tuple(a[0] for a, _ in SP.sampled(plan))
    if name == 'guided_first_none':
        assert prefix == [] and (0, 4) in pair
        from mmnas_amd.model import modules as M
        assert isinstance(net.backnone.cells_dec[0].dag[4][0].active_op, M.Zero)
    if name == 'no_guided':
        assert guided == [] and pair == [] and len(prefix) == 18


def test_arch_follows_set_sampled_and_replans():
    from mmnas_amd.retrieval import SupernetItmScorer
    net = _supernet()
    SP.install(net, SP.PRIOR)
    sc = SupernetItmScorer(net)
    first = sc.arch
    assert sc.guided_ops == SP.implied_split(SP.PRIOR)[1]
    SP.install(net, SP.NO_GUIDED)
    assert sc.arch == first                       # (nothing called yet: the plan is the old one)
    sc._sync()                                    # what every public call does first
    assert sc.arch != first and sc.arch == tuple(a[0] for a, _ in SP.sampled(SP.NO_GUIDED))
    assert sc.guided_ops == []
    net.set_chosen_op_active()
    sc._sync()
    assert sc.arch == tuple(int(torch.argmax(m.alpha_prob)) for m in net.redundant_modules)


def test_refusals():
    from mmnas.model.full_itm import Net_Full
    from mmnas_amd.retrieval import ItmScorer, SupernetItmScorer
    net = _supernet()
    with pytest.raises(ValueError, match='no architecture was sampled'):
        SupernetItmScorer(net)
    uni = dict(SP.PRIOR, dec=list(SP.PRIOR['dec']), swaps=((7, 2, 'uniimg_att_64'),))
    uni['dec'][7] = 'uniimg_att_64'
    SP.install(net, uni)
    with pytest.raises(ValueError, match='UniimgAtt.*only GuidedAtt may read pre'):
        SupernetItmScorer(net)
    # ... also when the candidate becomes active after construction
    SP.install(net, SP.PRIOR)
    net.backnone.cells_dec[0].dag[7][0].set_active([0], [1, 2, 3], write_gate=False)
    sc = SupernetItmScorer(net)
    net.backnone.cells_dec[0].dag[7][0].set_active([2], [0, 1, 3], write_gate=False)
    with pytest.raises(ValueError, match='UniimgAtt'):
        sc._sync()
    assert sc.arch is None                        # no stale plan survives
    with pytest.raises(ValueError, match='Net_Search'):           # the fixed-network scorer still refuses the supernet
        ItmScorer(net)
    c = cases.net_case('itm', 'mmnas_itm', 11, HSIZE=64, B=1, Sx=5, Sy=6)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    with pytest.raises(ValueError, match='ITM Net_Search'):
        SupernetItmScorer(Net_Full(c['cfg'], init))
    with pytest.raises(ValueError, match='positive'):
        SupernetItmScorer(net, pair_batch=0)


def test_stale_cache_check_needs_no_device():
    from mmnas_amd.retrieval import CaptionCache, ImageCache, SupernetItmScorer
    net = _supernet()
    SP.install(net, SP.PRIOR)
    sc = SupernetItmScorer(net)
    img = ImageCache(torch.zeros(2, 1, 1, 6, dtype=torch.bool), torch.zeros(2, 6, 6, 4), torch.zeros(2, 6, 64))
    img.arch = sc.arch
    assert img.rows(0, 1).arch == sc.arch
    SP.install(net, SP.NO_GUIDED)
    with pytest.raises(ValueError, match='architecture'):
        sc.score_pairs(img, img, [0], [0])
    assert CaptionCache.arch is None


@pytest.mark.parametrize('world', [1, 2, 3])
@pytest.mark.parametrize('rest', [0, 1, 2])
def test_gather_mined_reordering_is_the_reference_statements(world, rest):
    from mmnas_amd import retrieval
    hard, per_rank = 5, 4
    rs = np.random.RandomState(10 * world + rest)
    parts = [torch.from_numpy(rs.randint(0, 29000, size=(per_rank, hard))) for _ in range(world)]
    # search_itm.py:297-305, the all_gather replaced by its result
    gather = [p.unsqueeze(1) for p in parts]
    want = torch.cat(gather, dim=1).view(-1, hard).cpu()
    if rest:
        want = want[: -rest]
    got = retrieval.interleave_ranks(parts)
    for r in range(world):                        # the sampler's order: rank r's i-th sample is dataset position r + world * i
        for i in range(per_rank):
            assert torch.equal(got[r + world * i], parts[r][i])
    got = got[:-rest] if rest else got
    assert torch.equal(got, want) and got.shape == (world * per_rank - rest, hard)
    if world == 1:                                # no process group: gather_mined only trims
        assert torch.equal(retrieval.gather_mined(parts[0], 1, rest), want)
    assert torch.equal(retrieval.gather_mined(parts[0], world, rest), parts[0][:-rest] if rest else parts[0])


def _five_tuple(rs, B, tag):
    return (torch.full((B, 4, 8), tag + 0.1), torch.full((B, 4, 5), tag + 0.2), torch.full((B, 4, 4, 4), tag + 0.3),
            torch.full((B, 6), int(tag)), torch.full((B, 6, 6, 3), tag + 0.5))


def test_triplet_batch_field_order():
    from mmnas_amd.harness import triplet_batch
    B = 3
    pos, neg = _five_tuple(None, B, 1.0), _five_tuple(None, B, 2.0)
    out = triplet_batch(pos, neg)
    assert len(out) == 5 and all(t.shape[0] == 3 * B for t in out)
    for i, src in ((0, (pos, pos, neg)), (1, (pos, pos, neg)), (2, (pos, pos, neg)), (3, (pos, neg, pos)), (4, (pos, neg, pos))):
        for k in range(3):
            assert torch.equal(out[i][k * B:(k + 1) * B], src[k][i]), (i, k)
    # the three slices are the script's three inputs (search_itm.py:373-375)
    negc = (pos[0], pos[1], pos[2], neg[3], neg[4])
    negi = (neg[0], neg[1], neg[2], pos[3], pos[4])
    for k, inp in enumerate((pos, negc, negi)):
        assert all(torch.equal(out[i][k * B:(k + 1) * B], inp[i]) for i in range(5))
    no_rel = triplet_batch(pos[:4] + (None,), neg[:4] + (None,))
    assert no_rel[4] is None and torch.equal(no_rel[3], out[3])


@pytest.mark.parametrize('kind', ['bce', 'margin'])
def test_batched_triplet_equals_the_three_argument_loss(kind):
    from mmnas_amd import harness, losses
    from mmnas_amd.utils.itm_loss import Margin_Loss
    B = 5
    g = torch.Generator().manual_seed(3)
    scores = torch.rand(3 * B, generator=g).requires_grad_(True)
    loss_fn = harness.BCE_Loss() if kind == 'bce' else Margin_Loss()
    bt = harness.BatchedTriplet(loss_fn)
    got = bt(scores, None)
    ref = scores.detach().clone().requires_grad_(True)
    want = loss_fn(ref[:B], ref[B:2 * B], ref[2 * B:])
    assert torch.equal(got, want)
    got.backward()
    want.backward()
    assert torch.equal(scores.grad, ref.grad)
    assert torch.equal(bt(scores.detach(), torch.zeros(3)), want.detach())          # the target is ignored
    assert harness.fused_loss(bt) is bt and losses.fused(bt) is bt
    with pytest.raises(ValueError, match='3B'):
        bt(torch.rand(7), None)
