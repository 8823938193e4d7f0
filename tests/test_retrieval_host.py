"""CPU checks of mmnas_amd.retrieval: the recall / rank fallback against a numpy restatement of the reference's evaluation
(train_itm.py:505-546), the documented tie rule, the mining fallback against harness.hard_negative_indices, and the
decoder planner of ItmScorer (split and refusals)."""
import numpy as np
import pytest
import torch

from tests.golden import cases


def reference_recall(score_matrix):
    """train_itm.py:505-546 restated (5 captions per image, argsort ranks)."""
    npts = score_matrix.shape[0]
    minnum_rank_image = np.array([1e7] * npts)
    for i in range(npts):
        cur_rank = np.argsort(score_matrix[i])[::-1]
        for index, j in enumerate(cur_rank):
            if j in range(5 * i, 5 * i + 5):
                minnum_rank_image[i] = index
                break
    score_t = score_matrix.transpose()
    minnum_rank_caption = np.array([1e7] * npts * 5)
    for i in range(5 * npts):
        img_id = i // 5
        cur_rank = np.argsort(score_t[i])[::-1]
        for index, j in enumerate(cur_rank):
            if j == img_id:
                minnum_rank_caption[i] = index
                break
    res = {}
    for name, r in (('i2t', minnum_rank_image), ('t2i', minnum_rank_caption)):
        res[name + '_r1'] = 100.0 * len(np.where(r < 1)[0]) / len(r)
        res[name + '_r5'] = 100.0 * len(np.where(r < 5)[0]) / len(r)
        res[name + '_r10'] = 100.0 * len(np.where(r < 10)[0]) / len(r)
        res[name + '_medr'] = np.floor(np.median(r)) + 1
        res[name + '_meanr'] = r.mean() + 1
    return res, minnum_rank_image, minnum_rank_caption


def distinct_matrix(rs, Ni, G=5, targets=(0, 4, 5, 9, 10), axis='rows'):
    """Distinct scores (k / N for a permutation k), the ground truth of each query placed at a target rank: rows = the best
    own caption of image i at rank targets[i % len]; cols = caption j's own image at that rank (where the rank exists)."""
    Nc = G * Ni
    N = Ni * Nc
    while True:   # (redrawn in the rare case that two crafted values round to the same float32)
        S = _craft(rs, (rs.permutation(N).reshape(Ni, Nc) + 1.0) / N, Ni, Nc, N, G, targets, axis).astype(np.float32)
        if len(np.unique(S)) == S.size:
            return S


def _craft(rs, S, Ni, Nc, N, G, targets, axis):
    if axis == 'rows':
        for i in range(Ni):
            own = list(range(G * i, G * i + G))
            others = np.sort(np.delete(S[i], own))[::-1]
            r = min(targets[i % len(targets)], len(others))
            hi = others[r - 1] if r > 0 else 2.0
            lo = others[r] if r < len(others) else -1.0
            S[i, own[0]] = lo + (hi - lo) * rs.uniform(0.25, 0.75)
            for g, c in enumerate(own[1:]):
                S[i, c] = -2.0 - (i * G + g) / N      # below every other score: the first own caption is the best one
    else:
        for j in range(Nc):
            o = j // G
            others = np.sort(np.delete(S[:, j], o))[::-1]
            r = min(targets[j % len(targets)], len(others))
            hi = others[r - 1] if r > 0 else 2.0
            lo = others[r] if r < len(others) else -1.0
            S[o, j] = lo + (hi - lo) * rs.uniform(0.25, 0.75)
    return S


@pytest.mark.parametrize('Ni', [1, 7, 100])
@pytest.mark.parametrize('axis', ['rows', 'cols'])
def test_recall_fallback_equals_reference_loops(Ni, axis):
    from mmnas_amd import retrieval
    S = distinct_matrix(np.random.RandomState(100 + Ni), Ni, axis=axis)
    want, r_img, r_cap = reference_recall(S)
    got = retrieval.recall_at_k(S, caps_per_image=5)
    for k, v in want.items():
        assert got[k] == pytest.approx(float(v), abs=0, rel=1e-12), (k, got[k], v)
    assert got['i2t_ties'] == 0 and got['t2i_ties'] == 0
    i2t, _, t2i, _ = retrieval.rank_matrix(torch.from_numpy(S))
    assert np.array_equal(i2t, r_img.astype(np.int64)) and np.array_equal(t2i, r_cap.astype(np.int64))
    # the crafted ground-truth ranks occur
    ranks = r_img if axis == 'rows' else r_cap
    if Ni == 100:
        assert {0, 4, 5, 9, 10} <= set(ranks.astype(int).tolist())


def test_tie_rule_and_tie_counts():
    from mmnas_amd import retrieval
    # 2 images x 2 captions each; saturated scores of 1.0
    S = np.array([[1.0, 0.5, 1.0, 1.0],     # image 0: best own 1.0; captions 2, 3 tie it -> rank 0, 2 tied candidates
                  [0.9, 0.2, 0.3, 0.1]], np.float32)   # image 1: best own 0.3; 0.9 above -> rank 1, no tie
    i2t, i2t_tie, t2i, t2i_tie = retrieval.rank_matrix(S, caps_per_image=2)
    assert i2t.tolist() == [0, 1] and i2t_tie.tolist() == [2, 0]
    # caption 0 (image 0): 1.0 vs 0.9 -> rank 0; caption 1: 0.5 vs 0.2 -> 0; caption 2 (image 1): 0.3 vs 1.0 -> rank 1;
    # caption 3: 0.1 vs 1.0 -> 1
    assert t2i.tolist() == [0, 0, 1, 1] and t2i_tie.tolist() == [0, 0, 0, 0]
    S2 = S.copy()
    S2[1, 0] = 1.0                           # caption 0: image 1 ties image 0 -> rank stays 0 (strictly greater), tie counted
    i2t, i2t_tie, t2i, t2i_tie = retrieval.rank_matrix(S2, caps_per_image=2)
    assert t2i.tolist() == [0, 0, 1, 1] and t2i_tie.tolist() == [1, 0, 0, 0]
    assert i2t.tolist() == [0, 1] and i2t_tie.tolist() == [2, 0]
    r = retrieval.recall_at_k(S2, caps_per_image=2)
    assert r['i2t_ties'] == 1 and r['t2i_ties'] == 1 and r['i2t_r1'] == 50.0 and r['t2i_r1'] == 50.0
    S2[0, 1] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        retrieval.recall_at_k(S2, caps_per_image=2)
    with pytest.raises(ValueError):
        retrieval.rank_matrix(np.zeros((3, 7), np.float32))


def test_hard_negative_fallback_matches_harness_and_stable_sort():
    from mmnas_amd import harness, retrieval
    rs = np.random.RandomState(5)
    N, C, k = 37, 64, 20
    scores = torch.from_numpy(rs.permutation(N * C).astype(np.float32) / (N * C))
    neg_idx = torch.from_numpy(rs.randint(0, 29000, size=(N, C)))
    got = retrieval.hard_negative_indices(scores, neg_idx, k)
    assert torch.equal(got, harness.hard_negative_indices(scores, neg_idx, k))
    tied = torch.from_numpy(rs.randint(0, 4, size=(N, C)).astype(np.float32))
    tied[0] = 1.0
    pos = torch.sort(tied, dim=-1, descending=True, stable=True)[1][:, :k]
    assert torch.equal(retrieval.topk_positions(tied, k), pos)
    assert torch.equal(retrieval.topk_positions(tied, k)[0], torch.arange(k))
    got = retrieval.hard_negative_indices(tied.reshape(-1), neg_idx, k)
    assert torch.equal(got, torch.gather(neg_idx, 1, pos))
    tied[3, 5] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        retrieval.hard_negative_indices(tied, neg_idx, k)


def _net(task='itm', arch='mmnas_itm', search=False, genotype=None):
    c = cases.net_case(task, arch if not search else None, 11, search=search, HSIZE=64, B=1, Sx=5, Sy=6)
    if genotype is not None:
        c['cfg'].GENOTYPE = genotype
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    if search:
        from mmnas.model.hygr_itm import Net_Search
        return Net_Search(c['cfg'], init)
    if task == 'vqa':
        from mmnas.model.full_vqa import Net_Full
    else:
        from mmnas.model.full_itm import Net_Full
    return Net_Full(c['cfg'], init)


def test_planner_splits_the_itm_decoder():
    from mmnas_amd.retrieval import ItmScorer
    net = _net()
    sc = ItmScorer(net)
    assert len(sc.prefix_nodes) == 1 and len(sc.guided_ops) == 10 and len(sc.pair_nodes) == 7
    g = cases.load_arch('mmnas_itm')['dec']
    assert [n for _, n in sc.guided_ops] == [i for i, node in enumerate(g) if node == ['guided_att_64']]
    assert sc.prefix_nodes == [(0, 0)]


def test_planner_refusals():
    from mmnas_amd.retrieval import ItmScorer
    g = cases.load_arch('mmnas_itm')
    bad = {'enc': g['enc'], 'dec': [list(n) for n in g['dec']]}
    bad['dec'][4] = ['uniimg_att_64']
    with pytest.raises(ValueError, match='UniimgAtt'):
        ItmScorer(_net(genotype=bad))
    multi = {'enc': g['enc'], 'dec': [list(n) for n in g['dec']]}
    multi['dec'][2] = ['guided_att_64', 'feed_forward']
    with pytest.raises(ValueError, match='single-operator'):
        ItmScorer(_net(genotype=multi))
    with pytest.raises(ValueError, match='Net_Search'):
        ItmScorer(_net(search=True))
    with pytest.raises(ValueError, match="'vqa'"):
        ItmScorer(_net(task='vqa', arch='mmnas_vqa'))
