"""mmnas_amd.retrieval on the MI355X: the indexed attention core against mmnas_mha_core_fwd on gathered K / V (bitwise), the
pair head against a torch composition, score_pairs against full network forwards (HIP net at the train_itm dimensions, float64
oracle at a small config), score_matrix against the reference's evaluation loop (train_itm.py:463-491), the rank / top-k
kernels against their CPU fallbacks, a mining round trip (train_itm.py:306-320), determinism and the net's state."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import mmnas_oracle as O
from tests.golden import cases
from tests.util import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _net(c):
    from mmnas.model.full_itm import Net_Full
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Full(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()}, strict=True)
    return net.to(DEV).eval()


def _inputs(c):
    return tuple(torch.from_numpy(a).to(DEV) for a in c['inputs'])


def _indexed(Q, KV, kcol, vcol, di, mask8, kv_idx, Sk, dh, drop_p=0.0):
    from mmnas_amd import _lib as L
    P, Sq, _ = Q.shape
    O_ = torch.empty_like(Q)
    lse = torch.empty(P, di // dh, Sq, 2, dtype=torch.float32, device=DEV)
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = P, di // dh, Sq, Sk, dh
    d.ldq = d.ldo = di
    d.ldk = d.ldv = KV.shape[1]
    d.Q, d.K, d.V, d.mask = L.fptr(Q), KV.data_ptr() + 4 * kcol, KV.data_ptr() + 4 * vcol, L.ptr(mask8)
    d.O, d.lse = L.fptr(O_), L.fptr(lse)
    d.drop_p = drop_p
    rc = L.lib().mmnas_mha_core_fwd_indexed(C.byref(d), L.ptr(kv_idx), L.stream())
    return rc, O_


@pytest.mark.parametrize('Sq', [36, 100])
@pytest.mark.parametrize('Sk', [14, 15, 50, 64])
@pytest.mark.parametrize('dh', [64, 32])
def test_indexed_core_is_bitwise_the_dense_core_on_gathered_kv(Sq, Sk, dh):
    from mmnas_amd import ops
    g = torch.Generator().manual_seed(1000 * Sq + Sk + dh)
    Nc, di = 5, 256
    ld = 4 * di + 12                                   # a strided slice of a wider product: ldk != di
    KV = torch.randn(Nc * Sk, ld, generator=g).to(DEV)
    mask = torch.zeros(Nc, Sk, dtype=torch.bool)
    for b in range(1, Nc):                             # caption 0 unpadded, the others with padded tails
        mask[b, int(torch.randint(1, Sk, (1,), generator=g)):] = True
    mask = mask.to(DEV)
    kv_idx = torch.tensor([3, 0, 3, 4, 1, 1, 2, 4, 0], dtype=torch.int32, device=DEV)   # repeated and permuted
    P = kv_idx.numel()
    Q = torch.randn(P, Sq, di, generator=g).to(DEV)
    rc, got = _indexed(Q, KV, di, 3 * di, di, mask.view(torch.uint8), kv_idx, Sk, dh)
    assert rc == 0
    idx = kv_idx.long()
    K = KV.view(Nc, Sk, ld)[idx][:, :, di:2 * di].contiguous()
    V = KV.view(Nc, Sk, ld)[idx][:, :, 3 * di:4 * di].contiguous()
    with torch.no_grad():
        want = ops.mha_core(Q, K, V, mask[idx].view(P, 1, 1, Sk), None, dh)
    torch.cuda.synchronize()
    assert torch.equal(got, want), float((got - want).abs().max())


def test_indexed_core_scope_limits():
    from mmnas_amd import _lib as L
    Nc, di, Sk = 2, 128, 65
    KV = torch.zeros(Nc * Sk, 2 * di, device=DEV)
    mask8 = torch.zeros(Nc, Sk, dtype=torch.uint8, device=DEV)
    kv_idx = torch.zeros(3, dtype=torch.int32, device=DEV)
    Q = torch.zeros(3, 36, di, device=DEV)
    rc, _ = _indexed(Q, KV, 0, di, di, mask8, kv_idx, Sk, 64)
    assert rc == -1 and b'64 keys' in L.lib().mmnas_last_error()
    rc, _ = _indexed(Q, KV, 0, di, di, mask8[:, :50].contiguous(), kv_idx, 50, 64, drop_p=0.1)
    assert rc == -2 and b'dropout' in L.lib().mmnas_last_error()


def test_pair_head_matches_torch_composition():
    from mmnas_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    Nc, P, D, eps = 11, 37, 1024, 1e-6
    xflat = torch.randn(Nc, D, generator=g).to(DEV)
    yflat = torch.randn(P, D, generator=g).to(DEV)
    a = (1 + 0.2 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    Wp = (torch.randn(1, D, generator=g) / 32).to(DEV)
    bp = torch.randn(1, generator=g).to(DEV)
    cap = torch.randint(0, Nc, (P,), generator=g, dtype=torch.int32).to(DEV)
    logits = torch.empty(P, device=DEV)
    scores = torch.empty(P, device=DEV)
    L.check(L.lib().mmnas_itm_pair_head(L.fptr(xflat), L.ptr(cap), L.fptr(yflat), L.fptr(a), L.fptr(b), L.fptr(Wp), L.fptr(bp),
                                        L.fptr(logits), L.fptr(scores), None, None, 0, P, D, eps, L.stream()))
    z = (xflat[cap.long()] + yflat).double()
    zn = a.double() * (z - z.mean(-1, keepdim=True)) / (z.std(-1, keepdim=True) + eps) + b.double()
    want = (zn @ Wp.double().t()).squeeze(-1) + bp.double()
    assert rel_err(logits.cpu().numpy(), want.cpu().numpy()) <= 1e-6
    assert rel_err(scores.cpu().numpy(), torch.sigmoid(want).cpu().numpy()) <= 1e-6
    # placement into a matrix
    M = torch.zeros(5, 40, device=DEV)
    rows = torch.randint(0, 5, (P,), generator=g, dtype=torch.int32).to(DEV)
    cols = torch.randperm(40, generator=g)[:P].to(torch.int32).to(DEV)
    L.check(L.lib().mmnas_itm_pair_head(L.fptr(xflat), L.ptr(cap), L.fptr(yflat), L.fptr(a), L.fptr(b), L.fptr(Wp), L.fptr(bp),
                                        None, L.fptr(M), L.ptr(rows), L.ptr(cols), M.stride(0), P, D, eps, L.stream()))
    assert torch.equal(M[rows.long(), cols.long()].cpu(), scores.cpu())
    assert int((M != 0).sum()) == P


def _materialise(inputs_img, inputs_cap, img_idx, cap_idx):
    frcn, bbox, rel_img = inputs_img
    cap_ix, rel_cap = inputs_cap
    return frcn[img_idx], bbox[img_idx], rel_img[img_idx], cap_ix[cap_idx], rel_cap[cap_idx]


def test_score_pairs_matches_the_hip_net_at_train_itm_dimensions():
    from mmnas_amd.retrieval import ItmScorer
    c = cases.net_case_full(('full', 'itm', 'mmnas_itm', 512, 6, 50, 36, None), 9900)
    net = _net(c)
    x = _inputs(c)
    img_idx = torch.tensor([0, 1, 2, 3, 4, 5, 0, 0, 3, 5, 2, 1, 4], device=DEV)
    cap_idx = torch.tensor([0, 1, 2, 3, 4, 5, 3, 3, 1, 0, 5, 5, 2], device=DEV)
    sc = ItmScorer(net, pair_batch=8, encode_batch=4)
    imgs = sc.encode_images(*x[:3])
    caps = sc.encode_captions(x[3], x[4])
    logit = sc.score_pairs(imgs, caps, img_idx, cap_idx, logits=True)
    score = sc.score_pairs(imgs, caps, img_idx, cap_idx)
    with torch.no_grad():
        want = net(_materialise(x[:3], x[3:], img_idx, cap_idx)).double()
    want_logit = torch.log(want) - torch.log1p(-want)
    e_logit = rel_err(logit.cpu().numpy(), want_logit.cpu().numpy())
    e_score = rel_err(score.cpu().numpy(), want.cpu().numpy())
    print('score_pairs vs net() at train_itm dims: logits max rel err %.3e, scores %.3e (logits %s)' %
          (e_logit, e_score, np.round(want_logit.cpu().numpy(), 3)))
    assert e_logit <= 1e-4 and e_score <= 1e-4
    assert torch.equal(torch.sigmoid(logit), score) or rel_err(torch.sigmoid(logit).cpu().numpy(), score.cpu().numpy()) < 1e-6


def test_score_pairs_matches_float64_oracle():
    from mmnas_amd.retrieval import ItmScorer
    c = cases.net_case('itm', 'mmnas_itm', 9901, HSIZE=128, B=5, Sx=9, Sy=7)
    net = _net(c)
    x = _inputs(c)
    img_idx = torch.tensor([0, 4, 2, 2, 1, 3, 0], device=DEV)
    cap_idx = torch.tensor([1, 1, 0, 4, 3, 2, 0], device=DEV)
    sc = ItmScorer(net, pair_batch=4, encode_batch=3)
    got = sc.score_pairs(sc.encode_images(*x[:3]), sc.encode_captions(x[3], x[4]), img_idx, cap_idx)
    P64 = {k: torch.from_numpy(v).double() for k, v in c['P'].items()}
    ins = [torch.from_numpy(a) for a in c['inputs']]
    ins = [t.double() if t.dtype == torch.float32 else t for t in ins]
    ii, ci = img_idx.cpu(), cap_idx.cpu()
    want = O.net_forward('itm', P64, c['cfg'], (ins[0][ii], ins[1][ii], ins[2][ii], ins[3][ci], ins[4][ci]),
                         genotype=c['genotype'])
    e = rel_err(got.cpu().numpy(), want.detach().numpy())
    print('score_pairs vs float64 oracle: %.3e' % e)
    assert e <= 1e-3


def _matrix_case():
    c = cases.net_case('itm', 'mmnas_itm', 9902, HSIZE=128, B=20, Sx=9, Sy=7)
    return c, _net(c), _inputs(c)


def test_score_matrix_matches_reference_eval_loop_and_shards():
    from mmnas_amd.retrieval import ItmScorer
    c, net, x = _matrix_case()
    imgs, caps = tuple(t[:4] for t in x[:3]), (x[3], x[4])
    # train_itm.py:474-491: one image repeated against caption batches of EVAL_BATCH_SIZE
    want = torch.zeros(4, 20, device=DEV)
    with torch.no_grad():
        for i in range(4):
            for s in range(0, 20, 8):
                e = min(20, s + 8)
                n = e - s
                inp = (imgs[0][i:i + 1].repeat(n, 1, 1), imgs[1][i:i + 1].repeat(n, 1, 1), imgs[2][i:i + 1].repeat(n, 1, 1, 1),
                       caps[0][s:e], caps[1][s:e])
                want[i, s:e] = net(inp)
    sc = ItmScorer(net, pair_batch=32, encode_batch=8)
    full = sc.score_matrix(imgs, caps, caption_chunk=20)
    e = rel_err(full.cpu().numpy(), want.cpu().numpy())
    print('score_matrix vs reference loop: %.3e' % e)
    assert e <= 1e-4
    a = sc.score_matrix(imgs, caps, rows=(0, 2), caption_chunk=20)
    b = sc.score_matrix(imgs, caps, rows=(2, 4), caption_chunk=20)
    assert torch.equal(a + b, full)
    assert torch.equal(sc.score_matrix(imgs, caps, caption_chunk=7), full)
    cache = sc.score_matrix(sc.encode_images(*imgs), sc.encode_captions(*caps))
    assert torch.equal(cache, full)


def test_rank_kernel_equals_fallback():
    from mmnas_amd import retrieval
    g = torch.Generator().manual_seed(8)
    for S in (torch.rand(1000, 5000, generator=g), torch.randint(0, 6, (1000, 5000), generator=g).float() / 5,
              torch.rand(7, 35, generator=g)):
        got = retrieval.rank_matrix(S.to(DEV))
        want = retrieval.rank_matrix(S)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert retrieval.recall_at_k(S.to(DEV)) == retrieval.recall_at_k(S)
    S = S.to(DEV)
    S[3, 4] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        retrieval.recall_at_k(S)


def test_topk_kernel_equals_fallback():
    from mmnas_amd import retrieval
    g = torch.Generator().manual_seed(9)
    for S, k in ((torch.rand(29000, 64, generator=g), 5), (torch.randint(0, 3, (29000, 64), generator=g).float(), 5),
                 (torch.rand(1000, 5000 // 5, generator=g), 20), (torch.randint(0, 4, (300, 1024), generator=g).float(), 1024),
                 (torch.rand(3, 7, generator=g), 7)):
        assert torch.equal(retrieval.topk_positions(S.to(DEV), k).cpu(), retrieval.topk_positions(S, k))
    S = torch.rand(4, 64, device=DEV)
    S[2, 1] = float('nan')
    with pytest.raises(ValueError, match='NaN'):
        retrieval.topk_positions(S, 5)


def test_mining_round_trip_matches_naive_path():
    """train_itm.py:306-320 at small dimensions: every anchor image against NEG_RANDSIZE random captions."""
    from mmnas_amd import harness, retrieval
    from mmnas_amd.retrieval import ItmScorer
    c, net, x = _matrix_case()
    rs = np.random.RandomState(4)
    n_anchor, rand_size, hard = 6, 16, 5
    anchors = torch.from_numpy(rs.randint(0, 20, n_anchor)).to(DEV)
    neg_idx = torch.from_numpy(np.stack([rs.choice(20, rand_size, replace=False) for _ in range(n_anchor)]))
    img_idx = anchors.repeat_interleave(rand_size)
    cap_idx = neg_idx.reshape(-1).to(DEV)
    with torch.no_grad():
        naive_scores = net(_materialise(x[:3], x[3:], img_idx, cap_idx))
    gaps = torch.sort(naive_scores.view(n_anchor, rand_size), -1)[0].diff(dim=-1)
    sc = ItmScorer(net, pair_batch=40, encode_batch=8)
    scores = sc.score_pairs(sc.encode_images(*x[:3]), sc.encode_captions(x[3], x[4]), img_idx, cap_idx)
    got = retrieval.hard_negative_indices(scores, neg_idx, hard)
    want = harness.hard_negative_indices(naive_scores, neg_idx, hard)
    gap, diff = float(gaps.min()), float((scores - naive_scores).abs().max())
    print('mining: smallest score gap %.3e, largest path difference %.3e' % (gap, diff))
    assert gap > 2 * diff                     # distinct scores, farther apart than the two paths differ
    assert torch.equal(got.cpu(), want.cpu())


def test_score_matrix_is_deterministic_and_leaves_the_net_alone():
    from mmnas_amd.retrieval import ItmScorer
    c, net, x = _matrix_case()
    net.train()
    net.attflat_y.eval()                       # a mixed state is restored module by module
    p0 = net.proj.weight
    p0.grad = torch.full_like(p0, 0.25)
    sc = ItmScorer(net, pair_batch=16, encode_batch=8)
    m1 = sc.score_matrix(tuple(t[:4] for t in x[:3]), (x[3], x[4]), caption_chunk=9)
    m2 = sc.score_matrix(tuple(t[:4] for t in x[:3]), (x[3], x[4]), caption_chunk=9)
    assert torch.equal(m1, m2)
    assert net.training and not net.attflat_y.training and net.attflat_x.training
    assert torch.equal(p0.grad, torch.full_like(p0, 0.25))
    assert all(p.grad is None for n, p in net.named_parameters() if n != 'proj.weight')
