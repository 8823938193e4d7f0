"""A/B of the ITM retrieval evaluation at the train_itm dimensions (HSIZE 512, 36 regions, 50 tokens, arch/mmnas_itm.json,
random weights and inputs):

  A  the reference's evaluation loop statement for statement (train_itm.py:474-491): every image repeated against caption
     batches of EVAL_BATCH_SIZE = 320, one full net() forward per pair;
  B  mmnas_amd.retrieval.ItmScorer.score_matrix (captions encoded once, the pair side per pair).

A and B alternate, --rounds each, over --images x --captions pairs (default 8 x 5000 = 40 k); pairs/s of each round, the
median ratio and the largest difference of the two matrices are printed.  Then recall_at_k on a --rank-images x 5 score matrix:
the rank kernel alone (HIP events) and the whole call (ranks, the copy back, the metrics), against the reference's numpy loops
(train_itm.py:505-546) over the first --numpy-rows images.  Last line: one JSON record.

  python tools/itm_retrieval_ab.py [--images 8 --captions 5000 --rounds 3]

--supernet: the search script's side instead (search_itm.py dimensions: HSIZE 256, 36 regions, 50 tokens, one sampled
architecture, MixedOp.MODE None):

  A  one step of the hard-negative mining pass as the script runs it (search_itm.py:278-294): net(inputs) over the
     NEG_BATCHSIZE x NEG_RANDSIZE = 128 x 32 pair batch, argsort, the selection;
  B  retrieval.mine_hard_negatives over a SupernetItmScorer: the 128 anchor images and the candidate captions encoded (every
     call, inside the timed region), score_pairs, the top-k kernel.  The candidates are drawn from --caption-pool captions:
     640 by default, the reuse of the script's own pass (29 000 x 32 draws from 145 000 captions: 6.4 uses per caption).

then a triplet weight step at B = 64 (forward + backward, no optimizer step): the 3B batch through SearchLoop
(harness.triplet_batch / BatchedTriplet), and three B-forwards and the one 3B forward through the per-call path (plain autograd,
MMNAS_CHAIN default).  A and B alternate, --rounds each, timed between device events.  Last line: one JSON record.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.golden import cases  # noqa: E402


def build(args, dev):
    from mmnas.model.full_itm import Net_Full
    c = cases.net_case_full(('full', 'itm', 'mmnas_itm', 512, 2, 50, 36, None), 9950)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Full(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()}, strict=True)
    net = net.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    Ni, Nc, Sy, Sx = args.images, args.captions, 36, 50
    frcn = torch.relu(torch.randn(Ni, Sy, 2048, device=dev, generator=g))
    bbox = torch.zeros(Ni, Sy, 5, device=dev)
    rel_img = torch.randn(Ni, Sy, Sy, 4, device=dev, generator=g)
    ny = torch.randint(10, Sy + 1, (Ni,), device=dev, generator=g)
    for i in range(Ni):                      # padded regions, as the loaders pad behind the detected boxes
        frcn[i, ny[i]:] = 0
        rel_img[i, ny[i]:] = 0
        rel_img[i, :, ny[i]:] = 0
    cap = torch.randint(1, c['token_size'], (Nc, Sx), device=dev, generator=g)
    nx = torch.randint(5, Sx + 1, (Nc,), device=dev, generator=g)
    cap[torch.arange(Sx, device=dev)[None, :] >= nx[:, None]] = 0
    rel_cap = torch.randn(Nc, Sx, Sx, 3, device=dev, generator=g)
    return net, (frcn, bbox, rel_img), (cap, rel_cap)


def path_a(net, imgs, caps, bs=320):
    frcn_l, bbox_l, rel_l = imgs
    cap_l, rel_cap_l = caps
    scores_mat = torch.zeros(frcn_l.shape[0], cap_l.shape[0], device=frcn_l.device)
    with torch.no_grad():
        for start_y in range(frcn_l.shape[0]):
            frcn_, bbox_, rel_ = frcn_l[start_y:start_y + 1], bbox_l[start_y:start_y + 1], rel_l[start_y:start_y + 1]
            for start_x in range(0, cap_l.shape[0], bs):
                end_x = min(start_x + bs, cap_l.shape[0])
                n = end_x - start_x
                inp = (frcn_.repeat(n, 1, 1), bbox_.repeat(n, 1, 1), rel_.repeat(n, 1, 1, 1), cap_l[start_x:end_x],
                       rel_cap_l[start_x:end_x])
                scores_mat[start_y, start_x:end_x] = net(inp)
    return scores_mat


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def numpy_reference_ranks(S, rows):
    """train_itm.py:505-546's argsort loops (i2t part) over the first `rows` images: seconds per image."""
    t = time.perf_counter()
    for i in range(rows):
        cur_rank = np.argsort(S[i])[::-1]
        for index, j in enumerate(cur_rank):
            if j in range(5 * i, 5 * i + 5):
                break
    return (time.perf_counter() - t) / rows


def _events(fn):
    """(result, milliseconds between two device events around fn)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def _supernet(dev, seed):
    from mmnas.model.hygr_itm import Net_Search
    c = cases.net_case_full(('search', 'itm', None, 256, 2, 50, 36, None), seed)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()}, strict=True)
    return c, net.to(dev)


def _random_set(c, dev, Ni, Nc, seed, Sy=36, Sx=50):
    g = torch.Generator(device=dev).manual_seed(seed)
    frcn = torch.relu(torch.randn(Ni, Sy, 2048, device=dev, generator=g))
    rel_img = torch.randn(Ni, Sy, Sy, 4, device=dev, generator=g)
    ny = torch.randint(10, Sy + 1, (Ni,), device=dev, generator=g)
    pad = torch.arange(Sy, device=dev)[None, :] >= ny[:, None]
    frcn[pad] = 0
    rel_img[pad] = 0
    rel_img.transpose(1, 2)[pad] = 0
    cap = torch.randint(1, c['token_size'], (Nc, Sx), device=dev, generator=g)
    nx = torch.randint(5, Sx + 1, (Nc,), device=dev, generator=g)
    cap[torch.arange(Sx, device=dev)[None, :] >= nx[:, None]] = 0
    rel_cap = torch.randn(Nc, Sx, Sx, 3, device=dev, generator=g)
    return (frcn, torch.zeros(Ni, Sy, 5, device=dev), rel_img), (cap, rel_cap)


def supernet_main(args):
    from mmnas.model.mixed import MixedOp, seed_arch_sampler
    from mmnas_amd import harness, retrieval
    dev = 'cuda:0'
    anchors_n, rand, hard = 128, 32, 5                # NEG_BATCHSIZE, NEG_RANDSIZE, NEG_HARDSIZE (search_itm.py:87-89)
    c, net = _supernet(dev, 9960)
    net.eval()
    seed_arch_sampler(888)
    MixedOp.MODE = None
    net.reset_binary_gates()
    imgs, caps = _random_set(c, dev, anchors_n, args.caption_pool, 1)
    g = torch.Generator().manual_seed(2)
    anchor_idx = torch.arange(anchors_n)
    cand_idx = torch.stack([torch.randperm(args.caption_pool, generator=g)[:rand] for _ in range(anchors_n)])
    ii, ci = anchor_idx.repeat_interleave(rand).to(dev), cand_idx.reshape(-1).to(dev)
    pairs = anchors_n * rand

    def path_a():
        with torch.no_grad():
            scores = net((imgs[0][ii], imgs[1][ii], imgs[2][ii], caps[0][ci], caps[1][ci]))
            scores = scores.view(-1, rand)
            arg_scores = torch.argsort(scores, dim=-1, descending=True)[:, :hard]
            arg_scores_bi = torch.arange(arg_scores.size(0)).unsqueeze(1).expand_as(arg_scores)
            return cand_idx[arg_scores_bi, arg_scores.cpu()].to(scores.device), scores

    sc = retrieval.SupernetItmScorer(net, pair_batch=args.pair_batch)

    def path_b():
        ic, cc = sc.encode_images(*imgs), sc.encode_captions(*caps)
        return retrieval.mine_hard_negatives(sc, ic, cc, anchor_idx, cand_idx, hard), (ic, cc)

    net.unused_modules_off()                           # the script mines in this state (search_itm.py:271)
    try:
        (sel_a, scores_a), _ = _events(path_a)         # warm-up of both paths
        (sel_b, (ic, cc)), _ = _events(path_b)
        ta, tb = [], []
        for r in range(args.rounds):
            ta.append(_events(path_a)[1])
            tb.append(_events(path_b)[1])
            print('round %d: A %.0f pairs/s (%.1f ms)   B %.0f pairs/s (%.1f ms)' %
                  (r, pairs / ta[-1] * 1e3, ta[-1], pairs / tb[-1] * 1e3, tb[-1]))
        diff = float((sc.score_pairs(ic, cc, ii, ci) - scores_a.reshape(-1)).abs().max())
        same = float((sel_a == sel_b).all(1).float().mean())
    finally:
        net.unused_modules_back()
    ma, mb = statistics.median(ta), statistics.median(tb)
    print('mining pass, %d anchors x %d candidates of %d captions, %d guided operators active: A (net() per pair batch) %.0f '
          'pairs/s   B (SupernetItmScorer, encoding included) %.0f pairs/s   B/A = %.2fx   max |score A - B| = %.2e   anchors '
          'with the same selection %.3f' % (anchors_n, rand, args.caption_pool, len(sc.guided_ops), pairs / ma * 1e3,
                                            pairs / mb * 1e3, ma / mb, diff, same))

    # the triplet weight step at B = 64 (forward + backward)
    B = 64
    c1, net1 = _supernet(dev, 9960)
    c2, net2 = _supernet(dev, 9960)
    net1.train()
    net2.train()
    (f, bb, r), (cp, rc) = _random_set(c, dev, 2 * B, 2 * B, 3)
    pos = (f[:B], bb[:B], r[:B], cp[:B], rc[:B])
    neg = (f[B:], bb[B:], r[B:], cp[B:], rc[B:])
    loss_fn = harness.BCE_Loss()
    loop = harness.SearchLoop(net1, loss_fn=harness.BatchedTriplet(loss_fn))
    plan = [(list(m.active_index), list(m.inactive_index)) for m in net.redundant_modules]
    net2.set_sampled(plan)
    batch3 = harness.triplet_batch(pos, neg)

    def step_3b():
        return loop.weight_step(batch3, None, optimize=False, plan=plan)

    def step_three():
        net2.zero_grad()
        return harness.itm_triplet_step(net2, loss_fn, pos, neg)

    bt = harness.BatchedTriplet(loss_fn)

    def step_3b_percall():
        net2.zero_grad()
        loss = bt(net2(batch3), None)
        loss.backward()
        return loss

    try:
        steps = {'searchloop_3b': step_3b, 'percall_three_forwards': step_three, 'percall_3b': step_3b_percall}
        times = {k: [] for k in steps}
        for k, fn in steps.items():
            _events(fn)
        for r in range(args.rounds + 2):
            for k, fn in steps.items():
                times[k].append(_events(fn)[1])
        l3, lt = float(step_3b().detach()), float(step_three().detach())
    finally:
        loop.reducer.fg.disable_sinks()
    med = {k: statistics.median(v) for k, v in times.items()}
    print('triplet weight step, B = %d (forward + backward): 3B batch through SearchLoop %.2f ms   three B-forwards, per-call path '
          '%.2f ms   one 3B forward, per-call path %.2f ms   losses %.6f / %.6f' %
          (B, med['searchloop_3b'], med['percall_three_forwards'], med['percall_3b'], l3, lt))
    print(json.dumps({'tool': 'itm_retrieval_ab --supernet', 'anchors': anchors_n, 'candidates': rand, 'caption_pool': args.caption_pool,
                      'rounds': args.rounds, 'guided_ops': len(sc.guided_ops), 'a_pairs_per_s': pairs / ma * 1e3,
                      'b_pairs_per_s': pairs / mb * 1e3, 'b_over_a': ma / mb, 'max_abs_score_diff': diff, 'same_selection': same,
                      'a_ms': ta, 'b_ms': tb, 'triplet_step_ms': med, 'triplet_step_all_ms': times}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--supernet', action='store_true')
    ap.add_argument('--caption-pool', type=int, default=640)
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--captions', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pair-batch', type=int, default=1024)
    ap.add_argument('--caption-chunk', type=int, default=1000)
    ap.add_argument('--rank-images', type=int, default=1000)
    ap.add_argument('--numpy-rows', type=int, default=20)
    args = ap.parse_args()
    if args.supernet:
        return supernet_main(args)
    from mmnas_amd import _lib as L
    from mmnas_amd import retrieval
    dev = 'cuda:0'
    net, imgs, caps = build(args, dev)
    sc = retrieval.ItmScorer(net, pair_batch=args.pair_batch)
    pairs = args.images * args.captions

    def run_b():
        return sc.score_matrix(imgs, caps, caption_chunk=args.caption_chunk)

    a, _ = timed(lambda: path_a(net, imgs, caps))    # warm-up of both paths (plans, workspaces, allocator)
    b, _ = timed(run_b)
    ta, tb = [], []
    for r in range(args.rounds):
        a, t = timed(lambda: path_a(net, imgs, caps))
        ta.append(t)
        b, t = timed(run_b)
        tb.append(t)
        print('round %d: A %.0f pairs/s (%.3f s)   B %.0f pairs/s (%.3f s)' % (r, pairs / ta[-1], ta[-1], pairs / tb[-1], tb[-1]))
    diff = float((a - b).abs().max())
    ratio = statistics.median(ta) / statistics.median(tb)
    print('A (reference loop, net() per pair): %.0f pairs/s   B (ItmScorer.score_matrix): %.0f pairs/s   B/A = %.2fx   '
          'max |A - B| = %.2e' % (pairs / statistics.median(ta), pairs / statistics.median(tb), ratio, diff))

    # ranks + recall at the Flickr30K test split's shape
    Ni = args.rank_images
    S = torch.rand(Ni, 5 * Ni, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    i2t = torch.empty(2, Ni, dtype=torch.int32, device=dev)
    t2i = torch.empty(2, 5 * Ni, dtype=torch.int32, device=dev)
    nan = torch.empty(1, dtype=torch.int32, device=dev)

    def kernel():
        L.check(L.lib().mmnas_rank_matrix(L.fptr(S), Ni, 5 * Ni, S.stride(0), L.ptr(i2t[0]), L.ptr(i2t[1]), L.ptr(t2i[0]),
                                          L.ptr(t2i[1]), L.ptr(nan), L.stream()))
    kernel()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ks = []
    for _ in range(20):
        e0.record()
        kernel()
        e1.record()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1) * 1e3)
    retrieval.recall_at_k(S)
    calls = [timed(lambda: retrieval.recall_at_k(S))[1] * 1e3 for _ in range(5)]
    per_img = numpy_reference_ranks(S.cpu().numpy(), min(args.numpy_rows, Ni))
    print('recall_at_k %d x %d: rank kernels %.1f us (median of 20, HIP events), whole call %.2f ms (median of 5); '
          'reference numpy loops %.1f ms per image -> ~%.1f s for the i2t pass' %
          (Ni, 5 * Ni, statistics.median(ks), statistics.median(calls), per_img * 1e3, per_img * Ni))
    print(json.dumps({'tool': 'itm_retrieval_ab', 'images': args.images, 'captions': args.captions, 'rounds': args.rounds,
                      'a_pairs_per_s': pairs / statistics.median(ta), 'b_pairs_per_s': pairs / statistics.median(tb),
                      'b_over_a': ratio, 'max_abs_diff': diff, 'a_s': ta, 'b_s': tb,
                      'rank_kernel_us': statistics.median(ks), 'recall_call_ms': statistics.median(calls),
                      'numpy_ref_ms_per_image': per_img * 1e3}))


if __name__ == '__main__':
    main()
