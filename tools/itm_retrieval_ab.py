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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8)
    ap.add_argument('--captions', type=int, default=5000)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--pair-batch', type=int, default=1024)
    ap.add_argument('--caption-chunk', type=int, default=1000)
    ap.add_argument('--rank-images', type=int, default=1000)
    ap.add_argument('--numpy-rows', type=int, default=20)
    args = ap.parse_args()
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
