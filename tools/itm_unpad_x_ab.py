"""A/B of the ragged language stream (ops.set_unpad_x): whole steps with the switch off and on, alternating in ONE process.

CAPTION LENGTHS ARE SYNTHETIC: drawn with a fixed seed (20261020) from a clipped normal -- mean 12, sd 3, rounded, clipped to
5..30 tokens -- under the 50-token padding of the ITM loaders (load_data_itm.py:94-97 pad to the longest caption of the dataset).
That distribution is a STAND-IN for "captions are a fraction of 50 tokens long", not a statistic of any dataset.  A second run
(--lengths long) draws the lengths uniformly from 40..50: the case where trimming and packing cannot pay.  VQA questions keep
bench.py's lengths (uniform 3..14 under 14 tokens), where the stream stays dense.

  train_itm   the fixed-architecture ITM net at the train_itm dimensions (HSIZE 512, B = 160, 36 regions, 50-token padding):
              itm_triplet_step (three forwards, one backward, flat gradient buffer) and a TrainLoop step over the 3B
              triplet_batch (forward, fused loss, backward, clip, Adam);
  search_itm  the ITM supernet at the search_itm dimensions (HSIZE 256, B = 64): SearchLoop weight step and arch step
              (mode 'full') over the 3B triplet_batch;
  train_vqa / search_vqa  TrainLoop step / SearchLoop weight + arch step at 14 tokens (B = 64, 100 regions).

Each side runs --inner steps back to back between two device events; off and on alternate, --rounds (9) each; medians and
min..max per side are printed.  The sides share one net and one optimizer state (the switch changes no result beyond
round-off), so a later block sees the weights an earlier one left.  The lengths ride on the token tensors (`_mmnas_lengths`, what
data.DevicePrefetcher(lengths=...) attaches), so the plan costs no device-to-host copy.

  python tools/itm_unpad_x_ab.py [--lengths short|long] [--rounds 9] [--inner 5] [--only train_itm,search_itm,...]
                                 [--off-only] [--out profiles/r15_itm_unpad_x_ab.txt]

--off-only: the switch-off side alone (no call into the switch: runs on a commit without it), for the parent-commit line.
The table is appended to --out.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmnas_amd import _lib  # noqa: E402,F401   (before the first CUDA call: the library sets its launch configuration at import)

DEV = 'cuda:0'
SEED = 20261020
PAD_ITM = 50


def caption_lengths(n, kind, rs):
    if kind == 'long':
        return rs.randint(40, 51, n)
    return np.clip(np.rint(rs.normal(12.0, 3.0, n)), 5, 30).astype(np.int64)


def timed_block(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def ab(name, fn, sides, rounds, inner, lines, warm=2):
    from mmnas.model import mixed
    from mmnas_amd import ops
    setter = getattr(ops, 'set_unpad_x', None)

    def run(on, n):
        mixed.seed_arch_sampler(4000)      # (search loops: every block samples the same architectures)
        prev = setter(on) if setter is not None else None
        try:
            return timed_block(fn, n)
        finally:
            if setter is not None:
                setter(prev)

    res = {k: [] for k in sides}
    for k in sides:
        run(k == 'on', warm)
    for _ in range(rounds):
        for k in sides:
            res[k].append(run(k == 'on', inner))
    text = '  %-44s' % name
    for k in sides:
        text += '  %-3s %8.3f ms (%8.3f .. %8.3f)' % (k, statistics.median(res[k]), min(res[k]), max(res[k]))
    if len(sides) == 2:
        text += '   off/on %5.2fx' % (statistics.median(res['off']) / statistics.median(res['on']))
    print(text)
    lines.append(text)


def with_lengths(ix, lens):
    """Token indices [B, T] with zeros behind each sample's length, on the device, the counts attached."""
    ix = ix.clone()
    for b, n in enumerate(lens):
        ix[b, int(n):] = 0
    t = ix.to(DEV)
    t._mmnas_lengths = [int(n) for n in lens]
    return t


def itm_batches(cfg, B, kind):
    """(pos, neg) 5-tuples at the ITM dimensions: 36 regions, none padded; captions padded to 50 tokens."""
    import bench
    out = []
    rs = np.random.RandomState(SEED)
    for seed in (1, 2):
        (frcn, bbox, y_rel, ques, x_rel), _ = bench.synth_batch(cfg, B, PAD_ITM, 36, bench.VOCAB, 1, SEED + seed)
        g = torch.Generator().manual_seed(SEED + 10 + seed)
        frcn = torch.relu(torch.randn(frcn.shape, generator=g)) + 0.01     # every image carries all 36 regions
        y_rel = torch.randn(y_rel.shape, generator=g)
        ques = torch.randint(1, bench.VOCAB, ques.shape, generator=g)
        lens = caption_lengths(B, kind, rs)
        x_rel = torch.randn(x_rel.shape, generator=g)
        for b, n in enumerate(lens):
            x_rel[b, int(n):] = 0
            x_rel[b, :, int(n):] = 0
        out.append((frcn.to(DEV), bbox.to(DEV), y_rel.to(DEV), with_lengths(ques, lens), x_rel.to(DEV)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lengths', choices=('short', 'long'), default='short')
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--only', default='train_itm,search_itm,train_vqa,search_vqa')
    ap.add_argument('--off-only', action='store_true')
    ap.add_argument('--out', default=os.path.join('profiles', 'r15_itm_unpad_x_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('itm_unpad_x_ab.py measures on the GPU; no device is visible')
    import bench
    from mmnas_amd import dp, losses as FL, ops
    from mmnas_amd.harness import BCE_Loss, BatchedTriplet, SearchLoop, TrainLoop, itm_triplet_step, triplet_batch
    sides = ('off',) if args.off_only else ('off', 'on')
    only = args.only.split(',')
    lines = ['%s: caption lengths %s, %d alternating rounds of %d steps, median (min .. max) ms per step%s' % (
        torch.cuda.get_device_name(0), 'clipped normal(12, 3) in 5..30 [synthetic stand-in]' if args.lengths == 'short' else 'uniform 40..50',
        args.rounds, args.inner, ', switch-off side only' if args.off_only else '')]
    print(lines[0])
    emb = torch.randn(bench.VOCAB, 300, generator=torch.Generator().manual_seed(1)).numpy()

    def init(ans):
        return {'token_size': bench.VOCAB, 'ans_size': ans, 'pretrained_emb': emb}

    torch.manual_seed(SEED)
    ops.manual_seed(SEED)
    if 'train_itm' in only:
        from mmnas.model.full_itm import Net_Full
        cfg = bench.make_cfg('train_itm')
        pos, neg = itm_batches(cfg, 160, args.lengths)
        net = Net_Full(cfg, init(1)).to(DEV).train()
        red = dp.GradReducer(list(net.parameters()))
        fn = FL.fused(BCE_Loss())
        try:
            ab('train_itm itm_triplet_step B=160', lambda: itm_triplet_step(net, fn, pos, neg, reducer=red), sides, args.rounds, args.inner, lines)
        finally:
            red.fg.disable_sinks()
        del net, red
        net = Net_Full(cfg, init(1)).to(DEV).train()
        loop = TrainLoop(net, loss_fn=BatchedTriplet(FL.fused(BCE_Loss())), lr=1e-5)
        try:
            ab('train_itm TrainLoop step, triplet_batch 3x160', lambda: loop.step(triplet_batch(pos, neg), None), sides, args.rounds, args.inner, lines)
        finally:
            loop.reducer.fg.disable_sinks()
        del net, loop
    if 'search_itm' in only:
        from mmnas.model.hygr_itm import Net_Search
        cfg = bench.make_cfg('search')
        pos, neg = itm_batches(cfg, 64, args.lengths)
        net = Net_Search(cfg, init(1)).to(DEV).train()
        loop = SearchLoop(net, loss_fn=BatchedTriplet(BCE_Loss()), arch_mode='full')
        try:
            ab('search_itm weight step, triplet_batch 3x64', lambda: loop.weight_step(triplet_batch(pos, neg), None), sides, args.rounds, args.inner, lines)
            ab("search_itm arch step 'full', triplet_batch 3x64", lambda: loop.arch_step(triplet_batch(pos, neg), None), sides, args.rounds, args.inner,
               lines)
        finally:
            loop.reducer.fg.disable_sinks()
        del net, loop
    for which in ('train_vqa', 'search_vqa'):
        if which not in only:
            continue
        cfg = bench.make_cfg('train' if which == 'train_vqa' else 'search')
        cpu_in, cpu_tg = bench.synth_batch(cfg, 64, bench.SX, bench.SY, bench.VOCAB, bench.ANS, 777)
        lens = (cpu_in[3] != 0).sum(1).tolist()
        inp = tuple(t.to(DEV) for t in cpu_in[:3]) + (with_lengths(cpu_in[3], lens), cpu_in[4].to(DEV))
        tgt = cpu_tg.to(DEV)
        if which == 'train_vqa':
            from mmnas.model.full_vqa import Net_Full as VqaNet
            loop = TrainLoop(VqaNet(cfg, init(bench.ANS)).to(DEV).train(), lr=1e-5)
            try:
                ab('train_vqa TrainLoop step B=64, 14 tokens', lambda: loop.step(inp, tgt), sides, args.rounds, args.inner, lines)
            finally:
                loop.reducer.fg.disable_sinks()
        else:
            from mmnas.model.hygr_vqa import Net_Search as VqaSearch
            loop = SearchLoop(VqaSearch(cfg, init(bench.ANS)).to(DEV).train(), arch_mode='full')
            try:
                ab('search_vqa weight step B=64, 14 tokens', lambda: loop.weight_step(inp, tgt), sides, args.rounds, args.inner, lines)
                ab("search_vqa arch step 'full' B=64, 14 tokens", lambda: loop.arch_step(inp, tgt), sides, args.rounds, args.inner, lines)
            finally:
                loop.reducer.fg.disable_sinks()
        del loop
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
