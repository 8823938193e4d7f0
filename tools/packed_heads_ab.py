"""A/B of the ragged decoder stream (ops.set_unpad) on a supernet whose attention candidates have heads of 16 / 32 / 128 / 256: whole
SearchLoop weight steps with the switch off and on, alternating in ONE process.

The search space is patched for this process (the registry's candidate lists are an OpsAdapter instance's dict):
  enc: self_att_32, self_att_128, feed_forward;  dec: self_att_16, rel_self_att_32, guided_att_128, guided_att_256
at the search dimensions (HSIZE 256, B = 64, 100 regions with bench.py's region counts, 14 tokens).  Each side runs --inner steps
back to back between two device events; off and on alternate, --rounds (9) each; medians and min..max per side are printed and
appended to --out.  Every block samples the same architectures (the sampler is re-seeded per block).

  python tools/packed_heads_ab.py [--rounds 9] [--inner 5] [--out profiles/r16_packed_heads_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmnas_amd import _lib  # noqa: E402,F401   (before the first CUDA call: the library sets its launch configuration at import)

DEV = 'cuda:0'
SEED = 20261021
ENC = ['self_att_32', 'self_att_128', 'feed_forward']
DEC = ['self_att_16', 'rel_self_att_32', 'guided_att_128', 'guided_att_256']
PRIOR = {'enc': ['self_att_32', 'feed_forward'] * 6, 'dec': ['rel_self_att_32', 'guided_att_128', 'guided_att_256'] * 6}


def timed_block(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', default=os.path.join('profiles', 'r16_packed_heads_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('packed_heads_ab.py measures on the GPU; no device is visible')
    import bench
    from mmnas_amd import ops
    from mmnas_amd.harness import SearchLoop
    from mmnas_amd.model import mixed, nets
    for ad in (mixed.OPS_ADAPTER, nets.OPS_ADAPTER):
        ad.Used_OPS.update(enc_safe=list(ENC), dec_safe=list(DEC), enc=ENC + ['none'], dec=DEC + ['none'])
    nets._PRIOR = PRIOR
    from mmnas.model.hygr_vqa import Net_Search
    cfg = bench.make_cfg('search')
    cpu_in, cpu_tg = bench.synth_batch(cfg, 64, bench.SX, bench.SY, bench.VOCAB, bench.ANS, 777)
    inp, tgt = tuple(t.to(DEV) for t in cpu_in), cpu_tg.to(DEV)
    counts = (cpu_in[0].abs().sum(-1) != 0).sum(1)
    torch.manual_seed(SEED)
    ops.manual_seed(SEED)
    emb = torch.randn(bench.VOCAB, 300, generator=torch.Generator().manual_seed(1)).numpy()
    net = Net_Search(cfg, {'token_size': bench.VOCAB, 'ans_size': bench.ANS, 'pretrained_emb': emb}).to(DEV).train()
    loop = SearchLoop(net, arch_mode='full')
    seen = []
    o_apply = ops.BackboneFn.apply
    ops.BackboneFn.apply = lambda *a: (seen.append(a[10] is not None), o_apply(*a))[1]

    def run(on, n):
        mixed.seed_arch_sampler(4000)
        prev = ops.set_unpad(on)
        try:
            return timed_block(lambda: loop.weight_step(inp, tgt), n)
        finally:
            ops.set_unpad(prev)

    res = {'off': [], 'on': []}
    try:
        for k in res:
            del seen[:]
            run(k == 'on', 2)
            assert seen == [k == 'on'] * 2, (k, seen)     # the chain ran, ragged exactly when the switch is on
        for _ in range(args.rounds):
            for k in res:
                res[k].append(run(k == 'on', args.inner))
    finally:
        ops.BackboneFn.apply = o_apply
        loop.reducer.fg.disable_sinks()
    lines = ['%s: supernet weight step, HSIZE 256, B = 64, 14 tokens, %d regions padded to %d (valid per image %d..%d, mean %.1f)' % (
                 torch.cuda.get_device_name(0), bench.SY, bench.SY, int(counts.min()), int(counts.max()), float(counts.float().mean())),
             '  candidates  enc: %s   dec: %s' % (', '.join(ENC), ', '.join(DEC)),
             '  ops.set_unpad off / on alternating in one process, %d rounds of %d steps between device events, median (min .. max) ms per step' % (
                 args.rounds, args.inner)]
    text = ' '
    for k in ('off', 'on'):
        text += '  %-3s %8.3f ms (%8.3f .. %8.3f)' % (k, statistics.median(res[k]), min(res[k]), max(res[k]))
    lines.append(text + '   off/on %5.2fx' % (statistics.median(res['off']) / statistics.median(res['on'])))
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
