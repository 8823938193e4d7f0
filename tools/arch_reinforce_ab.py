"""What an architecture step costs by mode at the benchmark's VQA supernet (bench.py's Net_Search and batch), one process, one
net and one SearchLoop per side, all from the same weights:

  two-fused          SearchLoop(arch_mode='two', fused_arch_update=True)
  full               SearchLoop(arch_mode='full')
  reinforce-M-negloss   SearchLoop(arch_mode='reinforce', reinforce_samples=M, reward_form='add'), the default NegLossReward
  reinforce-M-soft      the same with answering.SoftAccuracyReward()          M in 1, 2, 4, 8

The sides alternate (order reversed every other round) over --rounds rounds; each block is --inner arch_step() calls between
two device events with the host clock around the same block (closed by a synchronise).  Medians and min..max are reported.
Per side also: the device operations of one arch step (kernels and memory operations in torch.profiler's device events) and
the peak of torch's allocator over one arch step above what was allocated before it.

No ratio is fixed in advance: the file says what came out, and from it the M at which 'reinforce' stops being cheaper than
'two'-fused and than 'full'.  profiles/r17_arch_reinforce_resources.txt (registers, LDS, scratch of the update kernels, from
the compiler's resource remarks) is appended when it exists.

  python tools/arch_reinforce_ab.py [--rounds 9 --inner 4 --batch 64 --out profiles/r17_arch_reinforce_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmnas_amd import _lib  # noqa: E402,F401   (before the first CUDA call: the library sets its launch configuration at import)

DEV = 'cuda:0'
SAMPLES = (1, 2, 4, 8)


def timed_block(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, (time.perf_counter() - t0) * 1e6 / inner


def device_ops(fn):
    """Device events (kernels, copies, memsets) of one call, counted by torch.profiler."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = 0
    for e in prof.events():
        if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower():
            n += 1
    return n


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=4, help='arch steps per timed block')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join('profiles', 'r17_arch_reinforce_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('arch_reinforce_ab.py measures on the GPU; no device is visible')
    import bench
    from mmnas.model import mixed
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import answering, ops
    from mmnas_amd.harness import SearchLoop, fused_loss

    torch.manual_seed(888)
    ops.manual_seed(888)
    cfg = bench.make_cfg('search')
    emb = torch.randn(bench.VOCAB, 300, generator=torch.Generator().manual_seed(1)).numpy()
    init = {'token_size': bench.VOCAB, 'ans_size': bench.ANS, 'pretrained_emb': emb}
    loss_fn = fused_loss(torch.nn.BCEWithLogitsLoss(reduction='sum'))
    cpu_in, cpu_tg = bench.synth_batch(cfg, args.batch, bench.SX, bench.SY, bench.VOCAB, bench.ANS, 777)
    inp, tgt = tuple(t.to(DEV) for t in cpu_in), cpu_tg.to(DEV)

    sides = {'two-fused': dict(arch_mode='two', fused_arch_update=True), 'full': dict(arch_mode='full')}
    for M in SAMPLES:
        sides['reinforce-%d-negloss' % M] = dict(arch_mode='reinforce', reinforce_samples=M, reward_form='add')
        sides['reinforce-%d-soft' % M] = dict(arch_mode='reinforce', reinforce_samples=M, reward=answering.SoftAccuracyReward())
    names = list(sides)
    first = Net_Search(cfg, init)
    state = first.state_dict()
    loops = {}
    try:
        for k in names:
            net = first if k == names[0] else Net_Search(cfg, init)
            net.load_state_dict(state)
            loops[k] = SearchLoop(net.to(DEV).train(), loss_fn, **sides[k])
        step = {k: (lambda k=k: loops[k].arch_step(inp, tgt)) for k in names}
        mixed.seed_arch_sampler(5000)
        for k in names:                           # warm-up
            for _ in range(2):
                step[k]()
        ops_n = {k: device_ops(step[k]) for k in names}
        peak = {k: peak_bytes(step[k]) for k in names}
        res = {k: {'dev': [], 'host': []} for k in names}
        for r in range(args.rounds):
            for k in (names if r % 2 == 0 else names[::-1]):
                dv, h = timed_block(step[k], args.inner)
                res[k]['dev'].append(dv)
                res[k]['host'].append(h)
        errs = {k: int(loops[k].alpha_optim.err) for k in names if k.startswith('reinforce')}
    finally:
        MixedOp.MODE = None
        for loop in loops.values():
            loop.reducer.fg.disable_sinks()

    med = {k: {c: statistics.median(v[c]) for c in v} for k, v in res.items()}
    rng = {k: {c: (min(v[c]), max(v[c])) for c in v} for k, v in res.items()}
    lines = ['SearchLoop.arch_step by mode, benchmark VQA supernet (30 nodes), batch %d, %s; medians of %d alternating rounds, %d arch '
             'steps per block' % (args.batch, torch.cuda.get_device_name(0), args.rounds, args.inner),
             '  %-22s %12s %12s %12s %12s' % ('side', 'device us', 'host us', 'device ops', 'peak MiB')]
    for k in names:
        lines.append('  %-22s %12.1f %12.1f %12d %12.1f   (device min..max %.1f..%.1f, host %.1f..%.1f)'
                     % (k, med[k]['dev'], med[k]['host'], ops_n[k], peak[k] / 2.0 ** 20, rng[k]['dev'][0], rng[k]['dev'][1],
                        rng[k]['host'][0], rng[k]['host'][1]))
    for ref in ('two-fused', 'full'):
        for rw in ('negloss', 'soft'):
            cheaper = [M for M in SAMPLES if med['reinforce-%d-%s' % (M, rw)]['host'] < med[ref]['host']]
            first_not = next((M for M in SAMPLES if M not in cheaper), None)
            lines.append("  reward %-8s against '%s' (host us per step): cheaper at M in %s; stops being cheaper at M = %s"
                         % (rw, ref, cheaper or 'none', first_not if first_not is not None else 'beyond %d' % SAMPLES[-1]))
    lines.append('  err flags after the run (0: every reward was finite): %s' % json.dumps(errs))
    lines.append(json.dumps(dict(tool='arch_reinforce_ab', batch=args.batch, rounds=args.rounds, inner=args.inner, median_us=med,
                                 min_max_us=rng, device_ops=ops_n, peak_bytes=peak)))
    extra = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'r17_arch_reinforce_resources.txt')
    if os.path.exists(extra):
        with open(extra) as f:
            lines += ['', f.read().rstrip()]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
