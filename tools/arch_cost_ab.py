"""A/B of the architecture step with and without the expected-cost term at the benchmark's VQA supernet (bench.py's
Net_Search and batch: 30 nodes, 12 of width 2 and 18 of width 4), one process, per mode two loops over two nets with the
same weights:

  off   SearchLoop(arch_mode=mode, fused_arch_update=True): ArchAdam, one mmnas_alpha_full_step / mmnas_alpha_two_step launch;
  on    the same with cost_table=<flop table>, cost_weight=0.1, cost_form='log': one mmnas_alpha_*_step_cost launch.

Two measurements per mode, each between two device events and with the host clock around the same block (closed by a
synchronise), the sides alternating, --rounds each, medians and ranges reported:

  update  the update alone -- gate gradients in, alphas out -- from the gate gradients (and pairs) of one arch step;
  step    a whole arch_step(): sampling, forward, backward, the update.

Before every timed block the alphas, the optimizer's moments and the sampler's seed are put back, so both sides walk the same
sequence of samples.  The expectation is no measurable difference (one launch either way); the file says what came out.

  python tools/arch_cost_ab.py [--rounds 9 --inner 20 --inner-step 6 --batch 64 --out profiles/r14_arch_cost_ab.txt]
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
SIDES = ('off', 'on')


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20, help='updates per timed block')
    ap.add_argument('--inner-step', type=int, default=6, help='arch steps per timed block')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join('profiles', 'r14_arch_cost_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('arch_cost_ab.py measures on the GPU; no device is visible')
    import bench
    from mmnas.model import mixed
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import ops
    from mmnas_amd.cost import flop_cost_table
    from mmnas_amd.harness import SearchLoop, fused_loss

    torch.manual_seed(888)
    ops.manual_seed(888)
    cfg = bench.make_cfg('search')
    emb = torch.randn(bench.VOCAB, 300, generator=torch.Generator().manual_seed(1)).numpy()
    init = {'token_size': bench.VOCAB, 'ans_size': bench.ANS, 'pretrained_emb': emb}
    loss_fn = fused_loss(torch.nn.BCEWithLogitsLoss(reduction='sum'))
    cpu_in, cpu_tg = bench.synth_batch(cfg, args.batch, bench.SX, bench.SY, bench.VOCAB, bench.ANS, 777)
    inp, tgt = tuple(t.to(DEV) for t in cpu_in), cpu_tg.to(DEV)
    med, rng, moved = {}, {}, {}
    for mode in ('full', 'two'):
        torch.manual_seed(888)      # (a fresh pair of nets per mode: a loop owns its net's gradient sinks)
        first = Net_Search(cfg, init)
        second = Net_Search(cfg, init)
        second.load_state_dict(first.state_dict())
        nets = {'off': first.to(DEV).train(), 'on': second.to(DEV).train()}
        table = flop_cost_table(nets['on'], bench.SX, bench.SY)
        alpha0 = nets['off']._flat_alphas()[0].clone()
        loops = {'off': SearchLoop(nets['off'], loss_fn, arch_mode=mode, fused_arch_update=True),
                 'on': SearchLoop(nets['on'], loss_fn, arch_mode=mode, fused_arch_update=True, cost_table=table, cost_weight=0.1,
                                  cost_form='log')}
        assert loops['off'].alpha_optim.cost is None and loops['on'].alpha_optim.cost is not None

        def put_back(k, seed):
            nets[k]._flat_alphas()[0].copy_(alpha0)
            opt = loops[k].alpha_optim
            opt.m.zero_()
            opt.v.zero_()
            opt.steps = 0
            for m in nets[k].redundant_modules:
                m.alpha_version += 1
            mixed.seed_arch_sampler(seed)

        try:
            for k in SIDES:      # one arch step without the update: gate gradients (and pairs) for the update-alone timing
                put_back(k, 4000)
                loops[k].arch_step(inp, tgt, optimize=False)
            nets['on']._flat_grads[0].copy_(nets['off']._flat_grads[0])
            update = {k: loops[k].alpha_optim.step for k in SIDES}
            step = {k: (lambda k=k: loops[k].arch_step(inp, tgt)) for k in SIDES}
            for k in SIDES:
                update[k]()
            torch.cuda.synchronize()
            a, b = (nets[k]._flat_alphas()[0] for k in SIDES)
            fin = torch.isfinite(a)
            moved[mode] = float((a[fin] - b[fin]).abs().max())      # what the term changed in one update
            res = {what: {k: {'dev': [], 'host': []} for k in SIDES} for what in ('update', 'step')}
            for what, fns, inner in (('update', update, args.inner), ('step', step, args.inner_step)):
                for k in SIDES:                       # warm-up
                    put_back(k, 5000)
                    for _ in range(3):
                        fns[k]()
                for r in range(args.rounds):
                    for k in (SIDES if r % 2 == 0 else SIDES[::-1]):
                        put_back(k, 6000 + r)
                        dv, h = timed_block(fns[k], inner)
                        res[what][k]['dev'].append(dv)
                        res[what][k]['host'].append(h)
            med[mode] = {w: {k: {c: statistics.median(v[c]) for c in v} for k, v in r.items()} for w, r in res.items()}
            rng[mode] = {w: {k: {c: (min(v[c]), max(v[c])) for c in v} for k, v in r.items()} for w, r in res.items()}
        finally:
            MixedOp.MODE = None
            for loop in loops.values():
                loop.reducer.fg.disable_sinks()

    label = {'off': 'without the term', 'on': "cost_table, weight 0.1, 'log'"}
    lines = ['Architecture step with / without the expected-cost term, benchmark VQA supernet (30 nodes), batch %d, %s; medians of %d '
             'alternating rounds (%d updates / %d arch steps per block)'
             % (args.batch, torch.cuda.get_device_name(0), args.rounds, args.inner, args.inner_step)]
    for mode in ('full', 'two'):
        for what, title in (('update', 'the update alone (gate gradients in, alphas out), us per update'),
                            ('step', 'a whole arch_step(), us per step')):
            lines.append("  mode '%s': %s" % (mode, title))
            lines.append('    %-32s %12s %12s' % ('side', 'device us', 'host us'))
            for k in SIDES:
                m, g = med[mode][what][k], rng[mode][what][k]
                lines.append('    %-32s %12.1f %12.1f   (device min..max %.1f..%.1f, host %.1f..%.1f)'
                             % (label[k], m['dev'], m['host'], g['dev'][0], g['dev'][1], g['host'][0], g['host'][1]))
            off, on = med[mode][what]['off'], med[mode][what]['on']
            spread = max((rng[mode][what][k]['host'][1] - rng[mode][what][k]['host'][0]) / med[mode][what][k]['host'] for k in SIDES)
            lines.append('    on - off: %+.1f us device, %+.1f us host (%+.1f %% of the off side; the widest min..max range of a side is '
                         '%.1f %% of its median)' % (on['dev'] - off['dev'], on['host'] - off['host'],
                                                     100.0 * (on['host'] - off['host']) / off['host'], 100.0 * spread))
        lines.append("  mode '%s': largest alpha difference after one update with / without the term: %.3g" % (mode, moved[mode]))
    lines.append(json.dumps(dict(tool='arch_cost_ab', batch=args.batch, rounds=args.rounds, inner=args.inner, inner_step=args.inner_step,
                                 median_us=med, min_max_us=rng, alpha_diff_after_one_update=moved)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
