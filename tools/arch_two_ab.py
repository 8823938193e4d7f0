"""A/B of the ALPHA_BINARY_MODE 'two' architecture update at the benchmark's VQA supernet (bench.py's Net_Search and batch:
30 nodes, 12 of width 2 and 18 of width 4), one process, two loops over two nets with the same weights:

  torch   SearchLoop(arch_mode='two'): per node MixedOp.set_arch_param_grad over the sampled pair, torch.optim.Adam over
          the 30 alpha_prob parameters, per node rescale_updated_arch_param (search_vqa.py:330-335, mixed.py:179-208);
  fused   SearchLoop(arch_mode='two', fused_arch_update=True): ArchAdam(mode='two'), one mmnas_alpha_two_step launch.

Two measurements, each between two device events and with the host clock around the same block (closed by a
synchronise), the sides alternating, --rounds each, medians and ranges reported:

  update  the update alone -- gate gradients in, alphas out -- from the gate gradients and pairs of one arch step;
  step    a whole arch_step(): sampling, forward of two candidates per node, backward, the update.

Before every timed block the alphas and the sampler's seed are put back, so both sides walk the same sequence of pairs.
The launches per update / step are counted with torch.profiler in a pass of their own.

  python tools/arch_two_ab.py [--rounds 9 --inner 20 --inner-step 6 --batch 64 --out profiles/r09_arch_two_ab.txt]
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

from mmnas_amd import _lib  # noqa: E402,F401   (before the first CUDA call: the library sets its launch configuration at import)

DEV = 'cuda:0'


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


def count_launches(fn, reps=4):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n / float(reps) if n else None
    except Exception as exc:     # the count is an extra; the timings stand without it
        print('  (launch count unavailable: %s)' % (exc,))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20, help='updates per timed block')
    ap.add_argument('--inner-step', type=int, default=6, help='arch steps per timed block')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--out', default=os.path.join('profiles', 'r09_arch_two_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('arch_two_ab.py measures on the GPU; no device is visible')
    import bench
    from mmnas.model import mixed
    from mmnas.model.hygr_vqa import Net_Search
    from mmnas.model.mixed import MixedOp
    from mmnas_amd import ops
    from mmnas_amd.harness import ArchAdam, SearchLoop, fused_loss

    torch.manual_seed(888)
    ops.manual_seed(888)
    cfg = bench.make_cfg('search')
    emb = torch.randn(bench.VOCAB, 300, generator=torch.Generator().manual_seed(1)).numpy()
    init = {'token_size': bench.VOCAB, 'ans_size': bench.ANS, 'pretrained_emb': emb}
    loss_fn = fused_loss(torch.nn.BCEWithLogitsLoss(reduction='sum'))
    first = Net_Search(cfg, init)
    nets = {'torch': first.to(DEV).train()}
    second = Net_Search(cfg, init)
    second.load_state_dict(first.state_dict())
    nets['fused'] = second.to(DEV).train()
    loops = {'torch': SearchLoop(nets['torch'], loss_fn, arch_mode='two'),
             'fused': SearchLoop(nets['fused'], loss_fn, arch_mode='two', fused_arch_update=True)}
    assert isinstance(loops['torch'].alpha_optim, torch.optim.Adam) and isinstance(loops['fused'].alpha_optim, ArchAdam)
    cpu_in, cpu_tg = bench.synth_batch(cfg, args.batch, bench.SX, bench.SY, bench.VOCAB, bench.ANS, 777)
    inp, tgt = tuple(t.to(DEV) for t in cpu_in), cpu_tg.to(DEV)
    sides = ('torch', 'fused')
    try:
        # one arch step without the update on both sides: the same pairs, each side's own gate gradients
        for k in sides:
            mixed.seed_arch_sampler(4000)
            loops[k].arch_step(inp, tgt, optimize=False)
        pairs = {k: [(m.active_index[0], m.inactive_index[0]) for m in nets[k].redundant_modules] for k in sides}
        assert pairs['torch'] == pairs['fused']
        nets['fused']._flat_grads[0].copy_(nets['torch']._flat_grads[0])       # one backward's gate gradients for both
        alpha0 = {k: nets[k]._flat_alphas()[0].clone() for k in sides}
        assert torch.equal(alpha0['torch'], alpha0['fused'])

        def update_torch():
            net = nets['torch']
            MixedOp.MODE = 'two'
            try:
                for m in net.redundant_modules:
                    m.alpha_prob.grad = None
                net.set_arch_param_grad()
                loops['torch'].alpha_optim.step()
                net.rescale_updated_arch_param()
            finally:
                MixedOp.MODE = None

        update = {'torch': update_torch, 'fused': loops['fused'].alpha_optim.step}
        step = {k: (lambda k=k: loops[k].arch_step(inp, tgt)) for k in sides}

        def put_back(k, seed):
            nets[k]._flat_alphas()[0].copy_(alpha0[k])
            for m in nets[k].redundant_modules:
                m.alpha_version += 1
            mixed.seed_arch_sampler(seed)

        # agreement first: one update on both sides from the same alphas, pairs and gate gradients
        for k in sides:
            update[k]()
        torch.cuda.synchronize()
        a, b = (nets[k]._flat_alphas()[0].cpu().numpy() for k in sides)
        fin = np.isfinite(a)
        worst = float(np.abs(a[fin] - b[fin]).max() / np.abs(a[fin]).max())
        moved = float(np.abs(a[fin] - alpha0['torch'].cpu().numpy()[fin]).max())
        assert np.array_equal(fin, np.isfinite(b)) and worst < 1e-5 and moved > 0.05, (worst, moved)

        res = {what: {k: {'dev': [], 'host': []} for k in sides} for what in ('update', 'step')}
        for what, fns, inner in (('update', update, args.inner), ('step', step, args.inner_step)):
            for k in sides:                       # warm-up
                put_back(k, 5000)
                for _ in range(3):
                    fns[k]()
            for r in range(args.rounds):
                for k in (sides if r % 2 == 0 else sides[::-1]):
                    put_back(k, 6000 + r)
                    d, h = timed_block(fns[k], inner)
                    res[what][k]['dev'].append(d)
                    res[what][k]['host'].append(h)
        med = {w: {k: {c: statistics.median(v[c]) for c in v} for k, v in r.items()} for w, r in res.items()}
        rng = {w: {k: {c: (min(v[c]), max(v[c])) for c in v} for k, v in r.items()} for w, r in res.items()}
        launches = {}
        for what, fns in (('update', update), ('step', step)):
            launches[what] = {}
            for k in sides:
                put_back(k, 7000)
                launches[what][k] = count_launches(fns[k])
    finally:
        MixedOp.MODE = None
        for loop in loops.values():
            loop.reducer.fg.disable_sinks()

    label = {'torch': "per-node statements + torch Adam", 'fused': "ArchAdam(mode='two'), one launch"}
    lines = ["ALPHA_BINARY_MODE 'two' architecture update, benchmark VQA supernet (30 nodes), batch %d, %s; medians of %d "
             'alternating rounds (%d updates / %d arch steps per block)'
             % (args.batch, torch.cuda.get_device_name(0), args.rounds, args.inner, args.inner_step)]
    for what, title in (('update', 'the update alone (gate gradients in, alphas out), us per update'),
                        ('step', "a whole arch_step() in mode 'two', us per step")):
        lines.append('  %s' % title)
        lines.append('    %-36s %12s %12s %10s' % ('side', 'device us', 'host us', 'launches'))
        for k in sides:
            lines.append('    %-36s %12.1f %12.1f %10s   (device min..max %.1f..%.1f, host %.1f..%.1f)'
                         % (label[k], med[what][k]['dev'], med[what][k]['host'], launches[what][k], rng[what][k]['dev'][0],
                            rng[what][k]['dev'][1], rng[what][k]['host'][0], rng[what][k]['host'][1]))
        lines.append('    torch / fused: %.2fx (device events), %.2fx (host clock)'
                     % (med[what]['torch']['dev'] / med[what]['fused']['dev'], med[what]['torch']['host'] / med[what]['fused']['host']))
    t, f = med['step']['torch']['host'], med['step']['fused']['host']
    spread = max((rng['step'][k]['host'][1] - rng['step'][k]['host'][0]) / med['step'][k]['host'] for k in sides)
    lines.append('  whole step: the medians differ by %.1f %% of the torch side; the widest min..max range of a side is %.1f %% of its '
                 'median' % (100.0 * (t - f) / t, 100.0 * spread))
    lines.append('  share of a torch-path arch step spent in its update (host clock): %.1f %%'
                 % (100.0 * med['update']['torch']['host'] / med['step']['torch']['host']))
    lines.append(json.dumps(dict(tool='arch_two_ab', batch=args.batch, rounds=args.rounds, inner=args.inner, inner_step=args.inner_step,
                                 median_us=med, min_max_us=rng, launches=launches, max_rel_diff_after_one_update=worst)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
