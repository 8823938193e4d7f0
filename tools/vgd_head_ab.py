"""A/B of the grounding head (full_vgd.py:105-114): the composition the VGD nets run by default -- broadcast add, ops.layer_norm,
two ops.linear, log_softmax, one autograd node each -- against ops.grounding_head (csrc/vgdhead.hip, switch MMNAS_VGD_HEAD), in one
process on one device.

  micro  the head alone, forward + backward, at B = 64, S = 100, F = 1024 ('kld' mode: with the log_softmax): --inner calls back
         to back between two device events; the two sides alternate, --rounds each; medians (device events, and the host clock
         around the same block closed by a synchronise), the ratio, kernel launches per call by torch.profiler, and the peak
         allocated memory of one forward + backward above what is live before it.
  step   one whole TrainLoop step of the VGD Net_Full at the train_vgd dimensions (HSIZE 512, B = 64, 100 regions, VgdLoss) with
         the switch off and on -- the same loop and weights, the switch flipped between the alternating blocks -- with the same
         launch count and peak-memory figures.

  python tools/vgd_head_ab.py [--rounds 9 --inner 50 --step-rounds 7 --step-inner 10 --no-step --out FILE]

Prints the table, then one JSON line; --out receives both.
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
T = torch.from_numpy
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed_block(fn, inner):
    """(device-event microseconds, host-clock microseconds) per call of `inner` back-to-back calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    host = (time.perf_counter() - t0) * 1e6 / inner
    return start.elapsed_time(end) * 1e3 / inner, host


def ab(name, fa, fb, rounds, inner, warm=3):
    for _ in range(warm):
        fa()
        fb()
    res = {'a_dev': [], 'a_host': [], 'b_dev': [], 'b_host': []}
    for _ in range(rounds):
        for key, f in (('a', fa), ('b', fb)):
            d, h = timed_block(f, inner)
            res[key + '_dev'].append(d)
            res[key + '_host'].append(h)
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = {k: (min(v), max(v)) for k, v in res.items()}
    say('  %-38s composition %9.1f us (host %9.1f, range %.1f-%.1f)   fused %9.1f us (host %9.1f, range %.1f-%.1f)   ratio %5.3fx' %
        (name, med['a_dev'], med['a_host'], *spread['a_dev'], med['b_dev'], med['b_host'], *spread['b_dev'],
         med['a_dev'] / med['b_dev']))
    return dict(name=name, median_us=med, min_max_us=spread, ratio_device=med['a_dev'] / med['b_dev'],
                ratio_host=med['a_host'] / med['b_host'])


def count_launches(fn):
    """Device operations (kernels, memsets, copies) one call enqueues, by torch.profiler; None when it gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return n / 4.0 if n else None
    except Exception as exc:     # the count is an extra; the timings stand without it
        say('  (launch count unavailable: %s)' % (exc,))
        return None


def peak_bytes(fn):
    """Peak allocated memory during one call above what is allocated before it."""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def extras(r, fa, fb):
    r['launches_composition'], r['launches_fused'] = count_launches(fa), count_launches(fb)
    r['peak_bytes_composition'], r['peak_bytes_fused'] = peak_bytes(fa), peak_bytes(fb)
    say('    device operations per call %s -> %s;  peak allocated above the resident set %.1f -> %.1f MB' %
        (r['launches_composition'], r['launches_fused'], r['peak_bytes_composition'] / 1e6, r['peak_bytes_fused'] / 1e6))
    return r


def micro(args):
    from mmnas_amd import ops
    B, S, F = args.batch, args.regions, args.width
    g = torch.Generator().manual_seed(5)
    r = lambda *sh: torch.randn(*sh, generator=g).to(DEV)
    p = dict(yf=r(B, S, F), xp=r(B, F), a=1 + 0.1 * r(F), b=0.1 * r(F), ws=r(1, F) * F ** -0.5, bs=0.1 * r(1), wr=r(4, F) * F ** -0.5,
             br=0.1 * r(4))
    for v in p.values():
        v.requires_grad_()
    gs, gr = r(B, S), r(B, S, 4)

    def composition():      # the VGD branch of nets._Net.forward with the switch off
        xy = ops.layer_norm(p['xp'].unsqueeze(1) + p['yf'], p['a'], p['b'], 1e-6)
        scores = torch.nn.functional.log_softmax(ops.linear(xy, p['ws'], p['bs']).squeeze(-1), dim=-1)
        return scores, ops.linear(xy, p['wr'], p['br'])

    def fused():
        return ops.grounding_head(p['yf'], p['xp'], p['a'], p['b'], 1e-6, p['ws'], p['bs'], p['wr'], p['br'], log_softmax=True)

    def run(head):
        for v in p.values():
            v.grad = None
        scores, reg = head()
        torch.autograd.backward([scores, reg], [gs, gr])

    fa, fb = (lambda: run(composition)), (lambda: run(fused))
    # agreement first
    fa()
    ga = {k: v.grad.clone() for k, v in p.items()}
    oa = [t.detach().clone() for t in composition()]
    fb()
    ob = [t.detach() for t in fused()]
    worst = max(float((x - y).abs().max() / x.abs().max()) for x, y in zip(oa, ob))
    # (proj_scores.bias: its gradient is a sum that vanishes under log_softmax, round-off on both sides)
    worst_g = max(float((ga[k] - v.grad).abs().max() / ga[k].abs().max()) for k, v in p.items() if k != 'bs')
    assert worst <= 1e-4 and worst_g <= 1e-3, (worst, worst_g)
    say('head alone, forward + backward, B=%d S=%d F=%d (median of %d alternating rounds of %d calls; outputs agree to %.1e, '
        'gradients to %.1e):' % (B, S, F, args.rounds, args.inner, worst, worst_g))
    return [extras(ab('grounding head fwd + bwd', fa, fb, args.rounds, args.inner), fa, fb)]


def step(args):
    from mmnas.model.full_vgd import Net_Full
    from mmnas_amd import losses as FL
    from mmnas_amd import ops
    from mmnas_amd.harness import TrainLoop
    from tests.golden import cases
    c = cases.losses_cases(True)[2]
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Full(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    net = net.to(DEV).train()
    t = {k: T(v).to(DEV) for k, v in cases.vgd_targets(c, 9204).items()}
    inputs = tuple(T(a).to(DEV) for a in c['inputs'])
    loop = TrainLoop(net, loss_fn=FL.VgdLoss(c['cfg']), lr=1e-5)

    def run(on):
        prev = ops.set_vgd_head(on)
        try:
            return loop.step(inputs, t)
        finally:
            ops.set_vgd_head(prev)

    fa, fb = (lambda: run(False)), (lambda: run(True))
    say('whole TrainLoop VGD step, B=%d, HSIZE %d, %d regions, switch off / on (median of %d alternating rounds of %d steps):' %
        (inputs[0].shape[0], c['cfg'].HSIZE, inputs[0].shape[1], args.step_rounds, args.step_inner))
    return [extras(ab('train_vgd TrainLoop step', fa, fb, args.step_rounds, args.step_inner), fa, fb)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--regions', type=int, default=100)
    ap.add_argument('--width', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--step-rounds', type=int, default=7)
    ap.add_argument('--step-inner', type=int, default=10)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('vgd_head_ab.py measures on the GPU; no device is visible')
    say('vgd_head_ab: %s, HIP_FORCE_DEV_KERNARG=%s (%s)' % (torch.cuda.get_device_name(0), _lib.KERNARG_VALUE, _lib.KERNARG_SOURCE))
    rec = dict(tool='vgd_head_ab', device=torch.cuda.get_device_name(0), B=args.batch, S=args.regions, F=args.width,
               rounds=args.rounds, inner=args.inner, micro=micro(args))
    if not args.no_step:
        rec.update(step_rounds=args.step_rounds, step_inner=args.step_inner, steps=step(args))
    say(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
