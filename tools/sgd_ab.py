"""A/B of the weight-optimizer step at the search_vqa supernet's parameter set (the benchmark's Net_Search: every parameter
but the alphas; the tensor and parameter counts are printed), all gradients present, clip 1.0:

  torch   clip_grad_norm_ + torch.optim.SGD(momentum 0.9, weight_decay 1e-4).step() over the separate tensors (`foreach` left
          at its default) -- what NET_OPTIM = 'sgd' costs on the unfused path;
  sgd     optim.FlatSGD.step(max_norm): one sum-of-squares launch + one mmnas_sgd_step launch over the flat buffers;
  adam    optim.FlatAdam.step(max_norm), for scale.

Each side runs --inner steps back to back between two device events; the sides alternate, --rounds each; medians of the
device-event time and of the host clock around the same block (closed by a synchronise) are reported, and the launches per
step counted with torch.profiler in a pass of their own.

  python tools/sgd_ab.py [--rounds 9 --inner 20 --out profiles/r08_sgd_ab.txt]
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


def supernet_shapes():
    import numpy as np
    import bench
    from mmnas.model.hygr_vqa import Net_Search
    init = {'token_size': bench.VOCAB, 'ans_size': bench.ANS, 'pretrained_emb': np.zeros((bench.VOCAB, 300), np.float32)}
    net = Net_Search(bench.make_cfg('search'), init)          # on the host: only the shapes are wanted
    return [tuple(p.shape) for k, p in net.named_parameters() if 'alpha' not in k]


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


def count_launches(fn):
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
        print('  (launch count unavailable: %s)' % (exc,))
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join('profiles', 'r08_sgd_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('sgd_ab.py measures on the GPU; no device is visible')
    from mmnas_amd.optim import FlatAdam, FlatSGD
    shapes = supernet_shapes()
    g = torch.Generator().manual_seed(3)
    init = [0.05 * torch.randn(s, generator=g) for s in shapes]
    grads = [0.01 * torch.randn(s, generator=g) for s in shapes]
    n_total = sum(t.numel() for t in init)
    lr, mom, wd, clip = 0.005, 0.9, 1e-4, 1.0

    def params():
        return [torch.nn.Parameter(t.clone().to(DEV)) for t in init]

    pa = params()
    for p, gr in zip(pa, grads):
        p.grad = gr.to(DEV)
    topt = torch.optim.SGD(pa, lr, momentum=mom, weight_decay=wd)
    keep = [p.grad.clone() for p in pa]

    def f_torch():
        torch._foreach_copy_([p.grad for p in pa], keep)     # clip_grad_norm_ scales the gradients in place: restore (not part of a real step)
        torch.nn.utils.clip_grad_norm_(pa, clip)
        topt.step()

    def f_torch_restore_only():
        torch._foreach_copy_([p.grad for p in pa], keep)

    flat = {}
    for name, opt in (('sgd', FlatSGD(params(), lr=lr, momentum=mom, weight_decay=wd)), ('adam', FlatAdam(params(), lr=lr))):
        opt.zero_grad()
        for p, gr in zip(opt.params, grads):
            p.grad.copy_(gr.to(DEV))
        flat[name] = opt
    sides = [('torch', f_torch), ('torch_restore', f_torch_restore_only), ('sgd', lambda: flat['sgd'].step(max_norm=clip)),
             ('adam', lambda: flat['adam'].step(max_norm=clip))]
    # agreement first: one step on both SGD sides from the same state
    f_torch()
    flat['sgd'].step(max_norm=clip)
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(pa, flat['sgd'].params))
    assert worst < 1e-6, worst
    for _ in range(3):
        for _, f in sides:
            f()
    res = {k: {'dev': [], 'host': []} for k, _ in sides}
    for _ in range(args.rounds):
        for k, f in sides:
            d, h = timed_block(f, args.inner)
            res[k]['dev'].append(d)
            res[k]['host'].append(h)
    med = {k: {w: statistics.median(v[w]) for w in v} for k, v in res.items()}
    rng = {k: {w: (min(v[w]), max(v[w])) for w in v} for k, v in res.items()}
    launches = {k: count_launches(f) for k, f in sides}
    lines = ['weight-optimizer step, %d tensors / %d parameters, clip %.1f, %s; median of %d alternating rounds of %d steps'
             % (len(shapes), n_total, clip, torch.cuda.get_device_name(0), args.rounds, args.inner),
             '  %-44s %12s %12s %10s' % ('side', 'device us', 'host us', 'launches')]
    label = {'torch': 'clip_grad_norm_ + torch SGD (+ grad restore)', 'torch_restore': '  of which: the grad restore alone',
             'sgd': 'FlatSGD.step(max_norm)', 'adam': 'FlatAdam.step(max_norm)'}
    for k, _ in sides:
        lines.append('  %-44s %12.1f %12.1f %10s   (device min..max %.1f..%.1f)' % (label[k], med[k]['dev'], med[k]['host'], launches[k],
                                                                                    rng[k]['dev'][0], rng[k]['dev'][1]))
    net = {w: med['torch'][w] - med['torch_restore'][w] for w in ('dev', 'host')}
    lines.append('  torch side net of the restore: device %.1f us, host %.1f us; FlatSGD is %.2fx (device) / %.2fx (host) of that'
                 % (net['dev'], net['host'], net['dev'] / med['sgd']['dev'], net['host'] / med['sgd']['host']))
    lines.append('  streaming floor of the SGD update at 5 TB/s (20 B per parameter + 4 B for the norm): %.1f us' % (n_total * 24 / 5e12 * 1e6))
    lines.append(json.dumps(dict(tool='sgd_ab', tensors=len(shapes), parameters=n_total, rounds=args.rounds, inner=args.inner,
                                 median_us=med, min_max_us=rng, launches=launches, max_abs_diff_after_one_step=worst)))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
