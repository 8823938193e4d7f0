"""A/B of the grounding and retrieval training losses: the torch composition (harness.vgd_loss, BCE_Loss, Margin_Loss) against
the HIP form (mmnas_amd.losses), forward + backward, random inputs.

  micro  VGD at B = 64 x 100 regions in both score modes and both mask layouts (row: scores_mask [B,1] + bbox_mask [B,S,1],
         what grounding_targets returns; full: [B,S] + [B,S,4], the loader's), ITM at B = 160 for BCE_Loss and Margin_Loss.
         Each side runs --inner forward + backward calls back to back between two device events; A and B alternate, --rounds
         each; the median microseconds per call (device events, and the host clock around the same block closed by a
         synchronise) and the ratio are printed.  Kernel launches per call are counted with torch.profiler in a pass of its own.
  step   one whole TrainLoop step of the VGD Net_Full at the train_vgd dimensions (HSIZE 512, B = 64, 100 regions) and one
         whole itm_triplet_step of the ITM Net_Full (B = 160), each with the torch composition and with the fused loss,
         alternating on one device.

  python tools/loss_ab.py [--rounds 9 --inner 50 --step-rounds 7 --step-inner 10 --no-step --out FILE]

Prints the table, then one JSON line (also written to --out).
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


def vgd_inputs(B, S, layout, seed=5):
    rs = np.random.RandomState(seed)
    ps = torch.log_softmax(T(rs.standard_normal((B, S)).astype(np.float32)), -1)
    pr = T((1.5 * rs.standard_normal((B, S, 4))).astype(np.float32))
    sc = rs.dirichlet(np.ones(S), B).astype(np.float32)
    sc[rs.uniform(size=(B, S)) < 0.5] = 0
    bb = rs.standard_normal((B, S, 4)).astype(np.float32)
    sm = (rs.uniform(size=(B, 1) if layout == 'row' else (B, S)) < 0.8).astype(np.float32)
    bm = (rs.uniform(size=(B, S, 1)) < 0.2).astype(np.float32)
    if layout == 'full':
        bm = bm * np.ones((1, 1, 4), np.float32)
    return [t.to(DEV) for t in (ps, pr, T(sc), T(sm), T(bb), T(bm))]


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
    print('  %-34s torch %8.1f us (host %8.1f)   fused %7.1f us (host %7.1f)   ratio %5.2fx' %
          (name, med['a_dev'], med['a_host'], med['b_dev'], med['b_host'], med['a_dev'] / med['b_dev']))
    return dict(name=name, median_us=med, min_max_us=spread, ratio_device=med['a_dev'] / med['b_dev'],
                ratio_host=med['a_host'] / med['b_host'])


def count_launches(fn):
    """Device kernels (and memsets / copies) one call enqueues, by torch.profiler; None when the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
        n = 0
        for e in prof.events():
            if str(getattr(e, 'device_type', '')).endswith('CUDA'):
                n += 1
        return n / 4.0 if n else None
    except Exception as exc:     # the count is an extra; the timings stand without it
        print('  (launch count unavailable: %s)' % (exc,))
        return None


def micro(args):
    from mmnas_amd import losses as FL
    from mmnas_amd.harness import BCE_Loss, vgd_loss
    from mmnas_amd.utils.itm_loss import Margin_Loss
    out = []
    B, S = args.batch, args.regions
    print('VGD loss forward + backward, B=%d S=%d; ITM triplet losses, B=%d (median of %d alternating rounds of %d calls):' %
          (B, S, args.itm_batch, args.rounds, args.inner))
    for mode in ('kld', 'bce'):
        for layout in ('row', 'full'):
            arrs = vgd_inputs(B, S, layout)
            ps, pr = arrs[0].requires_grad_(), arrs[1].requires_grad_()

            def fa(ps=ps, pr=pr, arrs=arrs, mode=mode):
                ps.grad = pr.grad = None
                vgd_loss(ps, pr, *arrs[2:], scores_loss=mode).backward()

            def fb(ps=ps, pr=pr, arrs=arrs, mode=mode):
                ps.grad = pr.grad = None
                FL.vgd_loss_fused(ps, pr, *arrs[2:], scores_loss=mode).backward()

            # agreement first
            fa()
            la, ga = float(vgd_loss(ps, pr, *arrs[2:], scores_loss=mode).detach()), (ps.grad.clone(), pr.grad.clone())
            fb()
            lb = float(FL.vgd_loss_fused(ps, pr, *arrs[2:], scores_loss=mode).detach())
            assert abs(la - lb) <= 1e-4 * abs(la), (la, lb)
            assert torch.allclose(ga[0], ps.grad, rtol=1e-4, atol=1e-7) and torch.allclose(ga[1], pr.grad, rtol=1e-4, atol=1e-7)
            r = ab('vgd %s masks=%s' % (mode, layout), fa, fb, args.rounds, args.inner)
            r['launches_torch'], r['launches_fused'] = count_launches(fa), count_launches(fb)
            out.append(r)
    rs = np.random.RandomState(6)
    s = [T(rs.uniform(0.01, 0.99, args.itm_batch).astype(np.float32)).to(DEV).requires_grad_() for _ in range(3)]
    for name, ref in (('itm BCE_Loss', BCE_Loss()), ('itm Margin_Loss', Margin_Loss())):
        mine = FL.fused(ref)

        def fa(ref=ref):
            for t in s:
                t.grad = None
            ref(*s).backward()

        def fb(mine=mine):
            for t in s:
                t.grad = None
            mine(*s).backward()

        fa()
        ga = [t.grad.clone() for t in s]
        fb()
        la, lb = float(ref(*s).detach()), float(mine(*s).detach())
        assert abs(la - lb) <= 1e-4 * abs(la), (la, lb)
        assert all(torch.allclose(a, t.grad, rtol=1e-4, atol=1e-7) for a, t in zip(ga, s))
        r = ab(name, fa, fb, args.rounds, args.inner)
        r['launches_torch'], r['launches_fused'] = count_launches(fa), count_launches(fb)
        out.append(r)
    print('  kernel launches per call (torch / fused): ' +
          ', '.join('%s %s / %s' % (r['name'], r['launches_torch'], r['launches_fused']) for r in out))
    return out


def _build(cls, c):
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = cls(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    return net.to(DEV).train()


def steps(args):
    from mmnas.model.full_itm import Net_Full as ItmNet
    from mmnas.model.full_vgd import Net_Full as VgdNet
    from mmnas_amd import losses as FL
    from mmnas_amd.harness import BCE_Loss, TrainLoop, itm_triplet_step, vgd_loss
    from tests.golden import cases
    out = []
    c_pos, c_neg, c_vgd = cases.losses_cases(True)
    print('whole steps (median of %d alternating rounds of %d steps):' % (args.step_rounds, args.step_inner))
    # VGD: TrainLoop step (forward, loss, backward, clip, Adam) at the train_vgd dimensions
    t = {k: T(v).to(DEV) for k, v in cases.vgd_targets(c_vgd, 9204).items()}
    t['scores_mask'] = t['scores_mask'][:, :1].contiguous()           # the layouts grounding_targets returns
    t['bbox_mask'] = t['bbox_mask'][:, :, :1].contiguous()
    inputs = tuple(T(a).to(DEV) for a in c_vgd['inputs'])
    loops = [TrainLoop(_build(VgdNet, c_vgd), loss_fn=fn, lr=1e-5) for fn in (
        lambda pred, tg: vgd_loss(pred[0], pred[1], tg['scores'], tg['scores_mask'], tg['bbox'], tg['bbox_mask']), FL.VgdLoss())]
    out.append(ab('train_vgd TrainLoop step B=%d' % inputs[0].shape[0], lambda: loops[0].step(inputs, t), lambda: loops[1].step(inputs, t),
                  args.step_rounds, args.step_inner))
    del loops
    # ITM: itm_triplet_step (three forwards, loss, one backward) at the train_itm dimensions
    net = _build(ItmNet, c_pos)
    pos = tuple(T(a).to(DEV) for a in c_pos['inputs'])
    neg = tuple(T(a).to(DEV) for a in c_neg['inputs'])
    fns = (BCE_Loss(), FL.fused(BCE_Loss()))

    def step(fn):
        net.zero_grad(set_to_none=True)
        itm_triplet_step(net, fn, pos, neg)

    out.append(ab('train_itm itm_triplet_step B=%d' % pos[0].shape[0], lambda: step(fns[0]), lambda: step(fns[1]), args.step_rounds,
                  args.step_inner))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--regions', type=int, default=100)
    ap.add_argument('--itm-batch', type=int, default=160)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--step-rounds', type=int, default=7)
    ap.add_argument('--step-inner', type=int, default=10)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('loss_ab.py measures on the GPU; no device is visible')
    rec = dict(tool='loss_ab', device=torch.cuda.get_device_name(0), B=args.batch, S=args.regions, itm_B=args.itm_batch,
               rounds=args.rounds, inner=args.inner, micro=micro(args))
    if not args.no_step:
        rec.update(step_rounds=args.step_rounds, step_inner=args.step_inner, steps=steps(args))
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
