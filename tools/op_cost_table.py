"""Measured cost table of the search spaces' candidates for the cost-aware architecture search (mmnas_amd.cost.CostTable,
harness.SearchLoop(cost_table=...)): every candidate of Used_OPS['enc'] / Used_OPS['dec'] alone, through the module API
(OpsAdapter().OPS[name](cfg, norm, residual)(x, y, x_mask, y_mask, rel)), at the search script's dimensions for the task
(HSIZE 256; tokens x regions: vqa 14 x 100, vgd 15 x 100, itm 50 x 36), one synthetic batch without padding resident on the
device.

Two figures per candidate, each between two device events after a warm-up, the candidates taking turns inside every round,
the median over --rounds reported (min..max kept in meta):
  fwd      forward in eval mode under no_grad, us per batch;
  fwd_bwd  forward + backward in train mode (dropout 0.1 as the scripts have it), us per batch.
The table itself takes fwd_bwd: a search step differentiates the sampled candidate.  `none` has no kernel on its path; whatever
the events see of it is host-issued elementwise work, reported as measured.

  python tools/op_cost_table.py --task vqa|vgd|itm [--batch 64 --rounds 9 --inner 10] --out profiles/r14_op_cost_<task>.json
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mmnas_amd import _lib  # noqa: E402,F401   (before the first CUDA call: the library sets its launch configuration at import)

DEV = 'cuda:0'
DIMS = {'vqa': (14, 100), 'vgd': (15, 100), 'itm': (50, 36)}      # (Sx tokens, Sy regions)


def timed_block(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(inner):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--task', choices=sorted(DIMS), required=True)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--inner', type=int, default=10, help='calls per timed block')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('op_cost_table.py measures on the GPU; no device is visible')
    import bench
    from mmnas_amd import ops
    from mmnas_amd.cost import CostTable, op_flops
    from mmnas_amd.utils.ops_adapter import OpsAdapter

    torch.manual_seed(1400)
    ops.manual_seed(1400)
    cfg = bench.make_cfg('search')
    Sx, Sy = DIMS[args.task]
    B, d = args.batch, cfg.HSIZE
    adapter = OpsAdapter()
    g = torch.Generator().manual_seed(14)
    stream = {}
    for kind, S, So in (('enc', Sx, Sy), ('dec', Sy, Sx)):
        stream[kind] = dict(x=torch.randn(B, S, d, generator=g).to(DEV), y=torch.randn(B, So, d, generator=g).to(DEV),
                            x_mask=torch.zeros(B, 1, 1, S, dtype=torch.bool, device=DEV),
                            y_mask=torch.zeros(B, 1, 1, So, dtype=torch.bool, device=DEV),
                            rel=torch.relu(torch.randn(B, S, S, cfg.REL_SIZE, generator=g)).to(DEV),
                            gout=torch.randn(B, S, d, generator=g).to(DEV))

    runs = []      # (kind, name, figure, fn)
    for kind in ('enc', 'dec'):
        s = stream[kind]
        for name in adapter.Used_OPS[kind]:
            op = adapter.OPS[name](cfg, norm=cfg.OPS_NORM, residual=cfg.OPS_RESIDUAL).to(DEV)
            x = s['x'].clone().requires_grad_(True)

            def fwd(op=op, s=s):
                op.eval()
                with torch.no_grad():
                    op(s['x'], s['y'], s['x_mask'], s['y_mask'], s['rel'])

            def fwd_bwd(op=op, s=s, x=x):
                op.train()
                out = op(x, s['y'], s['x_mask'], s['y_mask'], s['rel'])
                if out.requires_grad:
                    out.backward(s['gout'])
                x.grad = None
                for p in op.parameters():
                    p.grad = None

            runs.append((kind, name, 'fwd', fwd))
            runs.append((kind, name, 'fwd_bwd', fwd_bwd))

    for _, _, _, fn in runs:      # warm-up: workspaces, caches, clocks
        for _ in range(5):
            fn()
    seen = {(k, n, f): [] for k, n, f, _ in runs}
    for r in range(args.rounds):
        for kind, name, fig, fn in (runs if r % 2 == 0 else runs[::-1]):
            seen[(kind, name, fig)].append(timed_block(fn, args.inner))

    table = {'enc': {}, 'dec': {}}
    detail = {'enc': {}, 'dec': {}}
    for kind in ('enc', 'dec'):
        for name in adapter.Used_OPS[kind]:
            fb, fw = seen[(kind, name, 'fwd_bwd')], seen[(kind, name, 'fwd')]
            table[kind][name] = round(statistics.median(fb), 2)
            detail[kind][name] = dict(fwd_us=round(statistics.median(fw), 2), fwd_us_min_max=[round(min(fw), 2), round(max(fw), 2)],
                                      fwd_bwd_us=round(statistics.median(fb), 2),
                                      fwd_bwd_us_min_max=[round(min(fb), 2), round(max(fb), 2)],
                                      fwd_mflop_per_batch=B * op_flops(name, cfg, Sx, Sy, kind) / 1e6)
    config = ops.runtime_config()
    config['lib_path'] = os.path.relpath(config['lib_path'], os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    meta = dict(tool='op_cost_table', task=args.task, device=torch.cuda.get_device_name(0), batch=B, HSIZE=d, Sx=Sx, Sy=Sy,
                dropout=cfg.DROPOUT_R, norm=cfg.OPS_NORM, residual=cfg.OPS_RESIDUAL, rounds=args.rounds, inner=args.inner,
                figure='fwd_bwd_us: forward + backward in train mode, us per batch, median of alternating rounds between device events',
                candidates=detail, runtime_config=config)
    tab = CostTable(table['enc'], table['dec'], unit='us', meta=meta)
    for kind in ('enc', 'dec'):
        for name in adapter.Used_OPS[kind]:
            dt = detail[kind][name]
            print('%s %-18s fwd %9.2f us   fwd+bwd %9.2f us (%.2f..%.2f)' % (kind, name, dt['fwd_us'], dt['fwd_bwd_us'],
                                                                         *dt['fwd_bwd_us_min_max']))
    out = args.out or os.path.join('profiles', 'r14_op_cost_%s.json' % args.task)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    tab.to_json(out)
    print('wrote', out)


if __name__ == '__main__':
    main()
