"""Which GEMM kernel runs for which call: a fixed list of single calls, each the smallest shape that selects its kernel, under every
knob setting that selects kernels (tests/gemm_knobs.py's mechanism: the environment + mmnas_gemm_reload_tuning).  Seconds.

    rocprofv3 --kernel-trace --output-format csv -d /tmp/tr -o t -- python3 tools/gemm_dispatch_sweep.py      # run the calls
    python3 tools/gemm_dispatch_sweep.py --reduce /tmp/tr > profiles/<name>.txt        # (kernel, workgroups, threads) per dispatch

Run it once per library (MMNAS_LIB_PATH selects one) and diff the two reduced sequences: a change of the dispatch code that is
meant to launch the same kernels must leave them identical, row for row.  The run itself prints one line per call with a checksum
of its outputs (products added by float atomics may move in the last digits)."""
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SETTINGS = [{}] + [{k: v} for k, vs in (('SPLIT', (0, 1, 3, 6)), ('PF', (1,)), ('TILE', (64, 128)), ('LEAN', (0, 1, 2, 3)),
                                        ('PAIR', (0, 1, 3)), ('GENERIC', (1,)), ('SK', (0, 2))) for v in vs]
SETTINGS += [{'SPLIT': 0, 'PF': 1}] + [{'TILE': 128, 'SPLIT': v} for v in (0, 1, 3)]   # (kernels only two knobs together select)


def reduce_trace(root):
    kf = sorted(glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True))[0]
    rows = sorted(csv.DictReader(open(kf)), key=lambda r: int(r['Start_Timestamp']))
    for r in rows:
        if 'mmnas::' in r['Kernel_Name']:
            wg = int(r['Workgroup_Size_X'])
            print('%s\t%d\t%d' % (r['Kernel_Name'].split('(')[0], int(r['Grid_Size_X']) // max(wg, 1), wg))


def main():
    import numpy as np
    import torch
    from mmnas_amd import ops, _lib as L
    lib = L.lib()
    dev = 'cuda'
    rs = np.random.RandomState(7)
    g = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rnd = lambda *s: rs.standard_normal(s).astype(np.float32)
    NT, NN, TN = L.GEMM_NT, L.GEMM_NN, L.GEMM_TN

    def single(layout, M, N, K, colsum=False, planes=False, accumulate=False, ktab=None, a=None):
        ash, bsh = {NT: ((M, K), (N, K)), NN: ((M, K), (K, N)), TN: ((K, M), (K, N))}[layout]
        A, B = g(rnd(*ash)) if a is None else a, g(rnd(*bsh))
        Cm = g(rnd(M, N)) if accumulate else torch.empty(M, N, device=dev)
        grp = dict(M=M, A=[A], B=[ops.split_planes(B) if planes else B], C=Cm)
        if colsum:
            grp['colsum'] = torch.zeros(N, device=dev)
        d = ops.gemm_desc(layout, [grp], N, K, ash[1], bsh[1], N, accumulate=accumulate, b_planes=planes)
        if ktab is not None:
            d.ktab = L.ptr(ktab)
        L.check(lib.mmnas_gemm(C.byref(d), L.stream()))
        return [Cm] + ([grp['colsum']] if colsum else [])

    def live_table(rows, d):
        """dy [rows, d], zero outside the first 1, 31, 32, ... rows of each block of 100, and its live-row table"""
        mask = (np.arange(100)[None, :] >= np.resize((1, 31, 32, 33, 96, 100), rows // 100)[:, None]).reshape(-1)
        dy = rnd(rows, d)
        dy[mask] = 0
        dyd, md = g(dy), g(mask.astype(np.uint8))
        tab = torch.zeros(lib.mmnas_wgrad_live_table_ints(rows), dtype=torch.int32, device=dev)
        L.check(lib.mmnas_wgrad_live_table(L.fptr(dyd), L.ptr(md), rows, d, L.ptr(tab), L.stream()))
        return dyd, tab

    def pair(M, nin, nout, colsum=False, live=False):
        dy, tab = live_table(M, nout) if live else (g(rnd(M, nout)), None)
        x, W = g(rnd(M, nin)), g(rnd(nout, nin))
        dx, dW = torch.empty(M, nin, device=dev), torch.zeros(nout, nin, device=dev)
        grp = dict(M=M, A=[dy], B=[W], C=dx)
        if colsum:
            grp['colsum'] = torch.zeros(nin, device=dev)
        dg = ops.gemm_desc(NN, [grp], nin, nout, nout, nin, nin)
        wg = ops.gemm_desc(TN, [dict(M=nout, A=[dy], B=[x], C=dW)], nin, M, nout, nin, nin, accumulate=True)
        if live:
            wg.ktab = L.ptr(tab)
        ops.gemm_pair(dg, wg)
        return [dx, dW] + ([grp['colsum']] if colsum else [])

    def pair3(M, nin, nout):   # a three-segment data gradient next to three grouped weight gradients (SelfAtt's q, k, v)
        dy, W, x = [g(rnd(M, nout)) for _ in range(3)], [g(rnd(nout, nin)) for _ in range(3)], g(rnd(M, nin))
        dx, dW = torch.empty(M, nin, device=dev), [torch.zeros(nout, nin, device=dev) for _ in range(3)]
        dg = ops.gemm_desc(NN, [dict(M=M, A=dy, B=W, C=dx)], nin, nout, nout, nin, nin, nseg=3)
        wg = ops.gemm_desc(TN, [dict(M=nout, A=[a], B=[x], C=c) for a, c in zip(dy, dW)], nin, M, nout, nin, nin, accumulate=True)
        ops.gemm_pair(dg, wg)
        return [dx] + dW

    def tn_live():
        dy, tab = live_table(600, 1024)
        return single(TN, 1024, 256, 600, accumulate=True, ktab=tab, a=dy)

    def mlp():   # two layers + LayerNorm: the backward's first pair launch carries the LayerNorm parameter reduction
        d = 256
        p = [g(a).requires_grad_() for a in (rnd(2, 8, d), rnd(4 * d, d) * 0.05, rnd(d, 4 * d) * 0.05, rnd(4 * d), rnd(d), rnd(d), rnd(d))]
        y = ops.mlp_op(p[0], p[1:3], p[3:5], p[5], p[6], norm=True, residual=True, drop_p=0.0, training=True)
        y.backward(g(rnd(2, 8, d)))
        return [y.detach()] + [t.grad for t in p]

    def short_self_att():   # short-sequence SelfAtt: its one-launch backward leaves a weight gradient and no data gradient to pair with
        d = 256
        prev = lib.mmnas_set_small_ops(1), lib.mmnas_set_small_bwd(1)
        try:
            p = [g(a).requires_grad_() for a in [rnd(4, 14, d)] + [rnd(d, d) * 0.05 for _ in range(4)] + [rnd(d), rnd(d)]]
            y = ops.attention_op(p[0], None, None, None, p[1], p[2], p[3], p[4], None, None, p[5], p[6], dh=64, norm=True, residual=True,
                                 drop_p=0.0, training=True)
            y.backward(g(rnd(4, 14, d)))
        finally:
            lib.mmnas_set_small_ops(prev[0])
            lib.mmnas_set_small_bwd(prev[1])
        return [y.detach()] + [t.grad for t in p]

    def lstm_steps():   # the per-step LSTM entry points at T = 2
        T, B, E, H = 2, 4, 32, 32
        z = lambda *s: torch.zeros(*s, device=dev)
        x, Wih, Whh, bias = g(rnd(T, B, E)), g(rnd(4 * H, E) * 0.1), g(rnd(4 * H, H) * 0.1), g(rnd(4 * H))
        xp, Hall, Call, Gall, out = z(T, B, 4 * H), z(T + 1, B, H), z(T + 1, B, H), z(T, B, 4 * H), z(B, T, H)
        L.check(lib.mmnas_lstm_fwd(*[L.fptr(t) for t in (x, Wih, Whh, bias, xp, Hall, Call, Gall, out)], T, B, E, H, L.stream()))
        DG, dc, scratch = z(T + 1, B, 4 * H), z(B, H), z(B, H)
        L.check(lib.mmnas_lstm_bwd(*[L.fptr(t) for t in (g(rnd(B, T, H)), Whh, Call, Gall, DG, dc, scratch)], T, B, H, L.stream()))
        return [out, Call, DG, dc]

    calls = [('%s whole tiles' % n, lambda l=l: single(l, 128, 128, 64)) for n, l in (('NT', NT), ('NN', NN), ('TN', TN))]
    calls += [('%s three column tiles' % n, lambda l=l: single(l, 128, 192, 64)) for n, l in (('NT', NT), ('NN', NN))]
    calls += [
        ('NT hybrid 272 tiles', lambda: single(NT, 1088, 1024, 512)), ('NN hybrid 270 tiles', lambda: single(NN, 1152, 960, 512)),
        ('NT stream-K 14 tiles', lambda: single(NT, 128, 448, 512)), ('NN stream-K 16 tiles', lambda: single(NN, 128, 512, 512)),
        ('TN split-K 4 tiles', lambda: single(TN, 128, 128, 1024, accumulate=True)),
        ('TN split-K 1 tile', lambda: single(TN, 64, 64, 1024, accumulate=True)),
        ('NN column sums', lambda: single(NN, 128, 128, 64, colsum=True)), ('NT b_planes', lambda: single(NT, 128, 128, 64, planes=True)),
        ('TN live-row table', tn_live), ('NN odd shape', lambda: single(NN, 70, 37, 50)), ('NT odd shape', lambda: single(NT, 70, 37, 50)),
        ('TN odd shape', lambda: single(TN, 70, 37, 50)),
        ('pair dgrad three column tiles', lambda: pair(600, 192, 128)), ('pair whole tiles', lambda: pair(600, 128, 128)),
        ('pair one wgrad tile', lambda: pair(128, 64, 64)), ('pair dgrad stream-K', lambda: pair(128, 512, 512)),
        ('pair dgrad stream-K, wgrad split-K', lambda: pair(600, 512, 512)),
        ('pair dgrad too large to be lean', lambda: pair3(1152, 512, 1408)),
        ('pair dgrad column sums', lambda: pair(600, 128, 128, colsum=True)), ('pair live three column tiles', lambda: pair(600, 192, 128, live=True)),
        ('pair live whole tiles', lambda: pair(600, 128, 128, live=True)), ('pair live dgrad stream-K', lambda: pair(600, 512, 512, live=True)),
        ('pair live dgrad column sums', lambda: pair(600, 128, 128, colsum=True, live=True)),
        ('mlp_op fwd + bwd with LayerNorm', mlp), ('short SelfAtt fwd + bwd', short_self_att), ('lstm steps T=2', lstm_steps)]

    for knobs in SETTINGS:
        for k, v in knobs.items():
            os.environ['MMNAS_GEMM_' + k] = str(v)
        lib.mmnas_gemm_reload_tuning()
        for name, fn in calls:
            try:
                outs = fn()
                torch.cuda.synchronize()
                res = ' '.join('%.6e' % float(t.double().abs().sum()) for t in outs if t is not None)
            except L.MMNasHipError as e:
                res = 'refused: %s' % e
            print('%-18s %-34s %s' % (' '.join('%s=%s' % kv for kv in knobs.items()) or 'defaults', name, res), flush=True)
        for k in knobs:
            os.environ.pop('MMNAS_GEMM_' + k, None)
    lib.mmnas_gemm_reload_tuning()


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == '--reduce':
        reduce_trace(sys.argv[2])
    else:
        main()
