"""Tuning aid: times mmnas_mha_core_fwd / _bwd alone (HIP events around 50 launches, medians over alternating rounds).

    python tools/mha_bench.py                                   # the workloads' attention shapes
    python tools/mha_bench.py --shapes 64,4,256,256,64,0 64,4,512,512,64,1 --stream-mink 257 1

--shapes B,H,Sq,Sk,dh,bias ...   the problems (bias: 0 / 1, the key-major relation bias)
--stream-mink N ...              settings of MMNAS_MHA_STREAM_MINK (the fewest keys at which the forward streams the keys); with
                                 several, every round times each setting in turn, so that clock drift lands on all of them
--rounds R                       rounds (default 9); the median per setting is printed, with the time per score element B H Sq Sk

MMNAS_MHA_BWD_FUSED selects the backward kernel of the short shapes.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mmnas_amd import _lib as L  # noqa: E402   (before the first CUDA call: the library sets its launch configuration at import)

import torch  # noqa: E402

DEFAULT_SHAPES = ['64,4,100,100,64,0', '64,4,100,100,64,1', '64,8,100,100,64,0', '64,8,100,100,64,1', '64,4,100,14,64,0',
                  '64,8,100,14,64,0', '64,4,14,14,64,0']
LAUNCHES = 50


def problem(B, H, Sq, Sk, dh, bias, dev='cuda'):
    di = H * dh
    t = dict(Q=torch.randn(B, Sq, di, device=dev), dO=torch.randn(B, Sq, di, device=dev), K=torch.randn(B, Sk, di, device=dev),
             V=torch.randn(B, Sk, di, device=dev), mask=torch.zeros(B, Sk, dtype=torch.uint8, device=dev),
             bT=torch.randn(B, H, Sk, Sq, device=dev) if bias else None, O=torch.empty(B, Sq, di, device=dev),
             stats=torch.empty(B, H, Sq, 2, device=dev), delta=torch.empty(B, H, Sq, device=dev))
    t.update(dQ=torch.empty_like(t['Q']), dK=torch.empty_like(t['K']), dV=torch.empty_like(t['V']),
             dbT=torch.empty(B, H, Sk, Sq, device=dev) if bias else None)
    d = L.MhaDesc()
    d.B, d.H, d.Sq, d.Sk, d.dh = B, H, Sq, Sk, dh
    d.ldq = d.ldk = d.ldv = d.ldo = di
    d.Q, d.K, d.V, d.mask, d.biasT, d.O, d.lse = (L.fptr(t['Q']), L.fptr(t['K']), L.fptr(t['V']), L.ptr(t['mask']), L.fptr(t['bT']),
                                                 L.fptr(t['O']), L.fptr(t['stats']))
    d.drop_p, d.drop_site, d.drop_seed = 0.1, 0, 1234
    d.dO, d.dQ, d.dK, d.dV, d.dbiasT, d.delta = (L.fptr(t['dO']), L.fptr(t['dQ']), L.fptr(t['dK']), L.fptr(t['dV']), L.fptr(t['dbT']),
                                                 L.fptr(t['delta']))
    return d, t


def timed(fn, d):
    """microseconds per launch: LAUNCHES launches between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(LAUNCHES):
        fn(C.byref(d), L.stream())
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / LAUNCHES


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', nargs='+', default=DEFAULT_SHAPES, metavar='B,H,Sq,Sk,dh,bias')
    ap.add_argument('--stream-mink', nargs='+', type=int, default=None, metavar='N')
    ap.add_argument('--rounds', type=int, default=9)
    a = ap.parse_args()
    lib = L.lib()
    settings = a.stream_mink if a.stream_mink else [None]
    prev = os.environ.get('MMNAS_MHA_STREAM_MINK')
    for spec in a.shapes:
        B, H, Sq, Sk, dh, bias = (int(v) for v in spec.split(','))
        d, keep = problem(B, H, Sq, Sk, dh, bool(bias))
        calls = (('fwd', lib.mmnas_mha_core_fwd), ('bwd', lib.mmnas_mha_core_bwd))
        times = {(s, name): [] for s in settings for name, _ in calls}
        for rnd in range(-1, a.rounds):          # round -1: warm-up, not recorded
            for s in settings:
                if s is not None:
                    os.environ['MMNAS_MHA_STREAM_MINK'] = str(s)      # read at every call
                for name, fn in calls:
                    L.check(fn(C.byref(d), L.stream()))
                    us = timed(fn, d)
                    if rnd >= 0:
                        times[(s, name)].append(us)
        el = float(B) * H * Sq * Sk
        for s in settings:
            med = {name: statistics.median(times[(s, name)]) for name, _ in calls}
            print('B=%d H=%d Sq=%3d Sk=%3d dh=%d bias=%d%s | fwd %7.1f us (%.3f ps/element) | bwd %7.1f us (%.3f ps/element)'
                  % (B, H, Sq, Sk, dh, bias, '' if s is None else ' stream_mink=%3d' % s, med['fwd'], med['fwd'] * 1e6 / el,
                     med['bwd'], med['bwd'] * 1e6 / el), flush=True)
        del keep
    if prev is None:
        os.environ.pop('MMNAS_MHA_STREAM_MINK', None)
    else:
        os.environ['MMNAS_MHA_STREAM_MINK'] = prev


if __name__ == '__main__':
    main()
