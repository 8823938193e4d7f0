"""Every output of the entry points that share mmnas_amd/csrc/ln_rows.h, written as .npy for the library MMNAS_LIB_PATH selects:
two builds are compared array for array, bit for bit.  Inputs are the fixed ones of tests/ln_rows.py (all eight row classes plus
`interleaved`); the calls go through the drivers of tests/test_ln_rows_gpu.py.

    MMNAS_LIB_PATH=<build A> python tools/ln_bitdump.py dump DIR_A        (one process per library)
    MMNAS_LIB_PATH=<build B> python tools/ln_bitdump.py dump DIR_B
    python tools/ln_bitdump.py compare DIR_A DIR_B [DIR_A2]

`compare` prints one line per array: equal / DIFFERS.  With DIR_A2, a second dump of build A, an array that build A itself does
not reproduce (sums by floating-point atomics) is reported as `not reproducible` and left out of the verdict.  Exit status 1 when
a reproducible array differs or an array is missing on one side.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(out):
    import torch
    from oracle import dropout_rng  # noqa: F401  (imported by the test module)
    from mmnas_amd import _lib as L, ops
    from tests import ln_rows as LR, test_ln_rows_gpu as G

    os.makedirs(out, exist_ok=True)
    lib = L.lib()

    def save(prefix, res):
        for k, v in res.items():
            np.save(os.path.join(out, '%s.%s.npy' % (prefix, k)), np.asarray(v))

    def inputs(M, d):
        yield from ((cls, LR.rows(cls, M, d)) for cls in LR.CLASSES)
        yield 'interleaved', LR.interleaved(M, d)[0]

    # mmnas_layernorm_fwd / _bwd
    for M, d in [(5, d) for d in (4, 36, 256, 260, 512, 516, 1024, 1028, 2048)] + [(2053, 36)]:
        a, b = LR.params(d)
        gy = LR.grad_out(M, d)
        for cls, x in inputs(M, d):
            for use_ws in (False, True):
                for drop in (False, True):
                    save('ln.M%d.d%d.%s.%s.%s' % (M, d, cls, 'scratch' if use_ws else 'atomics', 'drop' if drop else 'plain'),
                         G._ln_direct(x, a, b, gy, use_ws, drop))
    # mmnas_node_mix_fwd / _bwd
    for d in (36, 256, 512, 1024):
        M = 6
        rs = np.random.RandomState(d)
        z0 = (1.5 * rs.standard_normal((M, d)) + 0.3).astype(np.float32)
        gate = rs.standard_normal(3).astype(np.float32)
        a, b = LR.params(d)
        for cls, x in inputs(M, d):
            save('node_mix.d%d.%s' % (d, cls), G._node_mix(x, z0, a, b, gate, LR.grad_out(M, d, 1)))
    # mmnas_node_mix_bwd_ln
    for M, d in ((6, 36), (6, 256), (2053, 36)):
        rs = np.random.RandomState(d + 1)
        z0 = (1.5 * rs.standard_normal((M, d)) + 0.3).astype(np.float32)
        gate = rs.standard_normal(3).astype(np.float32)
        a, b = LR.params(d)
        for cls, x in inputs(M, d):
            for drop in (False, True):
                save('node_mix_ln.M%d.d%d.%s.%s' % (M, d, cls, 'drop' if drop else 'plain'),
                     G._node_mix_fused(x, z0, a, b, gate, LR.grad_out(M, d, 2), drop))
    # the short self-attention, forward + backward
    prev = lib.mmnas_set_small_ops(1), lib.mmnas_set_small_bwd(1), lib.mmnas_set_small_ffn(1)
    try:
        for cls in LR.CLASSES + ('interleaved',):
            case = G._short_self_att_case('randn' if cls == 'interleaved' else cls)
            if cls == 'interleaved':
                case['x'] = LR.interleaved(42, 256)[0].reshape(3, 14, 256)
            got, launches = G._run_counted(lib, case)
            assert launches == 2, launches
            save('small_self_att.%s' % cls, {k.replace('/', '_'): G.host(v) if torch.is_tensor(v) else v for k, v in got.items()})
    finally:
        lib.mmnas_set_small_ops(prev[0]), lib.mmnas_set_small_bwd(prev[1]), lib.mmnas_set_small_ffn(prev[2])
    # the grounding head
    prev = ops.set_vgd_head(True)
    try:
        for F, logsm in ((8, True), (256, False), (512, True), (1024, False), (2048, True)):
            for cls, x in inputs(G.VGD_B * G.VGD_S, F):
                save('vgd_head.F%d.%s' % (F, cls), G._grounding_head_run(F, logsm, x.reshape(G.VGD_B, G.VGD_S, F), G.g, ops.grounding_head))
    finally:
        ops.set_vgd_head(prev)
    print('%d arrays in %s (library %s)' % (len(os.listdir(out)), out, L.LIB_PATH))


def same(p, q):
    a, b = np.load(p), np.load(q)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(da, db, da2=None):
    names = sorted(set(os.listdir(da)) | set(os.listdir(db)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(da, n), os.path.join(db, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            verdict, bad = 'MISSING on one side', bad + 1
        elif da2 is not None and not same(pa, os.path.join(da2, n)):
            verdict = 'not reproducible on the first build'
        elif same(pa, pb):
            verdict = 'equal'
        else:
            a, b = np.load(pa), np.load(pb)
            verdict, bad = 'DIFFERS (%d of %d elements)' % (int((a != b).sum()) if a.shape == b.shape else -1, a.size), bad + 1
        print('%-72s %s' % (n[:-4], verdict))
    print('%d arrays, %d differ' % (len(names), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == 'compare':
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)
