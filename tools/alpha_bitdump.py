"""Every output of the five architecture-update entry points of mmnas_amd/arch_update.py (csrc/alpha.hip), written as .npy: two
builds are compared array for array, bit for bit.  The inputs are the ones the tests define and nothing else:
tests/adam_cases.alpha_case ('full'), the 'two' cases of tests/test_arch_two_gpu.py, tests/arch_cost_cases.case (both modes,
both forms, the weights of the tests and weight 0) and tests/arch_reinforce_cases.combos(), each under the optimizer settings
its test uses.  One array per output (prob, m, v, prob_grad, stats, baseline) and chain, the steps stacked along axis 0.

    MMNAS_LIB_PATH=<build A> python tools/alpha_bitdump.py dump DIR_A [--device cpu|cuda]        (one process per library)
    MMNAS_LIB_PATH=<build B> python tools/alpha_bitdump.py dump DIR_B [--device cpu|cuda]
    python tools/alpha_bitdump.py compare DIR_A DIR_B

--device cpu (the default is cuda) takes the torch restatements instead of the kernels; ops.alpha_full_step has none and is
left out there.  `compare` prints one line per array, equal / DIFFERS; exit status 1 when one differs or is missing on one side.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def dump(out, device):
    import torch
    from mmnas_amd import _lib as L, ops
    from tests import adam_cases as A, arch_cost_cases as AC, arch_reinforce_cases as RC, test_arch_two_gpu as G
    from tests.test_arch_two_host import SETTINGS

    dev = 'cuda:0' if device == 'cuda' else 'cpu'
    T = torch.from_numpy
    os.makedirs(out, exist_ok=True)

    def save(prefix, steps):
        """steps: one dict of arrays (or None) per step."""
        for k in steps[0]:
            if steps[0][k] is not None:
                np.save(os.path.join(out, '%s.%s.npy' % (prefix, k)), np.stack([np.asarray(s[k]) for s in steps]))

    def host(**tensors):
        return {k: t.detach().cpu().numpy().copy() for k, t in tensors.items()}

    if dev != 'cpu':      # mmnas_alpha_full_step[_wd]
        for rows, width in A.ALPHA_SHAPES:
            for betas in A.ALPHA_BETAS:
                for wd in A.ALPHA_WDS:
                    c = A.alpha_case(rows, width, betas, wd)
                    prob = T(c['a0'].copy()).to(dev)
                    m, v, pg = torch.zeros_like(prob), torch.zeros_like(prob), torch.zeros_like(prob)
                    steps = []
                    for t in range(A.ALPHA_STEPS):
                        ops.alpha_full_step(prob, T(c['gg'][t].copy()).to(dev), m, v, pg, A.ALPHA_LR, betas, A.ALPHA_EPS, t + 1,
                                            weight_decay=wd)
                        steps.append(host(prob=prob, m=m, v=v, prob_grad=pg))
                    save('full.%dx%d.b%g.wd%g' % (rows, width, betas[0], wd), steps)
    # mmnas_alpha_two_step
    for rows, width in G.SHAPES:
        _, a0, pairs, gg = G._case(rows, width, 4, 100 + rows)
        for s, (lr, betas, wd) in enumerate(SETTINGS):
            prob = T(a0.copy()).to(dev)
            m, v, pg = torch.zeros_like(prob), torch.zeros_like(prob), torch.zeros_like(prob)
            steps = []
            for t in range(4):
                ops.alpha_two_step(prob, T(gg[t]).to(dev), m, v, pg, [tuple(int(x) for x in p) for p in pairs[t]], lr, betas, G.EPS,
                                   t + 1, weight_decay=wd)
                steps.append(host(prob=prob, m=m, v=v, prob_grad=pg))
            save('two.%dx%d.s%d' % (rows, width, s), steps)
    # mmnas_alpha_full_step_cost / mmnas_alpha_two_step_cost
    for mode in ('full', 'two'):
        for key in AC.combos(mode) + [(mode, rows, width, form, 0.0) for rows, width in AC.SHAPES[mode] for form in AC.FORMS]:
            for s in range(len(SETTINGS)):
                save('cost.%s.%dx%d.%s.w%g.s%d' % (key + (s,)), AC.replay(AC.case(*key), s, torch.float32, dev))
    # mmnas_alpha_reinforce_step
    for key in RC.combos():
        for s in range(len(SETTINGS)):
            steps = RC.replay(RC.case(*key), s, torch.float32, dev)
            assert not any(st.pop('err') for st in steps), key
            save('reinforce.%dx%d.M%d.%s.s%d' % (key + (s,)), steps)
    print('%d arrays in %s (device %s, library %s)' % (len(os.listdir(out)), out, dev, L.LIB_PATH if dev != 'cpu' else 'not used'))


def same(p, q):
    a, b = np.load(p), np.load(q)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare(da, db):
    names = sorted(set(os.listdir(da)) | set(os.listdir(db)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(da, n), os.path.join(db, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            verdict, bad = 'MISSING on one side', bad + 1
        elif same(pa, pb):
            verdict = 'equal'
        else:
            a, b = np.load(pa), np.load(pb)
            differ = int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(axis=1).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1
            verdict, bad = 'DIFFERS (%d of %d elements)' % (differ, a.size), bad + 1
        print('%-48s %s' % (n[:-4], verdict))
    print('%d arrays, %d differ' % (len(names), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    args = sys.argv[1:]
    device = 'cuda'
    if '--device' in args:
        i = args.index('--device')
        device = args[i + 1]
        del args[i:i + 2]
    if len(args) == 2 and args[0] == 'dump' and device in ('cpu', 'cuda'):
        dump(args[1], device)
    elif len(args) == 3 and args[0] == 'compare':
        sys.exit(compare(args[1], args[2]))
    else:
        sys.exit(__doc__)
