"""The kernels that only a runtime switch selects (docs/SWITCHES.md), each case of tests/fallback_cases.py in a fresh child
process: most native switches are read once per process and have no setter, so the in-process kernel tests see the default
side only.  One child at a time; the environment is this process's plus the case's switches.  Each test asserts, in order: the
child ran to the end; every switch of the case reports the intended value, from the environment, and was READ by the code
under test (a case whose switch never took effect must not pass as a test of the default path); every error is under the
bound of the default-path test the case borrows its shapes from (fallback_cases.BOUNDS).

What the 'read' check is worth: a row read ONCE carries the unread flag until the code under test consults it, so the check
shows that the dispatch that owns the switch was entered -- not that the shape then qualified for the other kernel (for
MMNAS_MHA_PAIR: mha_core_fwd_pair was entered; that the 100-region shape splits into two launches follows from its geometry
test, attention.hip).  Rows read at EVERY call (MMNAS_MHA_NW, MMNAS_SIDE_PRIO, MMNAS_HEAD_PROJT, MMNAS_REL_FWD_VALU) never carry
the flag: for them the check shows only that the value arrived from the environment, and which kernels they select rests on
the dispatch code (launch_fwd / launch_bwd in attention.hip, side_ctx and att_core_fwd in ops.hip).

Once a child ends by a signal or by its time limit, every later test of this module fails at once without starting another
process: nothing more is started on a device that has just faulted or hung."""
import json
import os
import subprocess
import sys

import pytest

from tests import fallback_cases as F
from tests.util import REPO

pytestmark = pytest.mark.gpu

# A child imports torch and loads the library (10-20 s when nothing is cached), runs a handful of small launches and the float64
# references of shapes with at most 3 x 128 x 128 scores (well under a second each), and at most eight tiny networks.  The
# limit is several times that: it ends a hung child, it is not something a healthy one comes near.
TIMEOUT = 240
TRIPPED = []          # why nothing more is started
INCLUSIVE = {'r', 'r_vs_per_op', 'grads_over_bound'}       # asserted with <= by the mirrored tests; everything else with <
GPU_FAULT_TEXT = ('illegal memory access', 'HSA_STATUS_ERROR', 'Memory access fault', 'hipErrorLaunchFailure', 'unspecified launch failure')
WANT = {'MMNAS_SIDE_FLUSH': 1}                               # a string row reports 1 when set and not empty


def _not_tripped():
    if TRIPPED:
        pytest.fail('not started: ' + TRIPPED[0], pytrace=False)


def _run_case(name):
    _not_tripped()
    case = F.CASES[name]
    env = dict(os.environ)
    env.update(case['env'])
    try:
        p = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'fallback_cases.py'), name], cwd=REPO, env=env,
                           capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired as e:
        TRIPPED.append('the child of case %s did not finish within %d s' % (name, TIMEOUT))
        pytest.fail(TRIPPED[0] + '\n' + str(e.stdout)[-1500:] + '\n' + str(e.stderr)[-3000:], pytrace=False)
    if p.returncode < 0 or p.returncode in (134, 139, 124, 137):
        TRIPPED.append('the child of case %s ended with status %d' % (name, p.returncode))
    elif p.returncode != 0 and any(t in p.stderr for t in GPU_FAULT_TEXT):
        # (a GPU fault that reached Python as an exception: the child exits 1, the device has faulted all the same)
        TRIPPED.append('the child of case %s reported a GPU fault (status %d)' % (name, p.returncode))
    assert p.returncode == 0, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]
    assert lines and lines[-1] == {'case': name, 'done': len(case['shapes'])}, p.stdout[-1500:]
    return lines[:-1]


@pytest.mark.parametrize('name', list(F.CASES))
def test_fallback_case(name):
    case = F.CASES[name]
    lines = _run_case(name)
    assert len(lines) == len(case['shapes'])
    last = lines[-1]['switches']
    for k, text in case['env'].items():
        assert last[k]['value'] == WANT.get(k, int(text) if text.lstrip('-').isdigit() else None), (k, last[k])
        assert last[k]['source'] == 'environment' and last[k]['read'], (k, last[k])
    for shape, line in zip(case['shapes'], lines):
        assert line['shape'] == json.loads(json.dumps(shape))
        print(name, line['shape'], line['errors'], line['notes'])
        bounds = F.bounds_of(name, shape)
        assert line['errors'] and set(line['errors']) <= set(bounds), line['errors']
        for k, e in line['errors'].items():
            ok = e <= bounds[k] if k in INCLUSIVE else e < bounds[k]        # (a NaN fails either)
            assert ok, (name, shape, k, e, bounds[k], line['notes'])


# ------------------------------------------------------------------------ switches read at every call: in this process
def _lone_rel_self_att(dims):
    """test_rel_self_att_with_lazy_handle's operator (tests/test_ops_gpu.py) fed a RelHandle, forward + backward: -> the output
    and every gradient, as numpy arrays."""
    import numpy as np
    import torch
    from mmnas_amd.model.modules import RelHandle
    from mmnas_amd.utils.ops_adapter import OpsAdapter
    from tests.golden import cases
    case = cases.op_case('rel_self_att_64', True, True, 2024, dims)
    rs = np.random.RandomState(7)
    B, S = dims['B'], dims['Sx']
    raw = rs.standard_normal((B, S, S, 4)).astype(np.float32)
    raw[:, S - 2:] = 0
    raw[:, :, S - 2:] = 0
    Wy = (rs.standard_normal((64, 4)) / 2).astype(np.float32)
    by = (0.1 * rs.standard_normal(64)).astype(np.float32)
    op = OpsAdapter().OPS['rel_self_att_64'](case['cfg'], norm=True, residual=True)
    op.load_state_dict({k: torch.from_numpy(v) for k, v in case['P'].items()})
    op = op.to('cuda').train()
    x = torch.from_numpy(case['x']).to('cuda').requires_grad_(True)
    Wyd = torch.from_numpy(Wy).to('cuda').requires_grad_(True)
    byd = torch.from_numpy(by).to('cuda').requires_grad_(True)
    h = RelHandle(torch.from_numpy(raw).to('cuda'), Wyd, byd)
    out = op(x, None, torch.from_numpy(case['x_mask']).to('cuda'), None, h)
    out.backward(torch.from_numpy(case['gout']).to('cuda'))
    assert h._dense is None                      # the lazy route: the [B,S,S,64] tensor was never built
    res = {'out': out.detach().cpu().numpy(), 'dx': x.grad.cpu().numpy(), 'dWy': Wyd.grad.cpu().numpy(), 'dby': byd.grad.cpu().numpy()}
    res.update({'g:' + k: p.grad.cpu().numpy() for k, p in op.named_parameters()})
    return res


@pytest.mark.parametrize('dims', [dict(B=3, Sx=7, Sy=5, HSIZE=128), dict(B=4, Sx=100, Sy=14, HSIZE=512)], ids=['S7', 'S100'])
def test_lone_rel_self_att_through_the_per_operator_fused_kernel(dims, monkeypatch):
    """MMNAS_REL_FWD_VALU=1 (read at every call): a lone RelSelfAtt fed a lazy RelHandle -- the only input for which
    att_core_fwd (ops.hip) consults the switch -- computes its bias with rel_fused_fwd_kernel (relfused.hip) instead of the
    one-operator form of rel_multi_fwd_kernel.  (1) test_rel_self_att_with_lazy_handle's own checks against the float64 oracle,
    at its bounds, under the switch.  (2) Against the default setting in this process: the two kernels evaluate the same two
    layers in fp32 with different summation orders; each setting is within (1)'s bound of float64 (the default by the test
    borrowed from), so the two are within twice that bound of each other -- and, both kernels being deterministic, an output
    that is NOT bit-identical shows that the switch changed the kernel that ran."""
    import numpy as np
    from tests.test_ops_gpu import test_rel_self_att_with_lazy_handle
    from tests.util import TOL, rel_err
    _not_tripped()
    monkeypatch.setenv('MMNAS_REL_FWD_VALU', '1')
    test_rel_self_att_with_lazy_handle(dims)
    got = _lone_rel_self_att(dims)
    monkeypatch.setenv('MMNAS_REL_FWD_VALU', '0')
    ref = _lone_rel_self_att(dims)
    again = _lone_rel_self_att(dims)
    assert np.array_equal(ref['out'], again['out'])          # deterministic: a difference below is the switch's
    for k in ref:
        e = rel_err(got[k], ref[k])
        print(dims['Sx'], k, e)
        assert e <= 2 * (TOL if k in ('out', 'dx') else 3e-3), (k, e)
    assert not np.array_equal(got['out'], ref['out']), 'MMNAS_REL_FWD_VALU=1 gave the bit pattern of the default kernel'


def test_head_projection_gradients_from_the_untransposed_loss_gradient(monkeypatch):
    """MMNAS_HEAD_PROJT=0: the answer projection's backward as the TN / NN pair on the loss gradient as it is, instead of the
    products on its transpose.  B = 4 with 13 answers is a shape at which the transposed form is the default (ANS % 4 != 0,
    B % 4 == 0).  Same logits; every parameter gradient against the default setting in this process, at the bound of
    test_head_one_glimpse_kernels_equal_the_gemm_form (tests/test_chain_gpu.py), which swaps another of the head's products
    for an equivalent form the same way: 3e-4 of the tensor's largest entry, floored at 1e-3 of the network's largest."""
    import numpy as np
    from tests.test_chain_gpu import _run
    from tests.util import rel_err
    _not_tripped()
    res = {}
    for projt in ('1', '0'):
        monkeypatch.setenv('MMNAS_HEAD_PROJT', projt)
        res[projt] = _run('vqa', 'mmnas_vqa', False, True, False, monkeypatch, B=4)
    (out_a, g_a, n_a), (out_b, g_b, n_b) = res['0'], res['1']
    assert n_a == 1 and n_b == 1
    assert rel_err(out_a, out_b) < 2e-6
    top = max(float(np.abs(g).max()) for g in g_b.values() if g is not None)
    assert float(np.abs(g_b['proj.weight']).max()) > 0
    for k in g_b:
        if g_b[k] is None:
            assert g_a[k] is None or not np.any(g_a[k]), k
            continue
        diff = float(np.abs(g_a[k] - g_b[k]).max())
        assert diff <= 3e-4 * max(float(np.abs(g_b[k]).max()), 1e-3 * top), (k, diff)
