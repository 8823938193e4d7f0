"""The fused grounding head without a GPU: the library exports the new entries, the host functions answer as documented, CPU
tensors take the torch composition of the reference's statements (full_vgd.py:105-114), and the switch MMNAS_VGD_HEAD is off unless
asked for."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.util import REPO, rel_err

T = torch.from_numpy


def test_library_exports_the_grounding_head_entries():
    from mmnas_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ('mmnas_vgd_head_supported', 'mmnas_vgd_head_bwd_ws_floats', 'mmnas_vgd_head_fwd', 'mmnas_vgd_head_bwd'):
        assert hasattr(raw, name), name
        assert name in L.SYMBOLS
    assert L.lib().mmnas_abi_version() == 1


def test_supported_range_at_its_edges():
    from mmnas_amd import _lib as L
    sup = L.lib().mmnas_vgd_head_supported
    assert [bool(sup(100, F)) for F in (4, 8, 2048, 2052, 1001)] == [False, True, True, False, False]
    assert [bool(sup(S, 1024)) for S in (0, 1, 1024, 1025)] == [False, True, True, False]
    # the whole documented range: every F % 4 == 0 in 8 .. 2048, every S in 1 .. 1024
    assert all(sup(1, F) for F in range(8, 2049, 4)) and all(sup(S, 8) for S in range(1, 1025))
    assert not any(sup(1, F) for F in range(8, 2049) if F % 4)


def test_workspace_size_is_positive_and_monotone_in_the_batch():
    from mmnas_amd import _lib as L
    wsf = L.lib().mmnas_vgd_head_bwd_ws_floats
    for S, F in ((1, 8), (100, 1024), (1024, 2048)):
        sizes = [wsf(B, S, F) for B in (1, 2, 3, 64, 65)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), (S, F, sizes)
    assert wsf(64, 100, 1024) >= 64 * 1024          # at least one dxp row per sample
    assert wsf(4, 100, 1001) == 0 and wsf(0, 100, 1024) == 0      # outside the range: no workspace, the call itself refuses


def test_unsupported_arguments_are_refused_before_any_launch():
    from mmnas_amd import _lib as L
    lib = L.lib()
    assert lib.mmnas_vgd_head_fwd(*([None] * 12), 2, 5, 1001, 1e-6, 1, None) == -1      # MMNAS_E_SHAPE
    assert b'F=1001' in lib.mmnas_last_error()
    assert lib.mmnas_vgd_head_fwd(*([None] * 12), 2, 5, 24, 1e-6, 1, None) == -2        # MMNAS_E_ARG: null pointers
    assert lib.mmnas_vgd_head_bwd(*([None] * 20), 2, 1025, 24, 1e-6, 1, None) == -1
    assert lib.mmnas_vgd_head_bwd(*([None] * 20), 2, 5, 24, 1e-6, 1, None) == -2


@pytest.mark.parametrize('logsm', [True, False])
def test_cpu_tensors_take_the_composition_and_backpropagate(logsm):
    from mmnas_amd import ops
    from oracle.mmnas_oracle import _linear, layer_norm
    g = torch.Generator().manual_seed(3)
    B, S, F = 3, 5, 24
    r = lambda *sh: torch.randn(*sh, generator=g)
    t = dict(yf=r(B, S, F), xp=r(B, F), a=1 + 0.1 * r(F), b=0.1 * r(F), ws=r(1, F) * F ** -0.5, bs=0.1 * r(1), wr=r(4, F) * F ** -0.5,
             br=0.1 * r(4))
    gs, gr = r(B, S), r(B, S, 4)

    def run(fn, dtype):
        p = {k: v.to(dtype).requires_grad_() for k, v in t.items()}
        scores, reg = fn(p)
        ((scores * gs.to(dtype)).sum() + (reg * gr.to(dtype)).sum()).backward()
        return [scores.detach().numpy(), reg.detach().numpy()] + [v.grad.numpy() for v in p.values()]

    def oracle(p):
        xy = layer_norm(p['xp'].unsqueeze(1) + p['yf'], p['a'], p['b'], 1e-6)
        s = _linear(xy, p['ws'], p['bs']).squeeze(-1)
        return (torch.log_softmax(s, dim=-1) if logsm else s), _linear(xy, p['wr'], p['br'])

    mine = lambda p: ops.grounding_head(p['yf'], p['xp'], p['a'], p['b'], 1e-6, p['ws'], p['bs'], p['wr'], p['br'], log_softmax=logsm)
    got, ref = run(mine, torch.float64), run(oracle, torch.float64)
    assert got[0].shape == (B, S) and got[1].shape == (B, S, 4)
    for i, (a, b) in enumerate(zip(got, ref)):
        if logsm and i == 2 + 5:       # d b_scores: a sum that is zero under log_softmax -- round-off on both sides
            assert abs(a).max() < 1e-12 and abs(b).max() < 1e-12
            continue
        assert rel_err(a, b) <= 1e-6, (i, rel_err(a, b))
    got32 = run(mine, torch.float32)                    # other dtypes run too (float32 here: the composition's own round-off)
    assert all(x.dtype == np.float32 for x in got32) and rel_err(got32[0], ref[0]) < 1e-4 and rel_err(got32[2], ref[2]) < 1e-3


def test_switch_is_off_unless_asked_for():
    code = ('import os, sys\n'
            'os.environ.pop("MMNAS_VGD_HEAD", None)\n'
            'from mmnas_amd import ops\n'
            'assert ops.vgd_head_enabled() is False\n'
            'assert ops.set_vgd_head(True) is False and ops.vgd_head_enabled() is True\n'
            'assert ops.set_vgd_head(False) is True and ops.vgd_head_enabled() is False\n'
            'print("ok")\n')
    env = {k: v for k, v in os.environ.items() if k != 'MMNAS_VGD_HEAD'}
    out = subprocess.run([sys.executable, '-c', code], cwd=REPO, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr
    env['MMNAS_VGD_HEAD'] = '1'
    out = subprocess.run([sys.executable, '-c', 'from mmnas_amd import ops; print(ops.vgd_head_enabled())'], cwd=REPO, env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == 'True', out.stderr


def test_cpu_net_full_vgd_forward_is_unchanged_by_the_switch(monkeypatch):
    """The HIP network refuses CPU tensors in its stem, long before the head; with the switch on it does so all the same, and the
    fused head is never reached."""
    from mmnas.model.full_vgd import Net_Full
    from mmnas_amd import _lib as L
    from mmnas_amd import ops
    c = cases.net_case('vgd', 'mmnas_vgd', 5, HSIZE=64, B=2, Sx=5, Sy=7, token_size=30)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Full(c['cfg'], init)
    net.load_state_dict({k: T(v) for k, v in c['P'].items()})
    keys = set(net.state_dict().keys())
    inp = tuple(T(a) for a in c['inputs'])
    calls = []
    orig = ops.grounding_head
    monkeypatch.setattr(ops, 'grounding_head', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    seen = []
    for on in (False, True):
        prev = ops.set_vgd_head(on)
        try:
            with pytest.raises(L.MMNasHipError) as ei:
                net(inp)
            seen.append(str(ei.value))
        finally:
            ops.set_vgd_head(prev)
    assert seen[0] == seen[1] and not calls
    assert set(net.state_dict().keys()) == keys      # the switch adds no parameter
