"""CPU checks of mmnas_amd.grounding: the numpy fallback against the reference's own targets and evaluation
(tests/golden/vgd.npz, make_golden_vgd.py), the float32 pairwise-sum order the targets kernel restates, argument refusals,
GroundingEvaluator's in-place BBOX_NORM swap and its all-reduce over two gloo ranks, the new entry points' host-side
validation under the AddressSanitizer build, and (opt-in) the fixture's regeneration."""
import json
import os
import shutil
import socket
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.golden import cases
from tests.util import REPO, load

T = torch.from_numpy
MODES = ('kld', 'bce')


def _batches():
    z = load('vgd.npz')
    out = []
    for k in range(int(z['n_batches'])):
        p = 'b%d|' % k
        d = {key[len(p):]: z[key] for key in z.files if key.startswith(p)}
        norm = d['norm']
        d['cfg'] = SimpleNamespace(OVERLAP_THRESHOLD=float(d['thr']), SCORES_LOSS=MODES[int(d['mode'])], BBOX_NORM=norm.size > 0,
                                   BBOX_NORM_MEANS=list(norm[:4]), BBOX_NORM_STDS=list(norm[4:]))
        out.append(d)
    return out


def ulps32(a, b):
    """Distance in float32 units in the last place (same-sign finite values; 0 where bitwise equal)."""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


BATCHES = _batches()


@pytest.mark.parametrize('k', range(len(BATCHES)))
def test_targets_fallback_against_the_reference(k):
    from mmnas_amd.grounding import _iou_np, grounding_targets
    d = BATCHES[k]
    t = grounding_targets(T(d['bbox']), T(d['nobj']), T(d['gt']), d['cfg'])
    assert np.array_equal(t['scores_mask'].numpy(), d['t_scores_mask'])
    assert np.array_equal(t['bbox_mask'].numpy(), d['t_bbox_mask'])
    # the fallback sums the scores with numpy itself: bitwise
    assert np.array_equal(t['scores'].numpy(), d['t_scores'])
    assert int(ulps32(t['bbox'].numpy(), d['t_bbox']).max()) <= 1
    for b in range(d['bbox'].shape[0]):
        n = int(d['nobj'][b])
        iou = _iou_np(d['bbox'][b, :n].astype(np.float64), d['gt'][b])
        assert np.array_equal(iou, d['t_iou'][b, :n])
        assert not d['t_scores'][b, n:].any() and not d['t_bbox'][b, n:].any() and not d['t_bbox_mask'][b, n:].any()


def test_fixture_covers_the_edge_cases():
    c = BATCHES[4]   # the crafted batch: see make_golden_vgd._crafted_batch
    assert list(c['t_scores_mask'][:, 0]) == [1, 1, 0, 1, 0, 0, 1, 1, 1, 1]
    assert c['t_iou'][0, 0] == 1.0 and c['t_iou'][1, 0] == 0.5 and c['t_iou'][9, 0] == 0.5 and not c['t_iou'][2].any()
    assert list(c['e_iou'][[0, 1, 9]]) == [1.0, 0.5, 0.5] and c['e_hit'][[0, 1, 9]].all()
    assert c['e_idx'][6] == 3 and c['pred_scores'][6, 3] == c['pred_scores'][6, 7]      # tie: the lower index
    assert c['e_idx'][7] == 50 and c['nobj'][7] == 5                                       # a padded row wins
    assert abs(c['pred_reg'][8, 0, 2]) >= 9.5 and list(c['e_box'][8]) == [0, 0, 639, 479]  # clipped whole-image box
    assert c['t_bbox'][5].any() and not c['t_scores'][5].any()                            # no target, boxes still filled


@pytest.mark.parametrize('k', range(len(BATCHES)))
def test_ground_fallback_against_the_reference(k):
    from mmnas_amd.grounding import ground_batch
    d = BATCHES[k]
    thr = float(d['thr'])
    r = ground_batch(T(d['pred_scores']), T(d['pred_reg']), T(d['bbox']), T(d['img_shape']), T(d['gt32']), thr)
    assert np.array_equal(r['idx'].numpy(), d['e_idx'])
    assert int(ulps32(r['box'].numpy(), d['e_box']).max()) <= 4
    # the same numpy exp as the reference host here: the boxes and the IoU come out bitwise
    assert np.array_equal(r['box'].numpy(), d['e_box'])
    assert np.array_equal(r['iou'].numpy(), d['e_iou'])
    near = np.abs(d['e_iou'] - thr) < 1e-5
    exact = d['e_iou'] == thr
    assert int((near & ~exact).sum()) == 0
    assert np.array_equal(r['hit'].numpy(), d['e_hit'])


def pairwise_sum_restated(a):
    """The order mmnas_vgd_targets sums the kld scores in (grounding.hip pw_sum), restated in Python float32."""
    f = np.float32
    n = len(a)
    if n > 128:
        n2 = n // 2
        n2 -= n2 % 8
        return f(pairwise_sum_restated(a[:n2]) + pairwise_sum_restated(a[n2:]))
    if n < 8:
        r = f(-0.0)
        for v in a:
            r = f(r + v)
        return r
    r = [f(v) for v in a[:8]]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = f(r[j] + a[i + j])
        i += 8
    res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
    for v in a[i:]:
        res = f(res + v)
    return res


def test_pairwise_order_is_numpys():
    rs = np.random.RandomState(3)
    for n in list(range(1, 140)) + [255, 256, 257, 500, 519, 777, 1000, 1023, 1024]:
        a = (rs.uniform(0.5, 1, n) * (rs.uniform(size=n) < 0.4)).astype(np.float32)
        assert pairwise_sum_restated(a) == a.sum(), n


def _cfg(**kw):
    c = dict(OVERLAP_THRESHOLD=0.5, SCORES_LOSS='kld', BBOX_NORM=False, BBOX_NORM_MEANS=None, BBOX_NORM_STDS=None)
    c.update(kw)
    return SimpleNamespace(**c)


def test_argument_refusals():
    from mmnas_amd.grounding import GroundingError, ground_batch, grounding_targets
    d = BATCHES[0]
    bbox, nobj, gt = T(d['bbox']), T(d['nobj']), T(d['gt'])
    S = bbox.shape[1]
    for bad in (0, S + 1):
        n = nobj.clone()
        n[3] = bad
        with pytest.raises(GroundingError, match='nobj'):
            grounding_targets(bbox, n, gt, _cfg())
    with pytest.raises(TypeError):
        grounding_targets(bbox.double(), nobj, gt, _cfg())
    with pytest.raises(TypeError):
        grounding_targets(bbox, nobj, gt.float(), _cfg())
    with pytest.raises(TypeError):
        grounding_targets(bbox, nobj.float(), gt, _cfg())
    with pytest.raises(ValueError):
        grounding_targets(bbox[:, :, :3].contiguous(), nobj, gt, _cfg())
    with pytest.raises(ValueError):
        grounding_targets(bbox, nobj[1:], gt, _cfg())
    with pytest.raises(ValueError):
        grounding_targets(torch.zeros(2, 1025, 4), torch.ones(2, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.float64), _cfg())
    with pytest.raises(ValueError, match='SCORES_LOSS'):
        grounding_targets(bbox, nobj, gt, _cfg(SCORES_LOSS='l1'))
    for v in (float('nan'), float('inf')):
        g = gt.clone()
        g[2, 1] = v
        with pytest.raises(GroundingError, match='NaN or infinite'):
            grounding_targets(bbox, nobj, g, _cfg())
        b = bbox.clone()
        b[1, 7, 2] = v
        with pytest.raises(GroundingError, match='NaN or infinite'):
            grounding_targets(b, nobj, gt, _cfg())
    args = [T(d[k]) for k in ('pred_scores', 'pred_reg', 'bbox', 'img_shape', 'gt32')]
    ground_batch(*args, 0.5)
    for i, v in ((0, float('nan')), (0, float('inf')), (1, float('nan')), (1, -float('inf'))):
        a = [x.clone() for x in args]
        a[i].view(-1)[17] = v
        with pytest.raises(GroundingError, match='NaN or infinite'):
            ground_batch(*a, 0.5)
    for i in range(5):
        a = list(args)
        a[i] = a[i].double()
        with pytest.raises(TypeError):
            ground_batch(*a, 0.5)
        a = list(args)
        a[i] = a[i][1:]
        with pytest.raises(ValueError):
            ground_batch(*a, 0.5)


# ---- GroundingEvaluator on the CPU -----------------------------------------------------------------------------------------------
def _vgd_net(seed=5):
    from mmnas.model.full_vgd import Net_Full
    c = cases.net_case('vgd', 'mmnas_vgd', seed, HSIZE=64, B=2, Sx=5, Sy=7, token_size=30)
    net = Net_Full(c['cfg'], {'token_size': c['token_size'], 'ans_size': c['ans_size'],
                              'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)})
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    return net, c


class _Replay(torch.nn.Module):
    """A stand-in VGD network for host tests: returns recorded outputs for the sample ids it is given."""
    TASK = 'vgd'

    def __init__(self, scores, reg):
        super().__init__()
        self.proj_reg = torch.nn.Linear(8, 4)
        self.scores, self.reg = scores, reg

    def forward(self, inputs):
        ids = inputs[0]
        return self.scores[ids], self.reg[ids]


def test_bbox_norm_swap_is_in_place_and_restored():
    from mmnas_amd.grounding import GroundingEvaluator
    net, c = _vgd_net()
    net.train()
    net.backnone.eval()          # mixed flags: every module's own flag must come back
    flags = {n: m.training for n, m in net.named_modules()}
    W, b = net.proj_reg.weight, net.proj_reg.bias
    w0, b0 = W.detach().clone(), b.detach().clone()
    ptrs = (W.data_ptr(), b.data_ptr())
    cfg = _cfg(BBOX_NORM=True, BBOX_NORM_MEANS=[0.01, -0.02, 0.05, -0.1], BBOX_NORM_STDS=[0.1, 0.13, 0.2, 0.27])
    ev = GroundingEvaluator(net, cfg)
    std = torch.from_numpy(np.array(cfg.BBOX_NORM_STDS)).float()
    mean = torch.from_numpy(np.array(cfg.BBOX_NORM_MEANS)).float()
    seen = {}
    B, S = 2, 7
    rs = np.random.RandomState(0)
    ps, pr = T(rs.standard_normal((B, S)).astype(np.float32)), T((0.1 * rs.standard_normal((B, S, 4))).astype(np.float32))

    def fwd(inputs):
        seen['W'], seen['b'] = W.detach().clone(), b.detach().clone()
        seen['training'] = any(m.training for m in net.modules())
        seen['grad'] = torch.is_grad_enabled()
        return ps, pr
    net.forward = fwd
    bbox = T(np.tile(np.array([[10, 10, 50, 50]], np.float32), (B, S, 1)))
    img = T(np.array([[300, 400]] * B, np.float32))
    gt = T(np.array([[10, 10, 50, 50]] * B, np.float32))
    ev.update(c['inputs'], bbox, img, gt)
    # the reference's float32 ops (train_vgd.py:412-420): two separate roundings
    assert torch.equal(seen['W'], w0 * torch.unsqueeze(std, 1)) and torch.equal(seen['b'], b0 * std + mean)
    assert not seen['training'] and not seen['grad']
    assert torch.equal(W, w0) and torch.equal(b, b0) and (W.data_ptr(), b.data_ptr()) == ptrs
    assert {n: m.training for n, m in net.named_modules()} == flags
    r = ev.compute()
    assert r['count'] == B and 0 <= r['hits'] <= B

    def boom(inputs):
        assert not torch.equal(W, w0)
        raise RuntimeError('forward failed')
    net.forward = boom
    with pytest.raises(RuntimeError, match='forward failed'):
        ev.update(c['inputs'], bbox, img, gt)
    assert torch.equal(W, w0) and torch.equal(b, b0) and (W.data_ptr(), b.data_ptr()) == ptrs
    assert {n: m.training for n, m in net.named_modules()} == flags
    del net.forward
    # the real forward of the HIP network refuses CPU tensors: the parameters come back all the same
    with pytest.raises(Exception):
        ev.update(tuple(T(a) for a in c['inputs']), bbox, img, gt)
    assert torch.equal(W, w0) and torch.equal(b, b0) and (W.data_ptr(), b.data_ptr()) == ptrs
    assert {n: m.training for n, m in net.named_modules()} == flags


def test_evaluator_refuses_other_networks():
    from mmnas_amd.grounding import GroundingEvaluator
    with pytest.raises(ValueError, match='VGD'):
        GroundingEvaluator(torch.nn.Linear(2, 2), _cfg())


def _replay_data():
    rs = np.random.RandomState(11)
    N, S = 24, 100
    d = BATCHES[0]
    scores = T(rs.standard_normal((N, S)).astype(np.float32))
    reg = T((0.2 * rs.standard_normal((N, S, 4))).astype(np.float32))
    bbox = T(np.concatenate([d['bbox'], d['bbox'][:8]]))
    gt = T(np.concatenate([d['gt32'], d['gt32'][:8]]))
    img = T(np.concatenate([d['img_shape'], d['img_shape'][:8]]))
    for i in range(0, N, 2):    # make some hits: the best proposal wins
        from mmnas_amd.grounding import _iou_np
        n = int(np.concatenate([d['nobj'], d['nobj'][:8]])[i])
        scores[i, int(np.argmax(_iou_np(bbox[i, :n].double().numpy(), gt[i, 0].double().numpy())))] = 10.0
        reg[i] = 0
    return scores, reg, bbox, img, gt


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_rank(rank, port, out):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=2)
    try:
        from mmnas_amd.grounding import GroundingEvaluator
        scores, reg, bbox, img, gt = _replay_data()
        ev = GroundingEvaluator(_Replay(scores, reg), _cfg())
        N = scores.shape[0]
        mine = torch.arange(N)[rank::2]
        for s in range(0, len(mine), 5):     # batches of 5 (the last one short)
            ids = mine[s:s + 5]
            ev.update((ids, None, None, None, None), bbox[ids], img[ids], gt[ids])
        r = ev.compute()
        with open(os.path.join(out, 'rank%d.json' % rank), 'w') as f:
            json.dump(r, f)
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_equal_one_rank(tmp_path):
    from mmnas_amd.grounding import GroundingEvaluator
    scores, reg, bbox, img, gt = _replay_data()
    ev = GroundingEvaluator(_Replay(scores, reg), _cfg())
    N = scores.shape[0]
    ev.update((torch.arange(N), None, None, None, None), bbox, img, gt)
    one = ev.compute()
    assert one['count'] == N and 0 < one['hits'] < N
    mp.spawn(_gloo_rank, args=(_port(), str(tmp_path)), nprocs=2, join=True)
    for rank in range(2):
        with open(os.path.join(str(tmp_path), 'rank%d.json' % rank)) as f:
            assert json.load(f) == one
    ev.reset()
    assert ev.compute()['count'] == 0


# ---- the new entry points' host-side validation under the AddressSanitizer build ------------------------------------------------
ASAN_DRIVER = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from mmnas_amd import _lib as L
l = L.lib()
buf = (C.c_double * 64)()
p = C.cast(buf, C.c_void_p).value
E_SHAPE, E_ARG = -1, -2
assert l.mmnas_vgd_targets(p, p, p, -1, 100, 0.5, 0, None, p, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vgd_targets(p, p, p, 4, 0, 0.5, 0, None, p, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vgd_targets(p, p, p, 4, 1025, 0.5, 0, None, p, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vgd_targets(p, p, p, 4, 100, 0.5, 2, None, p, p, p, p, p, None) == E_ARG
assert l.mmnas_vgd_targets(p, None, p, 4, 100, 0.5, 0, None, p, p, p, p, p, None) == E_ARG
assert b'vgd_targets: null pointer' in l.mmnas_last_error()
assert l.mmnas_vgd_targets(p, p, p, 0, 100, 0.5, 1, p, p, p, p, p, p, None) == 0      # B = 0: nothing launched
assert l.mmnas_vgd_ground(p, p, p, p, p, -2, 100, 0.5, p, p, p, p, None, p, None) == E_SHAPE
assert l.mmnas_vgd_ground(p, p, p, p, p, 4, 2000, 0.5, p, p, p, p, None, p, None) == E_SHAPE
assert l.mmnas_vgd_ground(p, p, None, p, p, 4, 100, 0.5, p, p, p, p, None, p, None) == E_ARG
assert l.mmnas_vgd_ground(p, p, p, p, p, 4, 100, 0.5, p, p, p, p, p, None, None) == E_ARG
assert l.mmnas_vgd_ground(p, p, p, p, p, 0, 100, 0.5, p, p, p, p, None, p, None) == 0
print('VGD_HOST_OK')
"""


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_vgd_entry_points_validate_under_address_sanitizer():
    csrc = os.path.join(REPO, 'mmnas_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, 'asan', '-j4'], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    lib = os.path.join(REPO, 'mmnas_amd', 'lib', 'libmmnas_hip_asan.so')
    rt = subprocess.run(['hipcc', '-print-file-name=libclang_rt.asan-x86_64.so'], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip('ASan runtime of the ROCm clang not found')
    env = dict(os.environ, LD_PRELOAD=rt, MMNAS_LIB_PATH=lib,
               ASAN_OPTIONS='detect_leaks=0:verify_asan_link_order=0:abort_on_error=1:halt_on_error=1')
    p = subprocess.run([sys.executable, '-c', ASAN_DRIVER % REPO], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'VGD_HOST_OK' in p.stdout, (p.stdout[-1500:], p.stderr[-4000:])
    assert 'AddressSanitizer' not in p.stderr, p.stderr[-4000:]


# ---- the fixture's recipe (opt-in: needs the reference checkout) ------------------------------------------------------------------
REF = os.environ.get('MMNAS_REFERENCE', '/root/reference')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'mmnas')) or os.environ.get('MMNAS_REGEN_VGD') != '1',
                    reason='opt-in (MMNAS_REGEN_VGD=1, needs the reference tree)')
def test_vgd_golden_regenerates_bit_exact(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import tests.golden.make_golden_vgd as mg\n"
            "mg.HERE = %r\n"
            "mg.gen_vgd()\n" % (REPO, str(tmp_path)))
    r = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(os.path.join(str(tmp_path), 'vgd.npz'))
    old = load('vgd.npz')
    assert sorted(new.files) == sorted(old.files)
    for k in new.files:
        assert np.array_equal(new[k], old[k]), k
