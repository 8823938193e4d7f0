"""Host side of the NET_OPTIM = 'sgd' path (no GPU): optim.CosineSchedule against torch's CosineAnnealingLR, the
constructor guards of SearchLoop, the exported symbols, and the key layout of tests/golden/traj_sgd.npz."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.golden.cases_sgd import SGD_HYPER, SGD_WEIGHT_PLANS
from tests.util import load

T_MAX, BASE, ETA_MIN = 200, 0.05, 0.0005


def _sgd():
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], BASE, momentum=0.9)


def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def _torch_logged_rate(sched):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')           # ("use get_last_lr()": the scripts do call get_lr(), search_vqa.py:359)
        return sched.get_lr()[0]


def _follow(mine, ms, ref, ts, epochs):
    """The scripts' epoch loop: step() at the top of the epoch, then the applied rate and the logged one on both sides."""
    for epoch in epochs:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')       # (torch warns that no optimizer.step() came first: the scripts' order)
            ts.step()
        ms.step()
        assert ms.last_epoch == ts.last_epoch
        a, b = mine.param_groups[0]['lr'], ref.param_groups[0]['lr']
        assert _close(a, b), ('applied', epoch, a, b)
        assert _close(ms.last_lr(), b)
        la, lb = ms.rate(), _torch_logged_rate(ts)
        assert _close(la, lb), ('logged', epoch, la, lb)


def test_cosine_schedule_equals_torch_cosine_annealing_over_every_epoch_and_after_a_resume():
    from mmnas_amd.optim import CosineSchedule
    mine, ref = _sgd(), _sgd()
    ts = torch.optim.lr_scheduler.CosineAnnealingLR(ref, T_MAX, eta_min=ETA_MIN)
    ms = CosineSchedule(mine, T_MAX, eta_min=ETA_MIN)
    assert mine.param_groups[0]['initial_lr'] == BASE and mine.param_groups[0]['lr'] == BASE      # construction changes nothing
    _follow(mine, ms, ref, ts, range(0, 37))
    ck_mine, ck_ref = mine.state_dict(), ref.state_dict()          # `'net_optim': net_optim.state_dict()` at the end of epoch 36
    assert ck_mine['param_groups'][0]['initial_lr'] == BASE
    _follow(mine, ms, ref, ts, range(37, T_MAX + 1))               # ... every epoch 0..200: past the minimum, onto the rising branch
    assert _close(ms.last_lr(), ref.param_groups[0]['lr'])
    # the stepping point: epoch e trains at the closed form's value for e + 1 (step() comes BEFORE the epoch's steps) ...
    probe = _sgd()
    ps = CosineSchedule(probe, T_MAX, eta_min=ETA_MIN)
    ps.step()
    want = ETA_MIN + (BASE - ETA_MIN) * (1 + np.cos(np.pi * 1 / T_MAX)) / 2
    assert abs(ps.last_lr() - want) < 1e-12
    # ... and the logged figure is NOT the applied one: get_lr() outside step() applies the recursion once more (kept quirk)
    want_logged = ETA_MIN + (BASE - ETA_MIN) * (1 + np.cos(np.pi * 1 / T_MAX)) / 2 * (1 + np.cos(np.pi / T_MAX)) / 2
    assert abs(ps.rate() - want_logged) < 1e-12 and ps.rate() < ps.last_lr()
    # resume at epoch 37 as search_vqa.py:226-231 does: fresh optimizer, load its checkpoint, schedule with last_epoch=start_epoch
    mine2, ref2 = _sgd(), _sgd()
    mine2.load_state_dict(ck_mine)
    ref2.load_state_dict(ck_ref)
    ts2 = torch.optim.lr_scheduler.CosineAnnealingLR(ref2, T_MAX, eta_min=ETA_MIN, last_epoch=37)
    ms2 = CosineSchedule(mine2, T_MAX, eta_min=ETA_MIN, last_epoch=37)
    assert ms2.last_epoch == ts2.last_epoch and ms2.base_lrs == ts2.base_lrs
    assert _close(mine2.param_groups[0]['lr'], ref2.param_groups[0]['lr'])
    _follow(mine2, ms2, ref2, ts2, range(37, T_MAX + 1))
    # its own state_dict carries the position
    ms3 = CosineSchedule(_sgd(), 7)
    ms3.load_state_dict(ms2.state_dict())
    assert (ms3.T_max, ms3.eta_min, ms3.last_epoch, ms3.base_lrs) == (ms2.T_max, ms2.eta_min, ms2.last_epoch, ms2.base_lrs)
    with pytest.raises(KeyError, match='initial_lr'):
        CosineSchedule(_sgd(), T_MAX, last_epoch=5)               # resuming without the optimizer's checkpoint


def _cpu_net():
    from mmnas.model.hygr_vqa import Net_Search
    c = cases.net_case('vqa', None, 1, search=True)
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    return Net_Search(c['cfg'], init)


def test_search_loop_guards_its_net_optim_argument():
    from mmnas_amd.harness import SearchLoop
    net = _cpu_net()
    with pytest.raises(ValueError, match='max_epoch'):
        SearchLoop(net, net_optim='sgd')
    with pytest.raises(ValueError, match='NET_OPTIM'):
        SearchLoop(net, net_optim='adamw', max_epoch=5)
    with pytest.raises(ValueError, match='NET_OPTIM'):
        SearchLoop(net, net_optim='SGD', max_epoch=5)


def test_flat_sgd_refuses_the_cpu_and_checks_its_arguments():
    from mmnas_amd import _lib as L
    from mmnas_amd.optim import FlatSGD
    ps = [torch.nn.Parameter(torch.zeros(5))]
    with pytest.raises(L.MMNasHipError, match='MI355X only'):
        FlatSGD(ps, lr=0.1, momentum=0.9)
    with pytest.raises(ValueError, match='absent_grads'):
        FlatSGD(ps, absent_grads='drop')
    with pytest.raises(ValueError, match='Nesterov'):
        FlatSGD(ps, nesterov=True)


def test_library_exports_the_sgd_entries():
    from mmnas_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in ('mmnas_sgd_step', 'mmnas_alpha_full_step_wd'):
        assert hasattr(raw, name) and name in L.SYMBOLS, name
    assert L.lib().mmnas_abi_version() == 1
    # host-side argument handling: n == 0 is a no-op whatever the pointers; a momentum step without its buffer is refused
    sgd = L.lib().mmnas_sgd_step
    assert sgd(None, None, None, 0, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, None) == 0
    one = ctypes.c_void_p(16)
    assert sgd(one, one, None, 4, 0.1, 0.9, 0.0, 0.0, 0, 0, None, 0.0, None) != 0
    assert b'buf' in L.lib().mmnas_last_error()
    assert sgd(one, one, one, 4, 0.1, 0.9, 0.1, 0.0, 1, 0, None, 0.0, None) != 0          # nesterov with dampening
    assert b'nesterov' in L.lib().mmnas_last_error()


def test_sgd_golden_key_layout():
    npz = load('traj_sgd.npz')
    ref = load('traj.npz')
    assert len(SGD_WEIGHT_PLANS) == 4
    for k in ('traj|losses', 'traj|grad_norms', 'traj|lr', 'traj|arch|gate_grads', 'traj|arch|prob_grads', 'traj|arch|alpha_after'):
        assert k in npz.files, k
        assert npz[k].dtype == ref[k].dtype and npz[k].shape[1:] == ref[k].shape[1:], k
    assert npz['traj|losses'].shape == (5,)                       # w1, w2, w3, arch, the closing forward
    assert npz['traj|grad_norms'].shape == (3,) and npz['traj|lr'].shape == (3,)          # one per optimizer step
    # the recorded rates are the schedule's: one step before w1 / w2, a second before w3
    H = SGD_HYPER
    want = [H['net_lr_min'] + (H['net_lr'] - H['net_lr_min']) * (1 + np.cos(np.pi * t / H['max_epoch'])) / 2 for t in (1, 1, 2)]
    assert np.allclose(npz['traj|lr'], want, rtol=1e-12, atol=0)
    for i in range(4):
        assert np.array_equal(npz['traj|plan%d' % i], ref['traj|plan%d' % i])              # traj_setup()'s injected samples
    for tag in ('w1', 'w2', 'w3', 'a'):
        keys = [str(k) for k in npz['traj|%s|keys' % tag]]
        assert keys == [str(k) for k in ref['traj|w1|keys']]
        assert npz['traj|%s|delta_norm' % tag].shape == (len(keys),)
        off = npz['traj|%s|delta_off' % tag]
        assert off.shape == (len(keys) + 1,) and off[-1] == npz['traj|%s|delta_sample' % tag].size
        for k in cases.TRAJ_FULL_KEYS:
            assert npz['traj|%s|P:%s' % (tag, k)].shape == ref['traj|w1|P:%s' % k].shape
    # the extra keys are exactly the third weight snapshot (traj|lr exists in traj.npz too, there as the warm-up rates)
    assert set(npz.files) - set(ref.files) == {k.replace('|w1|', '|w3|') for k in ref.files if '|w1|' in k}
    assert set(ref.files) <= set(npz.files)
    # weight decay reaches the unsampled candidates: no tensor stands still (in traj.npz they move on Adam's momentum only)
    assert float(npz['traj|w1|delta_norm'].min()) > 0
