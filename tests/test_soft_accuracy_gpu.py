"""mmnas_vqa_soft_accuracy on the GPU against numpy: B in {1, 3, 64} x A in {1, 2, 63, 64, 65, 3129} (one lane, a partial wave,
one column short of / at / past a full wave, the VQA vocabulary), rows strided (ld > A) inside guard bands, ties at the first,
a middle and the last index, +-inf; per_row bitwise, the mean within one float32 ulp of the float64 mean; the NaN flag set by
one NaN logit and by nothing else; the reward path returns a device tensor without reading anything back."""
import numpy as np
import pytest
import torch

from tests.guardband import Arena
from tests.test_soft_accuracy_host import loop_reference, make_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy
SHAPES = [(B, A) for B in (1, 3, 64) for A in (1, 2, 63, 64, 65, 3129)]


def _numpy(x, t):
    rows = t[np.arange(x.shape[0]), np.argmax(x, axis=1)]
    return rows, float(rows.astype(np.float64).sum() / x.shape[0])


def _launch(x, t, ld, ldt, per_row=True):
    from mmnas_amd import _lib as L
    B, A = x.shape
    ar = Arena(DEV, capacity=8 << 20)
    xl = ar.inp(x, ld=ld, name='logits')[0]
    tl = ar.inp(t, ld=ldt, name='target')[0]
    rows = ar.out(B, name='per_row')[1] if per_row else None
    out = ar.out(1, name='out')[1]
    flag = ar.inout(np.zeros(1, np.int32), name='nan_flag')[1]
    L.check(L.lib().mmnas_vqa_soft_accuracy(xl.data_ptr(), ld, tl.data_ptr(), ldt, B, A, L.ptr(rows), L.ptr(out), L.ptr(flag), L.stream()))
    ar.check()
    return rows, out, int(flag)


@pytest.mark.parametrize('B,A', SHAPES, ids=str)
def test_kernel_against_numpy_with_strided_rows(B, A):
    x, t = make_case(B, A, 100 * B + A)
    want_rows, want_mean = _numpy(x, t)
    if A <= 65:
        loop_rows, loop_mean = loop_reference(x, t)
        assert np.array_equal(loop_rows, want_rows) and loop_mean == want_mean
    rows, out, flag = _launch(x, t, A + 3, A + 1)
    assert flag == 0 and np.array_equal(rows.cpu().numpy(), want_rows)
    ulp = float(np.spacing(np.float32(abs(want_mean))))
    got = float(out.cpu()[0])
    print('B %d A %d mean %.9g float64 %.17g (%.2f ulp)' % (B, A, got, want_mean, abs(got - want_mean) / ulp))
    assert abs(got - want_mean) <= ulp
    rows2, out2, _ = _launch(x, t, A, A, per_row=False)                 # dense rows, no per_row: the same bits
    assert rows2 is None and torch.equal(out, out2)


@pytest.mark.parametrize('B,A,b,a', [(1, 1, 0, 0), (3, 65, 2, 64), (64, 3129, 63, 3128), (64, 3129, 17, 0), (3, 2, 1, 1)], ids=str)
def test_nan_flag_is_set_by_one_nan_logit_and_by_nothing_else(B, A, b, a):
    x, t = make_case(B, A, 7)
    x[:, A // 2] = np.inf if B > 1 else x[:, A // 2]                    # infinities are ordinary values
    assert _launch(x, t, A + 2, A)[2] == 0
    x[b, a] = np.nan
    rows, out, flag = _launch(x, t, A + 2, A)
    assert flag == 1
    keep = np.arange(B) != b                                              # the other rows are what they were
    assert np.array_equal(rows.cpu().numpy()[keep], _numpy(np.nan_to_num(x, nan=0.0), t)[0][keep])
    assert float(rows[b]) == float(t[b, a])                              # np.argmax: the first NaN wins


def test_functional_and_reward_paths_stay_on_the_device():
    from mmnas_amd import answering
    x, t = make_case(64, 3129, 3)
    want_rows, want_mean = _numpy(x, t)
    xd, td = T(x).to(DEV), T(t).to(DEV)
    r = answering.SoftAccuracyReward()(xd, td)
    f = answering.soft_accuracy(xd, td, check=False)
    assert isinstance(r, torch.Tensor) and r.is_cuda and r.dim() == 0 and r.dtype == torch.float32 and torch.equal(r, f)
    mean, rows = answering.soft_accuracy(xd, td, per_row=True)
    assert rows.is_cuda and np.array_equal(rows.cpu().numpy(), want_rows)
    assert abs(float(mean) - want_mean) <= float(np.spacing(np.float32(want_mean)))
    # a slice of a wider block goes to the kernel with its stride
    wide = torch.full((64, 3200), 99.0, device=DEV)
    wide[:, :3129] = xd
    assert torch.equal(answering.soft_accuracy(wide[:, :3129], td, check=False), f)
    # the reward feeds a quality buffer device to device
    quality = torch.zeros(4, device=DEV)
    quality[2].copy_(r)
    assert float(quality[2]) == float(r)
    xd[5, 77] = float('nan')
    with pytest.raises(answering.AnsweringError, match='NaN'):
        answering.soft_accuracy(xd, td)
    answering.soft_accuracy(xd, td, check=False)                          # never reads the flag
