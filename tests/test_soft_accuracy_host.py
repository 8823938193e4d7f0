"""answering.soft_accuracy on CPU tensors (the numpy restatement the kernel is checked against) against a plain loop: ties,
infinities, strided rows, the NaN flag; and the C entry's argument checks, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

T = torch.from_numpy


def loop_reference(x, t):
    """target[b, argmax_a x[b, a]] with the argmax written out: the lowest index of the maximum, infinities ordinary."""
    rows = []
    for b in range(x.shape[0]):
        best = 0
        for a in range(1, x.shape[1]):
            if x[b, a] > x[b, best]:
                best = a
        rows.append(t[b, best])
    rows = np.array(rows, np.float32)
    return rows, float(np.sum(rows.astype(np.float64)) / len(rows))


def make_case(B, A, seed):
    """Logits with the edge rows the argmax rule is about (where A allows): ties at the first, a middle and the last index,
    +inf twice, -inf everywhere, -inf but one."""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((B, A)).astype(np.float32)
    t = rs.choice(np.array([0.0, 0.3, 0.6, 0.9, 1.0], np.float32), size=(B, A))
    t[:, 0] = 1.0 - t[:, A - 1] if A > 1 else t[:, 0]              # (first and last differ: a wrong tie rule shows)
    top = np.float32(9.0)
    edges = [lambda r: (r.__setitem__(0, top), r.__setitem__(A - 1, top)),
             lambda r: (r.__setitem__(A // 2, top), r.__setitem__(A - 1, top)),
             lambda r: r.__setitem__(A - 1, top),
             lambda r: (r.__setitem__(A // 3, np.inf), r.__setitem__(A - 1, np.inf)),
             lambda r: r.fill(-np.inf),
             lambda r: (r.fill(-np.inf), r.__setitem__(A - 1, -1e30))]
    for b in range(B):
        if b < len(edges) or b % 7 == 0:
            edges[b % len(edges)](x[b])
    return x, t


@pytest.mark.parametrize('B,A', [(1, 1), (1, 7), (3, 2), (6, 65), (64, 130)], ids=str)
def test_restatement_against_a_plain_loop(B, A):
    from mmnas_amd import answering
    x, t = make_case(B, A, 10 * B + A)
    rows, mean = loop_reference(x, t)
    got, got_rows = answering.soft_accuracy(T(x), T(t), per_row=True)
    assert got.dim() == 0 and got.dtype == torch.float32 and np.array_equal(got_rows.numpy(), rows)
    assert float(got) == float(np.float32(mean))
    assert float(answering.soft_accuracy(T(x), T(t))) == float(got)
    # strided rows: a slice of a wider block
    wide_x, wide_t = np.full((B, A + 5), 50.0, np.float32), np.full((B, A + 3), 0.5, np.float32)
    wide_x[:, :A], wide_t[:, :A] = x, t
    got2, rows2 = answering.soft_accuracy(T(wide_x)[:, :A], T(wide_t)[:, :A], per_row=True)
    assert float(got2) == float(got) and np.array_equal(rows2.numpy(), rows)


def test_nan_flag_and_argument_errors():
    from mmnas_amd import answering
    x, t = make_case(5, 9, 1)
    x[3, 4] = np.nan
    with pytest.raises(answering.AnsweringError, match='NaN'):
        answering.soft_accuracy(T(x), T(t))
    x[3, 4] = np.inf
    answering.soft_accuracy(T(x), T(t))
    with pytest.raises(TypeError):
        answering.soft_accuracy(T(x), T(t[:, :8]))
    with pytest.raises(TypeError):
        answering.soft_accuracy(T(x), T(t).double())
    with pytest.raises(ValueError):
        answering.soft_accuracy(T(x[:0]), T(t[:0]))
    r = answering.SoftAccuracyReward()(T(x), T(t))
    assert isinstance(r, torch.Tensor) and r.dim() == 0 and float(r) == float(answering.soft_accuracy(T(x), T(t)))


def test_c_entry_rejects_bad_arguments_before_any_launch():
    from mmnas_amd import _lib as L
    lib = L.lib()
    buf = [(ctypes.c_float * 64)() for _ in range(5)]
    p = [ctypes.cast(b, ctypes.c_void_p).value for b in buf]

    def call(B=2, A=4, ld=4, ldt=4, null=()):
        q = [None if i in null else x for i, x in enumerate(p)]
        return lib.mmnas_vqa_soft_accuracy(q[0], ld, q[1], ldt, B, A, q[2], q[3], q[4], None)

    for kw in (dict(B=0), dict(B=-1), dict(A=0), dict(ld=3), dict(ldt=3)):
        assert call(**kw) == -1 and b'vqa_soft_accuracy' in lib.mmnas_last_error(), kw      # MMNAS_E_SHAPE
    for i in (0, 1, 3, 4):
        assert call(null=(i,)) == -2, i                                                        # MMNAS_E_ARG
    assert not any(any(b) for b in buf)
