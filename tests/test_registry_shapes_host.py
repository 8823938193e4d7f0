"""The preconditions of tests/test_registry_shapes_gpu.py, checked without a GPU for every case of its matrix
(tests/registry_shapes.py):
  (a) after the input conditioning a float64 oracle run records no ReLU input within 1e-5 of zero (relative to the
      largest pre-activation of its layer);
  (b) the oracle's own fp32 run is within 1e-4 of its float64 run under the GPU test's judge (3e-4 on the relation-path
      keys and drel) -- a tenth of the bars the kernels are held to, so those bars are statements about the kernels;
  (c) the matrix covers every registry name, every shape row and both norm / residual settings."""
import numpy as np
import pytest
import torch

from oracle import mmnas_oracle as O
from tests import registry_shapes as RS


@pytest.mark.parametrize('spec', [s for s in RS.MATRIX if s.form != 'im2col'], ids=RS.spec_id)   # (the two forms share one case)
def test_oracle_is_a_yardstick_for_the_case(spec):
    case = RS.build_case(spec)
    assert RS.count_suspects(case, case['_drops']) == 0
    assert case['x'].dtype == np.float32 and case['x'].shape == (RS.B, spec.Sx, spec.HSIZE)
    ref = RS.oracle(case, torch.float64)
    errs = RS.judge(RS.oracle(case, torch.float32), ref)
    for k, e in errs.items():
        assert e <= RS.key_tol(k, 1e-4, 3e-4), (k, e)
    if spec.drop:      # the replayed masks drop something
        p0 = RS.R.run_oracle_op(case, dtype=torch.float64)
        assert RS.judge({'out': ref['out']}, {'out': p0['out']})['out'] > 1e-2


def test_conditioning_moves_the_inputs_by_a_rounding_sized_step():
    """feed_forward at 390 rows has suspects before conditioning and none after; the inputs move by ~1e-4 of their scale
    and only in the rows that held a suspect."""
    spec = RS.Spec('feed_forward', 130, 5, 256, RS.NR, None, False)
    seed_case = RS.build_case(spec)
    raw = RS.raw_case(spec)
    n_raw = RS.count_suspects(raw)
    assert n_raw > 0 and seed_case['_rounds'] > 0
    moved = np.abs(seed_case['x'] - raw['x']).max(-1).reshape(-1)
    assert 0 < int((moved > 0).sum()) <= n_raw
    assert moved.max() <= 1e-3 * np.abs(raw['x']).max()


def test_judge_sees_one_wrong_element():
    """The judge is entry-wise: one element of the last row off by 2e-3 of the tensor's largest entry fails TOL, whichever
    tensor it is in; a gradient that is zero in the reference is measured against the operator's gradient scale."""
    spec = RS.Spec('guided_att_32', 40, 14, 256, RS.NR, None, False)
    ref = RS.oracle(RS.build_case(spec))
    assert max(RS.judge(ref, ref).values()) == 0.0
    for k in ref:
        got = {n: v.copy() for n, v in ref.items()}
        got[k].reshape(-1)[-1] += 2e-3 * np.abs(ref[k]).max()
        errs = RS.judge(got, ref)
        assert errs[k] > RS.TOL and all(e == 0.0 for n, e in errs.items() if n != k), k
    zero = dict(ref, dy=np.zeros_like(ref['dy']))
    gscale = max(np.abs(v).max() for n, v in zero.items() if n != 'out')
    got = dict(zero, dy=np.full_like(ref['dy'], 1e-7 * gscale))
    assert RS.judge(got, zero)['dy'] == pytest.approx(1e-3, rel=1e-3)


def test_matrix_covers_the_registry():
    names = {s.name for s in RS.MATRIX}
    assert names == set(O.ALL_OP_NAMES) and len(names) == 41
    assert set(RS.ELEMENTWISE + RS.ATTENTION + RS.CONVS + RS.MLPS) == names
    assert (len(RS.ELEMENTWISE), len(RS.ATTENTION), len(RS.CONVS), len(RS.MLPS)) == (5, 20, 8, 8)
    have = {(s.name, s.Sx, s.Sy, s.HSIZE, s.nr, s.form) for s in RS.MATRIX if not s.drop}
    for n in RS.ATTENTION:
        for sx, sy in RS.ATT_SHAPES:
            assert (n, sx, sy, 256, RS.NR, None) in have
        assert (n,) + RS.ATT_SHAPES[1] + (256, RS.PLAIN, None) in have
    for n in RS.ATT_WIDE:
        assert (n, 100, 14, 512, RS.NR, None) in have
    for n in RS.CONVS:
        for d in RS.CONV_HSIZE:
            for sx in RS.CONV_SX:
                forms = ('direct', 'im2col') if n.startswith('std_conv') and sx in RS.CONV_FORMS_SX else (None,)
                assert all((n, sx, 5, d, RS.NR, f) in have for f in forms)
            assert (n, RS.CONV_SX[1], 5, d, RS.PLAIN, None) in have
    for n in RS.MLPS + RS.ELEMENTWISE:
        for sx in (RS.ROW_SX_WIDE_FFN if n in ('feed_forward_16', 'feed_forward_32') else RS.ROW_SX):
            assert (n, sx, 5, 256, RS.NR, None) in have
        assert (n, RS.ROW_SX[1], 5, 256, RS.PLAIN, None) in have
    assert [s.name for s in RS.MATRIX if s.drop] == RS.DROP_NAMES
    assert all(s.Sx == 100 and s.Sy == 14 for s in RS.MATRIX if s.drop)
    assert len({RS.spec_id(s) for s in RS.MATRIX}) == len(RS.MATRIX)
