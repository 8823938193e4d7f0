"""Every registry operator (all 41 names), forward + backward through the module API, against the FLOAT64 oracle over the
WHOLE of every output (out, dx, dy, drel, every parameter gradient) at the lengths where the kernels behind it change.
The matrix, the input conditioning (no ReLU input within rounding of zero, so that an entry-wise bar is meaningful) and
the judge live in tests/registry_shapes.py; tests/test_registry_shapes_host.py checks on the CPU that the oracle's own
fp32 run sits a factor ten inside the bars used here.

The bar: err = |got - ref64| / max(max|ref64|, 1e-4 s) <= TOL = 1e-3 on every element (s: the operator's largest gradient
entry, 1 for `out`); 3e-3 on the relation-path keys (util.is_rel_path) and drel, the project's bar for them
(test_ops_gpu.py::test_rel_self_att_with_lazy_handle).  B = 3 everywhere: cases.masks leaves sample 0 unpadded, gives
sample 1 a ragged tail and pads sample 2 fully (uniform attention).

What each attention row is meant to reach (read from mmnas_mha_core_fwd / _bwd, launch_fwd / launch_bwd of
csrc/attention.hip and the range checks of csrc/attention_bwd16.hip).  At HSIZE = 256 the bases 256 / 128 / 64 / 32 / 16
give 1 / 2 / 4 / 8 / 16 heads with d_h = base (`_64_2`: inner width 512, 8 heads of 64); DHC is 64 for d_h >= 64 (d_h =
128 / 256 run 2 / 4 head-dim chunks and, in the general backward, mha_delta_kernel first), else d_h.  Self forms (self_att,
rel_self_att) have Sk = Sx keys, guided_att Sk = Sy, uniimg_att Sk = Sx + Sy.  "general backward" = mha_bwd_q_kernel<DHC,
min(NKC, 2), NW> + mha_bwd_kv_kernel; "fused" = mha_bwd_fused_kernel<NKB, bias> (d_h = 64, <= 128 queries and keys);
"bf16 cores" = mha_fwd_b16_kernel + mha_bwd_b16_kernel (d_h = 64, 65..128 keys, <= 128 queries).  rel_self_att_* adds the
score bias (biasT / dbiasT) and the relation kernels (relfused.hip) to its self_att_* row.

  (40, 14)   2-wave query groups.  self forms, 40 keys (2 key chunks): mha_fwd_kernel<DHC,2,2>; d_h = 64: fused<2,.>; others:
             bwd_q<DHC,2,2> + bwd_kv<DHC,2,1>.  guided, 14 keys: fwd<DHC,1,2>; fused<1,false> / bwd_q<DHC,1,2> +
             bwd_kv<DHC,1,4>.  uniimg, 54 keys: as the self forms.
  (100, 14)  the image stream, 4-wave groups.  self forms, 100 keys: d_h = 64 the bf16 cores; every other base
             fwd<DHC,4,4> + bwd_q<DHC,2,4> (two key blocks) + bwd_kv<DHC,4,1>.  guided, 14 keys: fwd<DHC,1,4>; fused<1,false>
             / bwd_q<DHC,1,4> + bwd_kv<DHC,1,4>.  uniimg, 114 keys: as the self forms.
  (14, 100)  the language stream, one-wave groups.  self forms, 14 keys: fwd<DHC,1,1>; fused<1,.> / bwd_q<DHC,1,1> +
             bwd_kv<DHC,1,1>; self_att_64 alone runs the short-sequence kernels (small.hip: sa_small_fwd / sa_small_bwd).
             guided, 100 keys from 14 queries: d_h = 64 the bf16 cores; others fwd<DHC,4,1> + bwd_q<DHC,2,1> + bwd_kv<DHC,4,1>.
             uniimg, 114 keys: as guided.
  (130, 70)  two query blocks of 128 (more than 128 queries: no fused / bf16 core for any base).  self forms, 130 keys (5
             key chunks): fwd<DHC,8,4>, bwd_q<DHC,2,4> with its key-block loop (3 blocks), bwd_kv<DHC,4,1> (2 key blocks).
             guided, 70 keys: fwd<DHC,4,4> + bwd_q<DHC,2,4> + bwd_kv<DHC,4,1>.  uniimg, 200 keys: fwd<DHC,8,4>, the same backward.
  (20, 250)  self forms, 20 keys: the smallest instantiations (fwd<DHC,1,1>).  guided, 250 keys: the one-shot forward's last
             instantiation fwd<DHC,8,1>; bwd_q<DHC,2,1> over 4 key blocks + bwd_kv<DHC,4,1>.  uniimg, 270 keys: the
             streaming forward mha_fwd_stream_kernel<32,1,1> / <64,1,1> / <64,2,2>; the general backward.
  HSIZE = 512, (100, 14): rel_self_att_16 -- 32 heads of 16, fwd<16,4,4> with bias and the relation kernels' full head tile
             (RF_HP = 32); self_att_16 -- the same cores without bias; self_att_64_2 -- inner width 1024, 16 heads on the
             bf16 cores, products with K = 1024; guided_att_64_2 -- 16 heads, fwd<64,1,4> + fused<1,false>.

test_rows_reach_their_kernel_classes asserts, from the library's launch counters, that the rows run the attention /
relation / short-sequence kernel classes at all (a silent re-route would make a row vacuous).

When MMNAS_REGISTRY_STATS names a file the worst error per (family, key kind) is written there at the end of the module
(profiles/r12_registry_shapes_error_stats.json is one such run)."""
import json
import os

import pytest
import torch

from tests import registry_shapes as RS
from tests.test_ops_gpu import run_hip_op

pytestmark = pytest.mark.gpu

ERR = {}     # 'family|key kind' -> {'worst': float, 'case': id, 'key': name, 'bar': float}


@pytest.fixture(scope='module', autouse=True)
def _write_error_stats():
    yield
    path = os.environ.get('MMNAS_REGISTRY_STATS')
    if ERR and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(ERR, f, indent=1, sort_keys=True)


def _record(spec, errs):
    for k, e in errs.items():
        tag = '%s|%s' % (RS.family(spec.name), RS.key_kind(k))
        if tag not in ERR or e > ERR[tag]['worst']:
            ERR[tag] = {'worst': e, 'case': RS.spec_id(spec), 'key': k, 'bar': RS.key_tol(k)}


def _check(spec, got, ref):
    errs = RS.judge(got, ref)
    _record(spec, errs)
    bad = {k: e for k, e in errs.items() if not e <= RS.key_tol(k)}
    assert not bad, (RS.spec_id(spec), bad)


@pytest.mark.parametrize('spec', [s for s in RS.MATRIX if not s.drop], ids=RS.spec_id)
def test_registry_op_vs_float64_oracle(spec, monkeypatch):
    direct = []
    if spec.form:
        from mmnas_amd import ops
        monkeypatch.setenv('MMNAS_CONV_IM2COL', '0' if spec.form == 'direct' else '1')
        orig = ops.ConvSeqFn.apply
        monkeypatch.setattr(ops.ConvSeqFn, 'apply', lambda *a: (direct.append(1), orig(*a))[1])
    case = RS.build_case(spec)
    got = run_hip_op(case)
    _check(spec, got, RS.oracle(case))
    if spec.form:          # the product really ran in the form asked for
        assert len(direct) == (1 if spec.form == 'direct' else 0)


@pytest.mark.parametrize('spec', [s for s in RS.MATRIX if s.drop], ids=RS.spec_id)
def test_dropout_replay_vs_float64_oracle(spec, monkeypatch):
    """Training mode at p = 0.1 with the seed pinned: the oracle multiplies by the masks the kernels derive from
    (seed, site, index)."""
    from mmnas_amd import ops
    monkeypatch.setattr(ops, 'next_seed', lambda: RS.DROP_SEED)
    case = RS.build_case(spec)
    got = run_hip_op(case, train=True, drop_p=RS.DROP_P)
    ref = RS.oracle(case)
    _check(spec, got, ref)
    ref0 = RS.R.run_oracle_op(case, dtype=torch.float64)        # the masks actually dropped something
    assert RS.judge({'out': got['out']}, {'out': ref0['out']})['out'] > 1e-2


REACH = [(sx, sy, d, name) for sx, sy in RS.ATT_SHAPES
         for d, name in ((256, 'self_att_64'), (256, 'rel_self_att_32'), (256, 'guided_att_128'), (256, 'uniimg_att_64'))]
REACH += [(100, 14, 512, name) for name in RS.ATT_WIDE]


@pytest.mark.parametrize('sx,sy,d,name', REACH)
def test_rows_reach_their_kernel_classes(sx, sy, d, name):
    from mmnas_amd import _lib as L
    lib = L.lib()
    case = RS.build_case(RS.Spec(name, sx, sy, d, RS.NR, None, False))
    arr = (L.ProfStat * len(L.K_NAMES))()
    L.check(lib.mmnas_prof_enable(1))
    try:
        run_hip_op(case)
        torch.cuda.synchronize()
        L.check(lib.mmnas_prof_collect(arr))
    finally:
        L.check(lib.mmnas_prof_enable(0))
    n = {k: arr[i].launches for i, k in enumerate(L.K_NAMES)}
    short = name == 'self_att_64' and sx == 14       # the short-sequence kernels take the whole operator
    assert (n['small_ops'] > 0) == short, n
    if not short:
        assert n['mha_fwd'] > 0 and n['mha_bwd'] > 0, n
    assert (n['rel_fwd'] > 0 and n['rel_bwd'] > 0) == name.startswith('rel_self_att'), n
