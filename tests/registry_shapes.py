"""The registry-shape matrix shared by tests/test_registry_shapes_gpu.py and tests/test_registry_shapes_host.py: the case
list, the input conditioning that keeps every ReLU pre-activation away from zero, and the entry-wise judge.

A case is a `Spec`; `build_case(spec)` rebuilds it deterministically (seeded inputs from tests/golden/cases.op_case, then
`condition`), so no arrays are stored anywhere.

ReLU kinks.  An entry-wise bar against a float64 reference only means something if no ReLU input sits within rounding of
zero: about 4e-5 of all pre-activations satisfy |z| <= 1e-5 max|z|, and one gate that falls on different sides in two
precisions moves a weight-gradient entry by up to 1e-1 of the tensor's scale (the oracle's own fp32 run does this in
feed_forward_16 at 300 rows and feed_forward_deep at 300 and 390 rows).  `condition` therefore nudges the inputs: every
suspect pre-activation z_s (|z_s| <= KINK_SUSPECT max|z|) of input row i is moved to |z_s| = KINK_TARGET max|z| by shifting
x_i along dz_s/dx_i (float64 autograd; every operator concerned acts on rows independently), and the run is repeated until
it records no suspect.  The shifts are ~1e-4 of the input scale.  The relation bias log(clamp(relu(.), 1e-6)) is not
conditioned: its keys keep the project's 3e-3 bar (tests/test_ops_gpu.py::test_rel_self_att_with_lazy_handle).
"""
import collections
import functools
import zlib

import numpy as np
import torch

from oracle import mmnas_oracle as O
from tests import oracle_runner as R
from tests.golden import cases
from tests.util import TOL, is_rel_path

B = 3   # cases.masks: sample 0 unpadded, sample 1 a ragged tail, sample 2 fully padded (uniform attention)

# name, Sx, Sy, HSIZE, (norm, residual), conv product form (None | 'direct' | 'im2col'), dropout replay
Spec = collections.namedtuple('Spec', 'name Sx Sy HSIZE nr form drop')

ELEMENTWISE = [n for n in O.ALL_OP_NAMES if O.parse_op_name(n)[0] in ('zero', 'identity', 'relu', 'gelu', 'leakyrelu')]
ATTENTION = [n for n in O.ALL_OP_NAMES if O.parse_op_name(n)[0] in ('self_att', 'rel_self_att', 'guided_att', 'uniimg_att')]
CONVS = [n for n in O.ALL_OP_NAMES if O.parse_op_name(n)[0] in ('sep_conv', 'std_conv')]
MLPS = [n for n in O.ALL_OP_NAMES if O.parse_op_name(n)[0] in ('ffn', 'ffn_deep', 'glu')]

ATT_SHAPES = [(40, 14), (100, 14), (14, 100), (130, 70), (20, 250)]     # (Sx, Sy) at HSIZE = 256
ATT_WIDE = ['rel_self_att_16', 'self_att_16', 'self_att_64_2', 'guided_att_64_2']   # HSIZE = 512 at (100, 14)
CONV_SX = [1, 4, 14, 100, 130]
CONV_HSIZE = [256, 96]
CONV_FORMS_SX = [14, 100]        # the wide (std_conv) kernels run in both product forms here
ROW_SX = [1, 14, 100, 130]       # MLP / GLU / element-wise at HSIZE = 256: 3, 42, 300 and 390 rows
ROW_SX_WIDE_FFN = [1, 14, 100]   # feed_forward_16 / _32
DROP_NAMES = ['self_att_16', 'rel_self_att_128', 'guided_att_64_2', 'uniimg_att_32', 'feed_forward_8', 'feed_forward_deep',
              'gated_linear_2', 'sep_conv_11', 'std_conv_11']
DROP_SEED, DROP_P = 0x0BADC0DE12345678, 0.1
NR, PLAIN = (True, True), (False, False)

KINK_SUSPECT = 1e-5
KINK_TARGET = 4e-5
KINK_ROUNDS = 50
REL_TOL = 3e-3                   # relation-path keys and drel


def _matrix():
    m = []
    for name in ATTENTION:
        for i, (sx, sy) in enumerate(ATT_SHAPES):
            m.append(Spec(name, sx, sy, 256, NR, None, False))
            if i == 1:
                m.append(Spec(name, sx, sy, 256, PLAIN, None, False))
    m += [Spec(name, 100, 14, 512, NR, None, False) for name in ATT_WIDE]
    for name in CONVS:
        for d in CONV_HSIZE:
            for i, sx in enumerate(CONV_SX):
                if name.startswith('std_conv') and sx in CONV_FORMS_SX:
                    m += [Spec(name, sx, 5, d, NR, form, False) for form in ('direct', 'im2col')]
                else:
                    m.append(Spec(name, sx, 5, d, NR, None, False))
                if i == 1:
                    m.append(Spec(name, sx, 5, d, PLAIN, None, False))
    for name in MLPS + ELEMENTWISE:
        for i, sx in enumerate(ROW_SX_WIDE_FFN if name in ('feed_forward_16', 'feed_forward_32') else ROW_SX):
            m.append(Spec(name, sx, 5, 256, NR, None, False))
            if i == 1:
                m.append(Spec(name, sx, 5, 256, PLAIN, None, False))
    m += [Spec(name, 100, 14, 256, NR, None, True) for name in DROP_NAMES]
    return m


MATRIX = _matrix()


def spec_id(s):
    return '%s-%dx%d-%d-%d%d%s%s' % (s.name, s.Sx, s.Sy, s.HSIZE, int(s.nr[0]), int(s.nr[1]), '-' + s.form if s.form else '',
                                     '-drop' if s.drop else '')


def family(name):
    kind = O.parse_op_name(name)[0]
    if kind in ('sep_conv', 'std_conv'):
        return 'conv'
    if kind in ('ffn', 'ffn_deep', 'glu'):
        return 'mlp'
    if kind in ('self_att', 'rel_self_att', 'guided_att', 'uniimg_att'):
        return kind
    return 'elementwise'


def key_kind(key):
    if key in ('out', 'dx', 'dy', 'drel'):
        return key
    return 'g:rel_path' if is_rel_path(key) else 'g:ln' if key.startswith('g:ln.') else 'g:bias' if key.endswith('bias') else 'g:weight'


def key_tol(key, tol=TOL, rel_tol=REL_TOL):
    return rel_tol if key == 'drel' or is_rel_path(key) else tol


def drop_sites(case):
    from tests.test_ops_gpu import _drop_sites
    return _drop_sites(case, DROP_SEED, DROP_P)


def conditioned(name):
    """Operators whose oracle path applies a ReLU to something computed from x alone, row by row."""
    kind, kw = O.parse_op_name(name)
    return kind in ('ffn', 'ffn_deep', 'relu') or (kind == 'glu' and kw['layers'] == 2)


def relu_inputs(case, drops=None):
    """One float64 oracle forward with torch.relu recorded: (x, [pre-activation tensors, still attached to x])."""
    seen = []
    relu = torch.relu

    def recording(t):
        seen.append(t)
        return relu(t)

    T, cfg = torch.from_numpy, case['cfg']
    P = {k: T(v).double() for k, v in case['P'].items()}
    x = T(case['x']).double().requires_grad_(True)
    if drops is not None:
        drops = {k: T(np.ascontiguousarray(v)).double() for k, v in drops.items() if v is not None}
    torch.relu = recording
    try:
        O.op_forward(case['name'], P, cfg, x, T(case['y']).double(), T(case['x_mask']), T(case['y_mask']), T(case['rel']).double(),
                     norm=cfg.OPS_NORM, residual=cfg.OPS_RESIDUAL, drops=drops)
    finally:
        torch.relu = relu
    return x, seen


def suspects(case, drops=None):
    """[(pre-activation tensor, its max |z|, flat indices of the entries with |z| <= KINK_SUSPECT max|z|)], and x."""
    x, seen = relu_inputs(case, drops)
    if not conditioned(case['name']):      # (the relation bias's ReLU is not conditioned: module docstring)
        seen = []
    found = []
    for z in seen:
        top = float(z.detach().abs().max())
        idx = torch.nonzero(z.detach().abs().reshape(-1) <= KINK_SUSPECT * top).reshape(-1)
        found.append((z, top, idx))
    return x, found


def count_suspects(case, drops=None):
    return sum(int(idx.numel()) for _, _, idx in suspects(case, drops)[1])


def condition(case, drops=None):
    """Nudge case['x'] (in place of the array: a new float32 array is stored) until no ReLU input of the float64 oracle run
    is a suspect.  Returns the number of rounds that moved something."""
    if not conditioned(case['name']):
        return 0
    d = case['x'].shape[-1]
    for rnd in range(KINK_ROUNDS + 1):
        x, found = suspects(case, drops)
        if not any(idx.numel() for _, _, idx in found):
            return rnd
        assert rnd < KINK_ROUNDS, 'input conditioning of %s did not settle in %d rounds' % (case['name'], KINK_ROUNDS)
        step = torch.zeros_like(x).reshape(-1, d)
        for z, top, idx in found:
            width = z.shape[-1]
            zf = z.reshape(-1)
            for j in idx.tolist():
                row = j // width                               # z is [B, Sx, width]: its row is x's row
                g = torch.autograd.grad(zf[j], x, retain_graph=True)[0].reshape(-1, d)[row]
                zs = float(zf[j].detach())
                want = (KINK_TARGET * top) * (1.0 if zs >= 0 else -1.0)
                step[row] += g * ((want - zs) / float(g.dot(g)))
        case['x'] = (x.detach() + step.reshape(x.shape)).float().numpy()
    raise AssertionError('unreachable')


def raw_case(spec):
    """The seeded inputs before conditioning (the two product forms of a convolution share one case)."""
    seed = 120000 + zlib.crc32(spec_id(spec._replace(form=None)).encode()) % 100000
    return cases.op_case(spec.name, spec.nr[0], spec.nr[1], seed, dict(B=B, Sx=spec.Sx, Sy=spec.Sy, HSIZE=spec.HSIZE))


@functools.lru_cache(maxsize=4)
def build_case(spec):
    """The conditioned case of one row of the matrix (its dropout multipliers under '_drops' for a replay case)."""
    case = raw_case(spec)
    case['_drops'] = drop_sites(case) if spec.drop else None
    case['_rounds'] = condition(case, case['_drops'])
    return case


def oracle(case, dtype=torch.float64):
    case['cfg'].DROPOUT_R = 0.0
    return R.run_oracle_op(case, drops=case['_drops'], dtype=dtype)


def judge(got, ref):
    """key -> max over ALL elements of |got - ref| / max(max|ref|, 1e-4 s), s = the operator's largest gradient entry (1 for
    'out'): the floor tests/test_ops_gpu.py::test_full_size_vs_oracle uses for gradients that are mathematically zero."""
    gscale = max([float(np.abs(ref[k]).max()) for k in ref if k != 'out' and ref[k].size] or [0.0])
    errs = {}
    for k in ref:
        a, b = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        assert a.shape == b.shape, (k, a.shape, b.shape)
        assert np.isfinite(a).all(), k
        den = max(float(np.abs(b).max()) if b.size else 0.0, 1e-4 * (gscale if k != 'out' else 1.0))
        num = float(np.abs(a - b).max()) if b.size else 0.0
        errs[k] = num / den if den > 0 else num
    for k in got:                      # an output the reference does not have (an unused input's gradient) is zero
        if k not in ref:
            assert not np.any(got[k]), k
    return errs
