"""Live-row weight gradients (mmnas_wgrad_live_table in ops.hip, mmnas_gemm_desc.ktab in gemm.hip, mmnas_set_wgrad_live): on a
padded batch the gradient that enters the image stream of a backbone chain is exactly 0 on the padded rows and stays 0 through
every chain operator, so the weight gradients dW += dY^T X reduce over the 32-row K-tiles that cover the live rows only.

1. the table against a numpy restatement of its rule; 2. TN accumulate products with and without a table, against float64 at
the bound of tests/test_kernels_gpu.py's accumulate products (test_gemm_tn_ragged_reduction_length: 3e-6); 3. a four-operator
chain with the switch off and on; 4. everything inside a tests/guardband.py Arena: bands, inputs and the planned scratch."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import dropout_rng
from oracle import mmnas_oracle as O
from tests.guardband import Arena
from tests.util import TOL, rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ACC_TOL = 3e-6      # accumulate products against float64 (tests/test_kernels_gpu.py)
T64 = lambda a: torch.from_numpy(np.asarray(a)).double()


def _L():
    import mmnas_amd._lib as L
    return L


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


@pytest.fixture
def ar():
    yield Arena(DEV, capacity=192 << 20)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a fault on the device: nothing more is started on it
        pytest.exit('GPU error in a live-row case, the session ends here: %s' % e, returncode=3)


def spread_bound(e_self):
    """How far two evaluations that differ only in the ORDER of their float atomics may lie apart, given what two runs with the
    switch off showed (e_self, normalised to the tensor's largest entry): four times that spread -- one more sample of the same
    distribution -- and, for the case that the two off runs happened to agree bit for bit, eight units of fp32 round-off
    (2^-24 of the largest entry each: a handful of addends of that size rounded in another order)."""
    return max(4.0 * e_self, 8 * 2.0 ** -24)


def live_tags(fn):
    """Run fn with the library's launch profiler on -> fn's result, the tags of its bracketed launches (MMNAS_PROF_DUMP rows).
    A product that walks a live-row table carries ' live' in its tag (plan_gemm: set only where the kernel takes the table)."""
    L = _L()
    lib = L.lib()
    fd, path = tempfile.mkstemp(suffix='.csv')
    os.close(fd)
    old = os.environ.get('MMNAS_PROF_DUMP')
    os.environ['MMNAS_PROF_DUMP'] = path
    L.check(lib.mmnas_prof_enable(1))
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        L.check(lib.mmnas_prof_collect((L.ProfStat * len(L.K_NAMES))()))
        L.check(lib.mmnas_prof_enable(0))
        if old is None:
            del os.environ['MMNAS_PROF_DUMP']
        else:
            os.environ['MMNAS_PROF_DUMP'] = old
        rows = open(path).read().splitlines()
        os.unlink(path)
    return res, [r.split(',')[1] for r in rows if r.count(',') >= 4]


# ---------------------------------------------------------------------------------------------------------------- 1. the table
def cover(live):
    """Greedy cover: the next 32-row tile starts at the first live row not yet covered."""
    tiles, pos = [], 0
    idx = np.flatnonzero(live)
    while True:
        j = idx[idx >= pos]
        if not len(j):
            return tiles
        tiles.append(int(j[0]))
        pos = int(j[0]) + 32


def prefix_mask(lengths, S):
    return np.arange(S)[None, :] >= np.asarray(lengths)[:, None]        # True = padding


def build_table(ar, dy, mask, name='tab'):
    """mmnas_wgrad_live_table on dy [M, d] and mask [M] (bool) -> (device table, count, start rows)."""
    L = _L()
    lib = L.lib()
    M, d = dy.shape
    n = lib.mmnas_wgrad_live_table_ints(M)
    assert n == 2 * ((M + 31) // 32) + 1
    (dyd, _), (md, _) = ar.inp(dy, name=name + '_dy'), ar.inp(mask.astype(np.uint8), name=name + '_mask')
    tabd, tabv = ar.inout(np.full(n, -7, np.int32), name=name)
    L.check(lib.mmnas_wgrad_live_table(L.fptr(dyd), L.ptr(md), M, d, L.ptr(tabd), L.stream()))
    ar.check()
    t = tabv.cpu().numpy()
    return tabd, int(t[0]), t[1:1 + int(t[0])].tolist(), dyd


def masked_zero(rs, mask, d):
    dy = rnd(rs, mask.size, d)
    dy[mask.reshape(-1)] = 0
    return dy


@pytest.mark.parametrize('d', [256, 512, 68])
def test_table_rule_padded_batch(ar, d):
    rs = np.random.RandomState(d)
    mask = prefix_mask((1, 31, 32, 33, 96, 100), 100)
    dy = masked_zero(rs, mask, d)
    _, count, rows, _ = build_table(ar, dy, mask.reshape(-1))
    assert rows == cover(~mask.reshape(-1))
    assert count == 12 and (600 + 31) // 32 == 19 and rows[-1] + 32 > 600        # the last tile runs past M


def test_table_rule_holes_empty_sample_and_no_padding(ar):
    rs = np.random.RandomState(1)
    S = 40
    mask = np.ones((3, S), bool)
    mask[0, [0, 5]] = False                     # valid rows 0 and 5 only; sample 1 has no valid row
    mask[2, :7] = False
    dy = masked_zero(rs, mask, 256)
    _, count, rows, _ = build_table(ar, dy, mask.reshape(-1), 'holes')
    assert rows == cover(~mask.reshape(-1)) == [0, 80] and count == 2
    M = 333                                      # no padding at all: the identity table
    _, count, rows, _ = build_table(ar, rnd(rs, M, 256), np.zeros(M, bool), 'dense')
    assert count == (M + 31) // 32 and rows == list(range(0, M, 32))
    _, count, rows, _ = build_table(ar, np.zeros((M, 256), np.float32), np.ones(M, bool), 'empty')
    assert count == 0 and rows == []


def test_table_rule_masked_rows_are_judged_by_their_values(ar):
    M, d = 200, 512
    mask = np.ones(M, bool)
    dy = np.zeros((M, d), np.float32)
    dy[40] = -0.0                                # only negative zeros: dead
    dy[77, 511] = 1e-30                          # one non-zero entry in the last column: live
    dy[150, 3] = np.nan                          # NaN: live
    dy[199, 260] = -np.inf
    _, count, rows, _ = build_table(ar, dy, mask)
    assert rows == [77, 150, 199] and count == 3
    # an unmasked row is live whatever it holds
    mask[10] = False
    _, count, rows, _ = build_table(ar, dy, mask, 'unmasked')
    assert rows == [10, 77, 150, 199]


@pytest.mark.parametrize('M', [6400, 8192])
def test_table_rule_many_rows(ar, M):
    """More than 4096 rows: the walk's second pair of bit words.  6400 = the benchmark's row count."""
    rs = np.random.RandomState(M)
    S = 100 if M == 6400 else 128
    mask = prefix_mask(rs.randint(1, S + 1, size=M // S), S)
    if M == 8192:
        mask[:] = True
        mask[-1, -1] = False
    dy = masked_zero(rs, mask, 8)
    _, count, rows, _ = build_table(ar, dy, mask.reshape(-1))
    assert rows == cover(~mask.reshape(-1)) and count <= (M + 31) // 32


# ------------------------------------------------------------------------------------------------------------- 2. the products
def tn_product(ar, A, Xs, C0s, tab, tag, pair=False):
    """dW_g = C0_g + A_g^T X_g as one grouped TN accumulate product (pair: behind a data-gradient product, one launch)."""
    from mmnas_amd import ops
    L = _L()
    K, M = A[0].shape
    N = Xs[0].shape[1]
    groups, outs = [], []
    for i, (a, x, c0) in enumerate(zip(A, Xs, C0s)):
        (ad, _), (xd, _) = ar.inp(a, name='%sA%d' % (tag, i)), ar.inp(x, name='%sX%d' % (tag, i))
        cd, cv = ar.inout(c0, name='%sC%d' % (tag, i))
        groups.append(dict(M=M, A=[ad], B=[xd], C=cd))
        outs.append(cv)
    wg = ops.gemm_desc(L.GEMM_TN, groups, N, K, M, N, N, accumulate=True)
    wg.ktab = L.ptr(tab) if tab is not None else None
    if pair:
        W = rnd(np.random.RandomState(3), M, N)
        (wd, _), (dxd, dxv) = ar.inp(W, name=tag + 'W'), ar.out((K, N), name=tag + 'dx')
        dg = ops.gemm_desc(L.GEMM_NN, [dict(M=K, A=[groups[0]['A'][0]], B=[wd], C=dxd)], N, M, M, N, N)
        ops.gemm_pair(dg, wg)
    else:
        L.check(L.lib().mmnas_gemm(C.byref(wg), L.stream()))
    ar.check()
    res = [v.cpu().numpy() for v in outs]
    if pair:
        assert rel_err(dxv.cpu().numpy(), (T64(A[0]) @ T64(W)).numpy()) < 1e-5
    return res


@pytest.mark.parametrize('N,M,ng,pair', [(64, 64, 1, False), (256, 1024, 1, True), (256, 256, 3, True), (512, 512, 1, False),
                                          (256, 1024, 1, False)])
def test_products_walk_the_table(ar, N, M, ng, pair):
    """K = 600 rows of six samples: A = dY is exactly 0 outside the live rows, X is random on all rows.  With the table, without
    it, and with NaN in every X row outside the table's tiles (which a table walk never reads and 0 * NaN would poison): all
    within the accumulate bound of float64.  64 x 64 has a single output tile and stays on the general kernel: dense, equal."""
    rs = np.random.RandomState(N + M + ng)
    mask = prefix_mask((1, 31, 32, 33, 96, 100), 100).reshape(-1)
    K = mask.size
    A = [masked_zero(rs, mask, M) for _ in range(ng)]
    X = rnd(rs, K, N)
    C0 = [rnd(rs, M, N) for _ in range(ng)]
    tab, count, rows, _ = build_table(ar, A[0], mask)
    assert count == 12
    want = [(T64(c) + T64(a).t() @ T64(X)).numpy() for a, c in zip(A, C0)]
    dense = tn_product(ar, A, [X] * ng, C0, None, 'd_', pair)
    live = tn_product(ar, A, [X] * ng, C0, tab, 'l_', pair)
    for g in range(ng):
        ed, el = rel_err(dense[g], want[g]), rel_err(live[g], want[g])
        print('N=%d M=%d group %d: dense %.2e live %.2e of float64' % (N, M, g, ed, el))
        assert ed < ACC_TOL and el < ACC_TOL
    if N * M > 64 * 64:          # the lean split-K kernel: it must have walked the table
        inside = np.zeros(K + 32, bool)
        for r in rows:
            inside[r:r + 32] = True
        Xn = X.copy()
        Xn[~inside[:K]] = np.nan
        poisoned = tn_product(ar, A, [Xn] * ng, C0, tab, 'n_', pair)
        for g in range(ng):
            assert np.isfinite(poisoned[g]).all() and rel_err(poisoned[g], want[g]) < ACC_TOL


def test_products_count_zero_and_identity_table(ar):
    rs = np.random.RandomState(9)
    K, M, N = 600, 1024, 256
    X, C0 = rnd(rs, K, N), rnd(rs, M, N)
    # count = 0: every row dead -- nothing is read and nothing is added (X is all NaN: a dense walk would add 0 * NaN)
    tab, count, _, _ = build_table(ar, np.zeros((K, M), np.float32), np.ones(K, bool), 'zero')
    assert count == 0
    got = tn_product(ar, [np.zeros((K, M), np.float32)], [np.full((K, N), np.nan, np.float32)], [C0], tab, 'z_')[0]
    assert np.array_equal(got.view(np.int32), C0.view(np.int32))
    # the identity table: the same pieces as the dense walk
    A = rnd(rs, K, M)
    tab, count, rows, _ = build_table(ar, A, np.zeros(K, bool), 'ident')
    assert rows == list(range(0, K, 32))
    want = (T64(C0) + T64(A).t() @ T64(X)).numpy()
    dense, live = tn_product(ar, [A], [X], [C0], None, 'id_')[0], tn_product(ar, [A], [X], [C0], tab, 'il_')[0]
    assert rel_err(dense, want) < ACC_TOL and rel_err(live, want) < ACC_TOL
    # ... and a reduction short enough for one piece per tile (no float atomics between pieces): bit-equal.  (Such a product is
    # not cut along K, so it runs on the general kernel, which ignores the table: this pins that a table handed to a kernel
    # without table support changes nothing; the table walk itself is proven by the NaN rows above and in the test before.)
    Ks = 96
    As, Xs = rnd(rs, Ks, M), rnd(rs, Ks, N)
    tab, count, rows, _ = build_table(ar, As, np.zeros(Ks, bool), 'short')
    assert rows == [0, 32, 64]
    dense, live = tn_product(ar, [As], [Xs], [C0], None, 'sd_')[0], tn_product(ar, [As], [Xs], [C0], tab, 'sl_')[0]
    assert np.array_equal(dense.view(np.int32), live.view(np.int32))
    assert rel_err(live, (T64(C0) + T64(As).t() @ T64(Xs)).numpy()) < ACC_TOL


# --------------------------------------------------------------------------------------------------------------- 3. the chain
B, SX, SY, D, H, DH, R, CREL = 4, 14, 100, 256, 4, 64, 64, 4
LENS = (10, 37, 64, 100)
XLENS = (14, 9, 5, 12)
P_DROP = 0.1
OPS = ('self_att_64', 'rel_self_att_64', 'guided_att_64', 'feed_forward')
SEEDS = (0x1234567811, 0x2345678922, 0x3456789033, 0x4567890144)
GATES = (0.9, 0.8, 1.1, 0.7)     # mixed chain: every node's sampled candidate (candidate 0 of a gate row of width 2)


class _Cfg:
    HSIZE, REL_SIZE = D, R


def _chain_case():
    rs = np.random.RandomState(42)
    c = dict(x=rnd(rs, B, SX, D), y=rnd(rs, B, SY, D), raw=rnd(rs, B, SY, SY, CREL),
             Wy=rnd(rs, R, CREL) / 2, by=0.1 * rnd(rs, R), P=[])
    for name in OPS:
        P = {}
        for k, sh in O.op_param_shapes(name, _Cfg, norm=True).items():
            if k == 'ln.a_2':
                P[k] = (1 + 0.1 * rnd(rs, *sh)).astype(np.float32)
            elif k == 'mhatt.linear_r.bias':
                P[k] = (1 + 0.1 * rnd(rs, *sh)).astype(np.float32)      # (the bias away from its 1e-6 clamp)
            elif len(sh) == 2:
                P[k] = (rnd(rs, *sh) / np.sqrt(sh[1])).astype(np.float32)
            else:
                P[k] = 0.1 * rnd(rs, *sh)
        c['P'].append(P)
    c['x_mask'], c['y_mask'] = prefix_mask(XLENS, SX), prefix_mask(LENS, SY)
    g = rnd(rs, B, SY, D)
    c['dy_any'] = g.copy()
    g[c['y_mask']] = 0
    c['dy_zero'] = g
    return c


def _chain_oracle(c, dy, mixed=False):
    """The four operators in float64 with the kernels' dropout masks replayed: name -> gradient of every weight matrix.
    mixed: every operator is the sampled candidate of a supernet node, its output scaled by the node's gate (mixed.py:59-68)."""
    P = [{k: T64(v).requires_grad_(True) for k, v in p.items()} for p in c['P']]
    x, y = T64(c['x']), T64(c['y'])
    rel = torch.relu(T64(c['raw']) @ T64(c['Wy']).t() + T64(c['by']))
    xm = torch.from_numpy(c['x_mask']).reshape(B, 1, 1, SX)
    ym = torch.from_numpy(c['y_mask']).reshape(B, 1, 1, SY)
    for i, name in enumerate(OPS):
        drops = {'out': dropout_rng.scaled_mask(SEEDS[i], 1, (B, SY, D), P_DROP)}
        if name == 'feed_forward':
            drops['hid0'] = dropout_rng.scaled_mask(SEEDS[i], 0, (B, SY, 4 * D), P_DROP)
        else:
            drops['att_map'] = dropout_rng.scaled_mask(SEEDS[i], 0, (B, H, SY, SX if name.startswith('guided') else SY), P_DROP)
        drops = {k: T64(v) for k, v in drops.items()}
        # (cell signature: the operator's own stream first; a guided operator's keys are the language rows)
        y = O.op_forward(name, P[i], _Cfg, y, x, ym, xm, rel, norm=True, residual=True, drops=drops)
        if mixed:
            y = GATES[i] * y
    (y * T64(dy)).sum().backward()
    return {'%d.%s' % (i, k): p.grad.numpy() for i in range(len(OPS)) for k, p in P[i].items() if p.dim() == 2 and 'linear_r' not in k}


def _run_chain(ar, c, dy, tag, live, side=0, mixed=False):
    """mmnas_chain_fwd + _bwd inside the arena -> (name -> weight gradients, name -> every other output).  Asserts that all
    eight image-stream weight-gradient launches walked a table with the switch on, and none with it off."""
    L = _L()
    lib = L.lib()
    up = lambda a, n: ar.inp(a, name=tag + n)[0]
    acc, recs = {}, []

    def grad(key, like):
        flat, view = ar.inout(np.zeros_like(like), name=tag + 'd_' + key)
        acc[key] = view
        return L.fptr(flat)

    Wyd, byd = up(c['Wy'], 'Wy'), up(c['by'], 'by')
    dWy, dby = grad('Wy', c['Wy']), grad('by', c['by'])
    for i, (name, P) in enumerate(zip(OPS, c['P'])):
        r = L.ChainOp()
        r.on_y, r.node = 1, i
        dev = {k: up(v, '%d.%s' % (i, k)) for k, v in P.items()}
        g = {k: grad('%d.%s' % (i, k), v) for k, v in P.items()}
        if name == 'feed_forward':
            r.kind = 1
            m = r.mlp
            m.nl = 2
            m.dims[0], m.dims[1], m.dims[2] = D, 4 * D, D
            m.flags, m.drop_p, m.eps, m.seed = L.F_NORM | L.F_RESIDUAL | L.F_TRAIN, P_DROP, 1e-6, SEEDS[i]
            for j, pre in enumerate(('mlp.fc.linear.', 'mlp.linear.')):
                m.W[j], m.b[j] = L.fptr(dev[pre + 'weight']), L.fptr(dev[pre + 'bias'])
                m.dW[j], m.db[j] = g[pre + 'weight'], g[pre + 'bias']
            m.ln_a, m.ln_b, m.dln_a, m.dln_b = L.fptr(dev['ln.a_2']), L.fptr(dev['ln.b_2']), g['ln.a_2'], g['ln.b_2']
        else:
            r.kind = 0
            a = r.att
            a.di, a.dh, a.H = D, DH, H
            a.flags = L.F_NORM | L.F_RESIDUAL | L.F_TRAIN | (0 if name.startswith('guided') else L.F_SELF)
            a.drop_p, a.eps, a.seed = P_DROP, 1e-6, SEEDS[i]
            for f, k in (('Wq', 'q'), ('Wk', 'k'), ('Wv', 'v'), ('Wm', 'merge')):
                setattr(a, f, L.fptr(dev['mhatt.linear_%s.weight' % k]))
                setattr(a, 'd' + f, g['mhatt.linear_%s.weight' % k])
            a.ln_a, a.ln_b, a.dln_a, a.dln_b = L.fptr(dev['ln.a_2']), L.fptr(dev['ln.b_2']), g['ln.a_2'], g['ln.b_2']
            if name.startswith('rel'):
                a.flags |= L.F_REL | L.F_RELRAW
                a.R, a.C = R, CREL
                a.Wr, a.br = L.fptr(dev['mhatt.linear_r.weight']), L.fptr(dev['mhatt.linear_r.bias'])
                a.dWr, a.dbr = g['mhatt.linear_r.weight'], g['mhatt.linear_r.bias']
                a.Wy, a.by, a.dWy, a.dby = L.fptr(Wyd), L.fptr(byd), dWy, dby
        recs.append(r)
    arr = (L.ChainOp * len(recs))(*recs)
    ch = L.Chain()
    ch.n_ops, ch.ops = len(recs), arr
    ch.B, ch.Sx, ch.Sy, ch.d = B, SX, SY, D
    ch.x_in, ch.y_in = L.fptr(up(c['x'], 'x')), L.fptr(up(c['y'], 'y'))
    ch.x_mask, ch.y_mask = L.ptr(up(c['x_mask'].astype(np.uint8), 'xm')), L.ptr(up(c['y_mask'].astype(np.uint8), 'ym'))
    ch.y_rel = L.fptr(up(c['raw'], 'raw'))
    if mixed:        # (before the plan: a mixed chain's arena holds the nodes' blocks behind the operators')
        gate = np.zeros((len(OPS), 2), np.float32)
        gate[:, 0] = GATES
        dgate, acc['gate'] = ar.inout(np.zeros_like(gate), name=tag + 'dgate')
        ch.mixed, ch.gate_width, ch.gate, ch.dgate = 1, 2, L.fptr(up(gate, 'gate')), L.fptr(dgate)
    sz = C.c_size_t()
    L.check(lib.mmnas_chain_plan(C.byref(ch), C.byref(sz)))
    arena, _ = ar.scratch(sz.value, name=tag + 'arena')
    outs = {}
    for k, shape in (('x_out', (B, SX, D)), ('y_out', (B, SY, D)), ('dx_in', (B, SX, D)), ('dy_in', (B, SY, D))):
        flat, outs[k] = ar.out(shape, name=tag + k)
        setattr(ch, k, L.fptr(flat))
    ch.arena, ch.dy_out = L.ptr(arena), L.fptr(up(dy, 'dy_out'))
    ch.dx_out, ch.use_side_stream = None, side
    prev = lib.mmnas_set_wgrad_live(live)
    try:
        L.check(lib.mmnas_chain_fwd(C.byref(ch), L.stream()))

        def bwd():
            L.check(lib.mmnas_chain_bwd(C.byref(ch), L.stream()))
            if side:
                L.check(lib.mmnas_chain_join(L.stream(), L.stream()))
        _, tags = live_tags(bwd)
    finally:
        lib.mmnas_set_wgrad_live(prev)
    # per operator: the merge projection's dW and the (grouped) dWq / dWk / dWv, or the two layers of the feed-forward
    assert sum(' live' in t for t in tags) == (8 if live else 0), tags
    ar.check()       # 4.: the arena's bands (the table lies inside it), every input, every output written and finite
    res = {k: v.cpu().numpy() for k, v in list(acc.items()) + list(outs.items())}
    is_w = lambda k: res[k].ndim == 2 and k.endswith('weight') and 'linear_r' not in k
    return {k: v for k, v in res.items() if is_w(k)}, {k: v for k, v in res.items() if not is_w(k)}


@pytest.fixture(scope='module')
def chain_case():
    c = _chain_case()
    c['want'] = {False: _chain_oracle(c, c['dy_zero']), True: _chain_oracle(c, c['dy_zero'], mixed=True)}
    return c


@pytest.mark.parametrize('side,mixed', [(0, False), (1, False), (0, True)])
def test_chain_switch_off_and_on(ar, chain_case, side, mixed):
    """(Once with the parameter-gradient work on the side stream, once as a mixed chain: each operator the sampled candidate of
    a supernet node, its output scaled by the node's gate.)  SelfAtt, RelSelfAtt, GuidedAtt and FeedForward on the image stream of a padded batch of 10, 37, 64 and 100 regions.  The
    weight gradients with the switch off and on against the float64 oracle (TOL, the chain tests' bound) and against each other
    at the accumulate products' bound; everything else bit for bit wherever two runs with the switch off agree bit for bit."""
    c = chain_case
    w_off, o_off = _run_chain(ar, c, c['dy_zero'], 'a_', 0, side, mixed)
    w_off2, o_off2 = _run_chain(ar, c, c['dy_zero'], 'b_', 0, side, mixed)
    w_on, o_on = _run_chain(ar, c, c['dy_zero'], 'c_', 1, side, mixed)
    # the padded rows' gradient stays exactly zero through the chain: what the table relies on
    assert not np.any(o_on['dy_in'][c['y_mask']])
    # Two outputs are sums of float atomics in no fixed order -- dx_in (the guided operator's key / value source gradient, an
    # accumulating product cut along K) and the hidden layer's bias gradient (column sums added per tile): two runs with the
    # switch off may or may not agree bit for bit, so two equal runs prove nothing; they are held to the off runs' spread.
    # Everything else must repeat bit for bit with the switch off, and then be the same bits with it on.
    atomic = ('dx_in', '3.mlp.fc.linear.bias')
    for k in o_off:
        if k in atomic:
            assert rel_err(o_on[k], o_off[k]) <= spread_bound(rel_err(o_off2[k], o_off[k])), k
        else:
            assert np.array_equal(o_off[k].view(np.int32), o_off2[k].view(np.int32)), k
            assert np.array_equal(o_on[k].view(np.int32), o_off[k].view(np.int32)), k
    assert {'x_out', 'y_out', 'dy_in'} <= set(o_off) and len(o_off) - len(atomic) >= 16
    assert len(w_on) == 14 and set(w_on) == set(c['want'][mixed])
    for k, want in c['want'][mixed].items():
        e_off, e_on, e_mut = rel_err(w_off[k], want), rel_err(w_on[k], want), rel_err(w_on[k], w_off[k])
        print('%-32s off %.2e on %.2e of float64, on - off %.2e' % (k, e_off, e_on, e_mut))
        assert e_off <= TOL and e_on <= TOL, k
        assert e_mut <= 1e-5, k


def test_chain_gradient_that_is_not_zero_under_the_mask(ar, chain_case):
    """A caller whose dy_out is random on the masked rows too: every row is live, the table is the identity and the switch
    changes nothing beyond the order of the float atomics."""
    c = chain_case
    w_off, o_off = _run_chain(ar, c, c['dy_any'], 'a_', 0)
    w_off2, o_off2 = _run_chain(ar, c, c['dy_any'], 'b_', 0)
    w_on, o_on = _run_chain(ar, c, c['dy_any'], 'c_', 1)
    assert np.any(o_on['dy_in'][c['y_mask']])
    for k in ('x_out', 'y_out', 'dy_in'):
        assert np.array_equal(o_on[k].view(np.int32), o_off[k].view(np.int32)), k
    assert rel_err(o_on['dx_in'], o_off['dx_in']) <= spread_bound(rel_err(o_off2['dx_in'], o_off['dx_in']))
    for k in w_off:
        e_self, e_mut = rel_err(w_off2[k], w_off[k]), rel_err(w_on[k], w_off[k])
        print('%-32s off - off %.2e on - off %.2e' % (k, e_self, e_mut))
        assert e_mut <= spread_bound(e_self), k
