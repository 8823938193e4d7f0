"""Key-limited walk of mmnas_rel_multi_fwd / _bwd (relmulti.hip, `key_mask`; mmnas_set_rel_keylimit): with the [B, S] key mask
of the attention cores that consume the bias, the kernels walk of every sample's [S_k, S_q] plane only the nk_b S elements
under keys below nk_b = 1 + the last unmasked key.  Forward leaves the rest of biasT unwritten, backward never reads dbiasT
there -- the cores replace the score under a masked key after adding the bias and write its bias gradient as exactly 0.

Direct calls inside a tests/guardband.py Arena (test_rel_multi's conditioning -- no bias gradient next to the clamp -- and its
bounds: gradients within 1e-4 of float64), then a supernet weight step and a MODE 'full' architecture step with the walk off
and on: logits, loss and every non-relation gradient bit for bit, the relation parameters' gradients to round-off."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.guardband import Arena
from tests.kernel_refs import rel_multi_pre, rel_multi_ref
from tests.util import REL_PATH_SELF_TOL, is_rel_path, rel_err

pytestmark = pytest.mark.gpu

DEV = 'cuda'
R = 64


def _L():
    import mmnas_amd._lib as L
    return L


def rnd(rs, *shape):
    return rs.standard_normal(shape).astype(np.float32)


def zeros(*shape):
    return np.zeros(shape, np.float32)


def bits(view):
    return view.cpu().numpy().view(np.int32)


@pytest.fixture
def ar():
    yield Arena(DEV)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a fault on the device: nothing more is started on it
        pytest.exit('GPU error in a key-limit case, the session ends here: %s' % e, returncode=3)


def _mask(S, kind):
    """One sample's key mask (True = masked) and its limit.  'full': nothing masked; an integer n: keys n.. masked (0: every
    key); 'holes': only keys 0 and 5 unmasked -- limit 6, the masked keys 1..4 are still computed."""
    m = np.ones(S, bool)
    if kind == 'full':
        m[:] = False
        return m, S
    if kind == 'holes':
        m[[0, 5]] = False
        return m, 6
    m[:kind] = False
    return m, kind


# (4, 23, 4, 4, 9): 36 head rows = 2 row tiles forward, 2 launches backward; limit 7 at S = 23: 161 elements, a partial last tile
CASES = [((4, 23, 4, 4, 9), ('full', 1, 7, 0)),
         ((4, 23, 4, 4, 9), ('holes', 7, 'full', 1)),
         ((3, 9, 3, 32, 1), (7, 'holes', 0)),
         ((2, 33, 4, 4, 3), (7, 'full')),
         ((2, 33, 4, 4, 3), (0, 0))]


@pytest.mark.parametrize('shape,kinds', CASES)
def test_key_limited_walk(ar, shape, kinds):
    B, S, C_, H, n_ops = shape
    L = _L()
    lib = L.lib()
    rs = np.random.RandomState(B * 31 + S + 7 * H + C_ + n_ops)
    assert lib.mmnas_rel_multi_supported(C_, R, H) == 1
    mask = np.zeros((B, S), bool)
    nk = []
    for b, kind in enumerate(kinds):
        mask[b], n = _mask(S, kind)
        nk.append(n)
    below = np.arange(S)[None, :] < np.array(nk)[:, None]                        # [B, S_k]: keys the walk covers
    assert all(not mask[b, n - 1] and mask[b, n:].all() for b, n in enumerate(nk) if n) and all(mask[b].all() for b, n in enumerate(nk) if not n)
    walked = np.broadcast_to(below[:, None, :, None], (B, H, S, S))
    unmasked = np.broadcast_to(~mask[:, None, :, None], (B, H, S, S))
    raw = rnd(rs, B, S, S, C_)
    Wy, by = rnd(rs, R, C_) / 2, 0.1 * rnd(rs, R)
    Wrs, brs = [rnd(rs, H, R) / 8 for _ in range(n_ops)], [0.1 * rnd(rs, H) for _ in range(n_ops)]
    gbs = []
    for i in range(n_ops):
        g = np.where(np.abs(rel_multi_pre(raw, Wy, by, Wrs[i], brs[i])) < 0.05, 0.0, rnd(rs, B, H, S, S))
        gbs.append(np.where(unmasked, g, 0.0).astype(np.float32))             # random under unmasked keys, 0 under masked ones
    (rawd, _), (Wyd, _), (byd, _) = ar.inp(raw, name='raw'), ar.inp(Wy, name='Wy'), ar.inp(by, name='by')
    (maskd, _) = ar.inp(mask.astype(np.uint8), name='key_mask')
    Wrd = [ar.inp(Wrs[i], name='Wr%d' % i)[0] for i in range(n_ops)]
    brd = [ar.inp(brs[i], name='br%d' % i)[0] for i in range(n_ops)]
    gb_dense = [ar.inp(gbs[i], name='dbiasT%d' % i)[0] for i in range(n_ops)]
    # ... and NaN at or beyond the limit: a walk that read there would carry it into every gradient
    gb_nan = [ar.inp(np.where(walked, gbs[i], np.nan).astype(np.float32), name='dbiasT%d_nan' % i)[0] for i in range(n_ops)]

    def run(tag, key_mask, switch, dbias, written):
        m = L.RelMulti()
        m.B, m.S, m.C, m.R, m.H, m.n_ops = B, S, C_, R, H, n_ops
        (dWyd, dWyv), (dbyd, dbyv) = ar.inout(zeros(R, C_), name=tag + 'dWy'), ar.inout(zeros(R), name=tag + 'dby')
        ws, _ = ar.scratch_floats(lib.mmnas_rel_multi_bwd_ws_floats(B, S), name=tag + 'ws')
        m.raw, m.Wy, m.by, m.dWy, m.dby, m.ws = L.fptr(rawd), L.fptr(Wyd), L.fptr(byd), L.fptr(dWyd), L.fptr(dbyd), L.fptr(ws)
        m.key_mask = L.ptr(maskd) if key_mask else None
        bias, dWr, dbr = [], [], []
        for i in range(n_ops):
            bias.append(ar.out((B, H, S, S), name='%sbiasT%d' % (tag, i), written=written))
            dWr.append(ar.inout(zeros(H, R), name='%sdWr%d' % (tag, i)))
            dbr.append(ar.inout(zeros(H), name='%sdbr%d' % (tag, i)))
            m.Wr[i], m.br[i], m.dbiasT[i] = L.fptr(Wrd[i]), L.fptr(brd[i]), L.fptr(dbias[i])
            m.biasT[i], m.dWr[i], m.dbr[i] = L.fptr(bias[i][0]), L.fptr(dWr[i][0]), L.fptr(dbr[i][0])
        prev = lib.mmnas_set_rel_keylimit(switch)
        try:
            L.check(lib.mmnas_rel_multi_fwd(C.byref(m), L.stream()))
            L.check(lib.mmnas_rel_multi_bwd(C.byref(m), L.stream()))
        finally:
            lib.mmnas_set_rel_keylimit(prev)
        ar.check()          # bands, inputs, and the footprint: `written` elements written and finite, the rest still the fill
        return ([bits(v) for _, v in bias],
                [v.cpu().numpy() for _, v in dWr] + [v.cpu().numpy() for _, v in dbr] + [dWyv.cpu().numpy(), dbyv.cpu().numpy()])

    dense_b, dense_g = run('d_', False, 0, gb_dense, True)
    lim_b, lim_g = run('k_', True, 1, gb_nan, walked)
    # 1. forward values under keys below the limit: the dense call's, bit for bit (2.: the footprint, checked by run)
    for i in range(n_ops):
        assert np.array_equal(lim_b[i][walked], dense_b[i][walked]), i
    # 4. backward against float64; 5. against the dense call -- test_rel_multi's bound
    rdWr, rdbr, rdWy, rdby = rel_multi_ref(raw, Wy, by, Wrs, brs, gbs, np.ones((B, 1, S, S), np.float32))[1:]
    for got, dense, want in zip(lim_g, dense_g, list(rdWr) + list(rdbr) + [rdWy, rdby]):
        assert np.isfinite(got).all()
        assert rel_err(got, want) < 1e-4 and rel_err(dense, want) < 1e-4
        assert rel_err(got, dense) < 1e-4
    if not any(nk):
        assert all(not np.any(g) for g in lim_g)
    # 6. the assignment of tiles to waves is a function of the mask: a second run gives the same bits
    again_b, again_g = run('r_', True, 1, gb_nan, walked)
    assert all(np.array_equal(a, b) for a, b in zip(again_b, lim_b))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(again_g, lim_g))
    # 7. no mask with the switch on, the mask with the switch off: the whole plane, the dense result bit for bit
    for tag, key_mask, switch in (('n_', False, 1), ('o_', True, 0)):
        off_b, off_g = run(tag, key_mask, switch, gb_dense, True)
        assert all(np.array_equal(a, b) for a, b in zip(off_b, dense_b)), tag
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(off_g, dense_g)), tag


# ----------------------------------------------------------------------------------------------------------------------
# Chain level: the backbone chains hand every relation group the key mask of its operators' attention cores
# ----------------------------------------------------------------------------------------------------------------------
# A bitwise comparison needs gradients that are reproducible run to run with the walk off as well.  The embedding rows and the
# hidden-layer bias column sums are accumulated with float atomics (head.hip, gemm.hip): the same bits whatever the order only
# for up to two addends -- so at most 64 image rows (two 32-row tiles per column sum), every token once, two padding tokens.
LENS = (19, 1, 7)          # regions per sample of the padded batch: the maximum and 1 among them
XLENS = (6, 5, 5)          # tokens per sample


def _padded_case(net_case):
    def make(*a, **k):
        c = net_case(*a, **k)
        frcn, bbox, y_rel, ques, x_rel = (np.array(t) for t in c['inputs'])
        rs = np.random.RandomState(5)
        frcn = np.maximum(rs.standard_normal(frcn.shape), 0).astype(np.float32)
        frcn[:, :, 0] += 0.5                                                     # (no all-zero row among the valid ones)
        y_rel = rs.standard_normal(y_rel.shape).astype(np.float32)
        x_rel = rs.standard_normal(x_rel.shape).astype(np.float32)
        assert frcn.shape[:2] == (len(LENS), max(LENS)) and ques.shape == (len(XLENS), max(XLENS)) and ques.size < c['token_size']
        ques = 1 + np.arange(ques.size, dtype=ques.dtype).reshape(ques.shape)
        for b, (n, nx) in enumerate(zip(LENS, XLENS)):
            frcn[b, n:] = 0
            y_rel[b, n:] = 0
            y_rel[b, :, n:] = 0
            ques[b, nx:] = 0
            x_rel[b, nx:] = 0
            x_rel[b, :, nx:] = 0
        c['inputs'] = (frcn, bbox, y_rel, ques, x_rel)
        return c
    return make


@pytest.mark.parametrize('mode,n_rel', [(None, 6), ('full', 5)])
def test_chain_steps_with_and_without_the_key_limit(mode, n_rel, monkeypatch):
    """A supernet weight step (mode None) and a MODE 'full' architecture step built as
    test_hoisted_relation_bias_equals_the_per_operator_launches builds them (HSIZE 128), on a padded batch of 19, 1 and 7
    regions.  The bias under a masked key is replaced by the cores' select and its gradient is an exact zero: logits, loss and
    every gradient outside the relation path are the same bits; linear_r / linear_y_rel sum the same terms in another order."""
    import tests.test_chain_gpu as chain
    from mmnas_amd import _lib as L
    lib = L.lib()
    monkeypatch.setattr(chain.cases, 'net_case', _padded_case(chain.cases.net_case))
    losses = []
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def recording(*a, **k):
        out = bce(*a, **k)
        losses.append(out.detach().cpu().numpy().copy())
        return out
    monkeypatch.setattr(torch.nn.functional, 'binary_cross_entropy_with_logits', recording)
    flat = chain._rel_heavy_plan(mode, n_rel)
    outs = []
    for on in (0, 1):
        prev = lib.mmnas_set_rel_keylimit(on)
        try:
            outs.append(chain._run_unpad('vqa', None, True, False, mode, flat, B=len(LENS), Sy=max(LENS)))
        finally:
            lib.mmnas_set_rel_keylimit(prev)
    (out_a, g_a, seen_a), (out_b, g_b, seen_b) = outs[1], outs[0]
    assert seen_a == [False] and seen_b == [False]                               # the padded chain, both times
    assert np.array_equal(out_a.view(np.int32), out_b.view(np.int32))
    assert len(losses) == 2 and np.array_equal(losses[0].view(np.int32), losses[1].view(np.int32))
    top = max(float(np.abs(g).max()) for g in g_b.values() if g is not None)
    n_rel_keys = 0
    for k in g_b:
        if g_b[k] is None:
            assert g_a[k] is None or not np.any(g_a[k]), k
            continue
        assert g_a[k] is not None, k
        if not is_rel_path(k):
            assert np.array_equal(g_a[k].view(np.int32), g_b[k].view(np.int32)), k
            continue
        n_rel_keys += bool(np.any(g_b[k]))
        diff = float(np.abs(g_a[k] - g_b[k]).max())
        assert diff <= max(4e-5, REL_PATH_SELF_TOL) * max(float(np.abs(g_b[k]).max()), 3e-3 * top), (k, diff)      # (_same's bound)
    assert n_rel_keys >= 2 and np.any(g_a['linear_y_rel.weight'])
