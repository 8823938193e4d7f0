"""The ragged language stream (ops.set_unpad_x) without a GPU: the plan's decision as a function of the token counts, the
chain planner with mmnas_chain.x_off (arena size, argument checks with their messages), and the two places the counts
travel through without a device-to-host copy (data.DevicePrefetcher with two length pairs, harness.triplet_batch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import host_plan_driver as D


# ---------------------------------------------------------------------------------------- 1. the plan's decision
@pytest.mark.parametrize('lengths, T, want', [
    ((3, 14, 9), 20, (14, False)),                 # T' <= 16: trimmed, dense (the one-launch short-sequence operators)
    ((16, 2), 50, (16, False)),
    ((17, 2), 50, (17, True)),                     # the first packed length
    ((1, 5, 16, 17, 20), 23, (20, True)),
    ((128, 3), 128, (128, True)),                  # the largest packed length ...
    ((129, 3), 140, (129, False)),                 # ... and the first the packed attention cores do not take
    ((17, 17, 17), 23, (17, False)),               # no padding left behind the trim: dense
    ((50, 50), 50, (50, False)),                   # nothing to trim, nothing to pack
    ((5, 0, 7), 20, None),                         # a sample without a token
    ((5, 21), 20, None),                           # a count the tensor cannot hold
    ((), 20, None),
])
def test_decision_is_a_pure_function_of_lengths_and_T(lengths, T, want):
    from mmnas_amd import ops
    assert ops.language_decision(list(lengths), T) == want


def test_switch_and_cpu_tensors():
    from mmnas_amd import ops
    assert ops.unpad_x_enabled() is False                      # default off
    ix = torch.tensor([[4, 9, 2, 0, 0], [7, 0, 0, 0, 0]])
    ix._mmnas_lengths = [3, 1]
    assert ops.language_plan(ix, ix == 0) is None              # switch off
    assert ops.set_unpad_x(True) is False
    try:
        assert ops.unpad_x_enabled() is True
        assert ops.language_plan(ix, ix == 0) is None          # CPU tensors: today's path
        assert ops.language_plan(ix) is None
        assert ops.unpad_enabled() is False                    # independent of the decoder stream's switch
    finally:
        assert ops.set_unpad_x(False) is True
    assert ops.unpad_x_enabled() is False


# ---------------------------------------------------------------------------------------- 2. mmnas_chain_plan with x_off
def _itm_chain(L, enc_rel=False, **kw):
    """2 encoder layers (self-attention + FFN) and 2 decoder layers (self, guided, FFN) at the ITM dimensions."""
    recs, k = [], 0
    for _ in range(2):
        recs += [D.att_record(L, 0, True, enc_rel, 256, node=k), D.mlp_record(L, 0, 256, node=k + 1)]
        k += 2
    for _ in range(2):
        recs += [D.att_record(L, 1, True, False, 256, node=k), D.att_record(L, 1, False, False, 256, node=k + 1),
                 D.mlp_record(L, 1, 256, node=k + 2)]
        k += 3
    return D.chain(L, recs, **kw)


def _plan(L, ch):
    sz = C.c_size_t()
    rc = L.lib().mmnas_chain_plan(C.byref(ch), C.byref(sz))
    return rc, sz.value, L.lib().mmnas_last_error().decode()


def test_chain_plan_with_x_off_shrinks_and_checks_its_arguments():
    from mmnas_amd import _lib as L
    assert 'x_off' in dict((f[0], f[1]) for f in L.Chain._fields_)
    B, Sx, Sy, d = 160, 50, 36, 256
    ch, keep = _itm_chain(L, B=B, Sx=Sx, Sy=Sy, d=d)
    rc, padded, _ = _plan(L, ch)
    assert rc == 0
    Nx = B * 12
    ch.x_off, ch.Nx = D.FAKE, Nx
    rc, packed, msg = _plan(L, ch)
    assert rc == 0, msg
    # every language-stream block follows the packed row count: at least the encoder's output, input-gradient and saved Q / K / V
    # / att blocks shrink by (B Sx - Nx) d floats each, and the guided operators' K / V with them
    assert packed < padded - 4 * 6 * (B * Sx - Nx) * d * 4
    # the packed plan depends on Nx alone, not on the padded length behind it (128 = the longest packed stream)
    ch.Sx = 128
    assert _plan(L, ch)[0] == 0
    ch.Sx = Sx
    # argument checks: MMNAS_E_ARG (-2) with a message
    ch.Nx = B * Sx + 1
    rc, _, msg = _plan(L, ch)
    assert rc == -2 and 'ragged language stream' in msg and 'Nx' in msg
    ch.Nx = 0
    assert _plan(L, ch)[0] == -2
    ch.Nx = Nx
    ch.Sx = 129
    rc, _, msg = _plan(L, ch)
    assert rc == -2 and 'Sx=129' in msg
    ch.Sx = Sx
    ch.use_side_stream = 1
    rc, _, msg = _plan(L, ch)
    assert rc == -2 and 'single stream' in msg
    ch.use_side_stream = 0
    assert _plan(L, ch)[0] == 0
    ch2, keep2 = _itm_chain(L, enc_rel=True, B=B, Sx=Sx, Sy=Sy, d=d)
    assert _plan(L, ch2)[0] == 0                               # (padded: an encoder relation operator is fine)
    ch2.x_off, ch2.Nx = D.FAKE, Nx
    rc, _, msg = _plan(L, ch2)
    assert rc == -2 and 'relation bias' in msg
    # both streams ragged; the mixed chain's node buffers follow the packed rows too
    ch.y_off, ch.y_tile_off, ch.Ny, ch.y_ntiles = D.FAKE, D.FAKE, B * 20, B * 13
    rc, both, msg = _plan(L, ch)
    assert rc == 0 and both < packed, msg


def test_mixed_chain_plan_with_x_off_shrinks():
    from mmnas_amd import _lib as L
    recs = []
    for k in range(4):
        recs += [D.att_record(L, 0, True, False, 256, node=k, cand=0, detached=int(k % 2 != 0)),
                 D.mlp_record(L, 0, 256, node=k, cand=1, detached=int(k % 2 == 0))]
    for k in range(4, 8):
        a = k % 3
        recs += [D.att_record(L, 1, True, False, 256, node=k, cand=0, detached=int(a != 0)),
                 D.att_record(L, 1, False, False, 256, node=k, cand=1, detached=int(a != 1)),
                 D.mlp_record(L, 1, 256, node=k, cand=2, detached=int(a != 2))]
    ch, keep = D.chain(L, recs, B=32, Sx=50, Sy=36, d=256, mixed=True)
    rc, padded, msg = _plan(L, ch)
    assert rc == 0, msg
    ch.x_off, ch.Nx = D.FAKE, 32 * 11
    rc, packed, msg = _plan(L, ch)
    assert rc == 0 and packed < padded - 8 * (32 * 50 - 32 * 11) * 256 * 4, msg


def test_att_op_plan_takes_packed_keys_under_dense_queries():
    """The guided operator of a ragged language stream: k_off without q_off."""
    from mmnas_amd import _lib as L
    op = L.AttOp()
    op.B, op.Sq, op.Sk, op.d, op.di, op.H, op.dh = 8, 36, 50, 256, 256, 4, 64
    op.flags = L.F_NORM | L.F_RESIDUAL
    p, q = L.Plan(), L.Plan()
    L.check(L.lib().mmnas_att_op_plan(C.byref(op), C.byref(p)))
    op.k_off, op.Mk = D.FAKE, 8 * 10
    L.check(L.lib().mmnas_att_op_plan(C.byref(op), C.byref(q)))
    assert q.save_bytes < p.save_bytes and q.ws_bwd_bytes < p.ws_bwd_bytes
    op.Mk = 8 * 50 + 1
    assert L.lib().mmnas_att_op_plan(C.byref(op), C.byref(q)) == -2
    op.Mk, op.flags = 8 * 10, op.flags | L.F_MASK
    assert L.lib().mmnas_att_op_plan(C.byref(op), C.byref(q)) == -2 and 'no mask' in L.lib().mmnas_last_error().decode()


# ---------------------------------------------------------------------------------------- 3. the counts travel with the batch
def _batch(B=4, S=6, T=7, F=8, seed=0):
    r = np.random.RandomState(seed)
    nreg, nwords = r.randint(1, S + 1, B), r.randint(1, T + 1, B)
    feat = r.randn(B, S, F).astype(np.float32)
    ix = r.randint(1, 90, (B, T)).astype(np.int64)
    for b in range(B):
        feat[b, nreg[b]:] = 0
        ix[b, nwords[b]:] = 0
    return feat, ix, nreg, nwords


def test_prefetcher_attaches_two_length_pairs():
    from mmnas_amd.data import DevicePrefetcher
    feat, ix, nreg, nwords = _batch()
    batch = {'frcn': feat, 'ix': ix, 'nreg': nreg, 'nwords': nwords}
    out = next(iter(DevicePrefetcher([batch], 'cpu', lengths=[('frcn', 'nreg'), ('ix', 'nwords')])))
    assert out['frcn']._mmnas_lengths == nreg.tolist() and out['ix']._mmnas_lengths == nwords.tolist()
    # the single-pair form is unchanged; tuples of positions work as well
    out = next(iter(DevicePrefetcher([batch], 'cpu', lengths=('frcn', 'nreg'))))
    assert out['frcn']._mmnas_lengths == nreg.tolist() and not hasattr(out['ix'], '_mmnas_lengths')
    out = next(iter(DevicePrefetcher([(feat, ix, nreg, nwords)], 'cpu', lengths=((0, 2), (1, 3)))))
    assert out[0]._mmnas_lengths == nreg.tolist() and out[1]._mmnas_lengths == nwords.tolist()
    # word counts that disagree with the zero-token padding are refused before the upload
    wrong = nwords.copy()
    wrong[2] = wrong[2] - 1 if wrong[2] > 1 else wrong[2] + 1
    with pytest.raises(ValueError, match='word counts'):
        next(iter(DevicePrefetcher([dict(batch, nwords=wrong)], 'cpu', lengths=[('ix', 'nwords')])))
    hole = ix.copy()
    b = int(np.argmax(nwords))
    if nwords[b] >= 2:
        hole[b, 0] = 0                                         # a zero token inside a question
        with pytest.raises(ValueError, match='word counts'):
            next(iter(DevicePrefetcher([dict(batch, ix=hole)], 'cpu', lengths=[('ix', 'nwords')])))
    out = next(iter(DevicePrefetcher([dict(batch, nwords=wrong)], 'cpu', lengths=[('ix', 'nwords')], validate=None)))
    assert out['ix']._mmnas_lengths == wrong.tolist()


def test_triplet_batch_carries_lengths():
    from mmnas_amd.harness import triplet_batch
    T = torch.from_numpy

    def part(seed, lens=True):
        feat, ix, nreg, nwords = _batch(seed=seed)
        f, i = T(feat), T(ix)
        if lens:
            f._mmnas_lengths, i._mmnas_lengths = nreg.tolist(), nwords.tolist()
        return (f, None, T(np.zeros((4, 6, 6, 4), np.float32)), i, None), nreg.tolist(), nwords.tolist()

    (pos, preg, pw), (neg, nreg, nw) = part(1), part(2)
    out = triplet_batch(pos, neg)
    assert out[0].shape[0] == 12 and out[1] is None and out[4] is None
    assert out[0]._mmnas_lengths == preg + preg + nreg           # images: (pos, pos, neg)
    assert out[3]._mmnas_lengths == pw + nw + pw                 # captions: (pos, neg, pos)
    assert not hasattr(out[2], '_mmnas_lengths')
    neg2, _, _ = part(2, lens=False)
    out = triplet_batch(pos, neg2)                               # one part without counts: none are attached
    assert not hasattr(out[0], '_mmnas_lengths') and not hasattr(out[3], '_mmnas_lengths')
