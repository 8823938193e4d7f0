"""mmnas_amd.answering on the MI355X: mmnas_vqa_answer against np.argmax / torch.argmax over ragged, tied, infinite and strided
rows, the NaN flag, no host synchronisation in answer_batch / VqaEvaluator.update, device credit and compute() against the
official evaluation's own numbers (tests/golden/vqa.npz), mmnas_vqa_accuracy against the numpy sums on a large subset,
VqaEvaluator on a VQA Net_Full at the train_vqa dimensions against the reference's per-batch path on the same outputs, and
mmnas_vqa_answer_targets against data.answer_targets."""
import numpy as np
import pytest
import torch

from tests.golden import cases
from tests.test_answering_host import (A, N, VOCAB, Z, _Replay, credit, logits_for, pred_accuracy, process_punctuation,
                                       reference_k, sampler_positions)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = torch.from_numpy


def planted(rs, B, A_):
    x = rs.standard_normal((B, A_)).astype(np.float32)
    for b in range(0, B, 3):          # ties of the maximum
        j = rs.choice(A_, min(A_, 3), replace=False)
        x[b, j] = x[b].max() + 1.0
    if B > 1:
        x[1] = -np.inf                # all -inf: index 0
    if B > 2:
        x[2, rs.randint(A_)] = np.inf
        x[2, rs.randint(A_)] = np.inf
    if B > 5:
        x[5, -1] = x[5].max() + 2.0   # the last column
    return x


@pytest.mark.parametrize('A_', [1, 63, 64, 65, 3129, 4099])
@pytest.mark.parametrize('B', [1, 64, 257])
def test_argmax_kernel_is_np_argmax(A_, B):
    from mmnas_amd.answering import answer_batch
    rs = np.random.RandomState(A_ * 1000 + B)
    x = planted(rs, B, A_)
    want = np.argmax(x, 1)
    assert np.array_equal(torch.argmax(T(x), 1).numpy(), want)
    r = answer_batch(T(x).to(DEV))
    assert r['pred'].dtype == torch.int64 and r['credit'] is None
    assert np.array_equal(r['pred'].cpu().numpy(), want)
    # a row slice of a wider tensor (row stride A + 7: rows not 16-byte aligned)
    wide = np.concatenate((x, np.full((B, 7), np.inf, np.float32)), 1)
    r = answer_batch(T(wide).to(DEV)[:, :A_])
    assert np.array_equal(r['pred'].cpu().numpy(), want)


def test_nan_raises_and_check_false_does_not():
    from mmnas_amd.answering import AnsweringError, answer_batch
    rs = np.random.RandomState(1)
    x = rs.standard_normal((64, 3129)).astype(np.float32)
    x[17, 3000] = np.nan
    x[17, 5] = np.nan
    d = T(x).to(DEV)
    with pytest.raises(AnsweringError, match='NaN'):
        answer_batch(d)
    r = answer_batch(d, check=False)
    assert int(r['pred'][17]) == 5            # np.argmax: the first NaN
    assert np.array_equal(np.delete(r['pred'].cpu().numpy(), 17), np.delete(np.argmax(x, 1), 17))


def test_device_credit_equals_the_reference():
    from mmnas_amd.answering import AnsweringError, answer_batch
    c = credit().to(DEV)
    k = reference_k()
    for p in range(int(Z['n_preds'])):
        pred = Z['preds'][p]
        idx = np.arange(N)
        idx[::97] = -1
        r = answer_batch(logits_for(pred, p).to(DEV), T(idx).to(DEV), c)
        assert np.array_equal(r['pred'].cpu().numpy(), pred)
        assert np.array_equal(r['credit'].cpu().numpy(), np.where(idx >= 0, k[np.arange(N), pred], -1))
    # every (question, entry) pair: logits that pick entry v for every question
    for v in range(A):
        x = np.zeros((N, A), np.float32)
        x[:, v] = 1.0
        r = answer_batch(T(x).to(DEV), torch.arange(N, device=DEV), c)
        assert np.array_equal(r['credit'].cpu().numpy(), k[:, v]), v
    for bad in (N, -2):
        idx = torch.arange(4, device=DEV)
        idx[2] = bad
        with pytest.raises(AnsweringError, match='index'):
            answer_batch(torch.zeros(4, A, device=DEV), idx, c)


@pytest.mark.parametrize('p', range(int(Z['n_preds'])))
def test_device_compute_reproduces_vqaeval(p):
    from mmnas_amd.answering import VqaEvaluator
    pred = Z['preds'][p]
    net = _Replay(logits_for(pred, p).to(DEV)).to(DEV)
    ev = VqaEvaluator(net, credit())
    assert ev.device.type == 'cuda' and ev.credit.device.type == 'cuda'
    pos = sampler_positions(N, 1, 0)
    for s in range(0, N, 64):
        ev.update((torch.tensor(pos[s:s + 64], device=DEV), None, None, None, None))
    r = ev.compute()
    ref = pred_accuracy(p)
    assert (r['overall'], r['perQuestionType'], r['perAnswerType']) == (ref['overall'], ref['perQuestionType'],
                                                                         ref['perAnswerType'])
    assert r['exact']['overall'] == (int(reference_k()[np.arange(N), pred].sum()), N)
    assert [x['answer'] for x in ev.results(VOCAB)] == [VOCAB[i] for i in pred]


def test_accuracy_kernel_on_a_large_subset():
    """mmnas_vqa_accuracy over 300 000 positions (the grid-stride loop, many workgroups per bin) against the numpy sums."""
    from mmnas_amd import _lib as L
    from mmnas_amd.answering import _totals_np
    c = credit()
    rs = np.random.RandomState(8)
    M = 300000
    q = rs.randint(0, N, M).astype(np.int32)
    cr = rs.randint(0, 31, M).astype(np.int32)
    want = _totals_np(c, cr, q)
    cd = c.to(DEV)
    na, nt = len(c.ans_type_names), len(c.ques_type_names)
    tot = torch.zeros(2 * (na + nt), dtype=torch.int64, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    qd, crd = T(q).to(DEV), T(cr).to(DEV)
    L.check(L.lib().mmnas_vqa_accuracy(L.ptr(crd), L.ptr(qd), L.ptr(cd.ans_type), L.ptr(cd.ques_type), M, N, na, nt, L.ptr(tot),
                                       L.ptr(flag), L.stream()))
    assert tot.cpu().tolist() == want and int(flag.item()) == 0
    assert sum(want[na:2 * na]) == M


def test_answer_batch_and_update_issue_no_host_sync():
    from mmnas_amd.answering import VqaEvaluator, answer_batch
    c = credit().to(DEV)
    pred = Z['preds'][0]
    x = logits_for(pred).to(DEV)
    idx = torch.arange(64, device=DEV)
    answer_batch(x[:64], idx, c, check=False)     # (first call: library load, allocator warm-up)
    net = _Replay(x).to(DEV)
    ev = VqaEvaluator(net, c)
    ids = torch.arange(64, device=DEV)
    ev.update((ids, None, None, None, None), index=ids)
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        r = answer_batch(x[64:128], idx, c, check=False)
        for s in range(0, N, 64):
            ev.update((torch.arange(s, min(s + 64, N), device=DEV), None, None, None, None))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert np.array_equal(r['pred'].cpu().numpy(), pred[64:128])
    assert ev.compute()['exact']['overall'][1] == N


# ---- the evaluator on a VQA Net_Full at the train_vqa dimensions ------------------------------------------------------------------
def _vqa_case(B=64, seed=23):
    from mmnas.model.full_vqa import Net_Full
    c = cases.net_case('vqa', 'mmnas_vqa', seed, HSIZE=512, B=B, Sx=14, Sy=100, token_size=2000, ans_size=3129)
    net = Net_Full(c['cfg'], {'token_size': c['token_size'], 'ans_size': c['ans_size'],
                              'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)})
    net.load_state_dict({k: T(v) for k, v in c['P'].items()}, strict=True)
    return net.to(DEV).train(), c


def _credit_3129():
    """The fixture's questions against a 3129-entry vocabulary (the fixture's entries first, then words no one answers)."""
    from mmnas_amd.answering import AnswerCredit
    from tests.test_answering_host import PDA, PP, split
    vocab = VOCAB + ['w%d' % i for i in range(3129 - A)]
    q, a = split()
    return AnswerCredit.build(q, a, vocab, lambda s: PP.get(s, s), lambda s: PDA.get(s, s)), vocab


def test_evaluator_matches_the_reference_eval_at_train_vqa_dimensions():
    from mmnas_amd.answering import VqaEvaluator
    net, c = _vqa_case()
    inputs = tuple(T(a).to(DEV) for a in c['inputs'])
    table, vocab = _credit_3129()
    B, W = 64, 2
    # the reference's per-batch path (train_vqa.py:379-393) at world 1: copy back, np.argmax
    flags = [(m, m.training) for m in net.modules()]
    net.eval()
    with torch.no_grad():
        ref_logits = net(inputs)
    for m, t in flags:
        m.training = t
    ref = np.argmax(ref_logits.cpu().data.numpy(), axis=1)
    # this batch as rank 1 of 2 over a 2 * 64 - 1 question subset: positions 1, 3, ..., 127 (127 is the sampler's padding)
    sub = list(range(100, 100 + 2 * B - 1))
    ev = VqaEvaluator(net, table, subset_indices=sub, rank=1, world_size=W)
    out = ev.update(inputs)
    assert net.training and all(m.training for m in net.modules())
    assert np.array_equal(np.argmax(out.cpu().numpy(), 1), ref)
    pred = ev._pred.cpu().numpy()
    cnt = ev._count.cpu().numpy()
    pos = np.arange(1, 2 * B, 2)
    keep = pos < len(sub)
    assert np.array_equal(pred[pos[keep]], ref[keep]) and (cnt[pos[keep]] == 1).all() and cnt[::2].sum() == 0
    k = table.lookup(np.asarray(sub)[pos[keep]], ref[keep])
    assert np.array_equal(ev._credit.cpu().numpy()[pos[keep]], k)
    # rank 0's half (the same batch again, at explicit positions 0, 2, ..., 126) completes the subset
    ev.update(inputs, index=torch.arange(0, 2 * B, 2))
    r = ev.compute()
    assert r['exact']['overall'][1] == len(sub)
    res = [x['answer'] for x in ev.results(vocab)]
    assert res[0::2] == [vocab[i] for i in ref] and res[1::2] == [vocab[i] for i in ref[:B - 1]]


def test_device_answer_targets_equal_the_loader_targets():
    from mmnas_amd import data
    from mmnas_amd.answering import AnsweringError, answer_indices, answer_targets
    a2i = {a: i for i, a in enumerate(cases.LOADER_ANSWERS)}
    sets = list(cases.LOADER_ANSWER_SETS)
    t = answer_targets(answer_indices(sets, a2i).to(DEV), len(a2i))
    assert np.array_equal(t.cpu().numpy(), data.answer_targets(sets, a2i))
    # the fixture's 1200 questions against 3129 entries (every count 0..10), and n = 64
    vocab = VOCAB + ['w%d' % i for i in range(3129 - A)]
    a2i = {s: i for i, s in enumerate(vocab)}
    lists = Z['answers'].tolist()
    ix = answer_indices(lists, a2i, normalize=process_punctuation)
    t = answer_targets(ix.to(DEV), 3129)
    assert np.array_equal(t.cpu().numpy(), data.answer_targets(lists, a2i, normalize=process_punctuation))
    long = [l * 6 + l[:4] for l in lists[:70]]
    ix = answer_indices(long, a2i, normalize=process_punctuation, n=64)
    t = answer_targets(ix.to(DEV), 3129)
    assert np.array_equal(t.cpu().numpy(), data.answer_targets(long, a2i, normalize=process_punctuation))
    bad = ix.clone()
    bad[3, 9] = 3129
    with pytest.raises(AnsweringError, match='index'):
        answer_targets(bad.to(DEV), 3129)


def test_explicit_positions_on_the_device():
    """update(index=...) through the kernel: -1 skips the row, a position past the subset, below -1 or one that would wrap
    into range as int32 sets the index flag, which compute() reports; answer_batch / answer_targets refuse wrapping rows."""
    from mmnas_amd.answering import AnsweringError, VqaEvaluator, answer_batch, answer_targets
    pred = Z['preds'][1]
    net = _Replay(logits_for(pred).to(DEV)).to(DEV)
    ev = VqaEvaluator(net, credit())
    ids = torch.arange(N, device=DEV)
    ev.update((ids, None, None, None, None), index=torch.cat((torch.arange(N - 1), torch.tensor([-1]))).to(DEV))
    with pytest.raises(AnsweringError, match='1 of %d questions never' % N):
        ev.compute()
    ev.update((ids[-1:], None, None, None, None), index=torch.tensor([N - 1], device=DEV))
    r = ev.compute()
    assert r['exact']['overall'] == (int(reference_k()[np.arange(N), pred].sum()), N)
    assert r['overall'] == pred_accuracy(1)['overall']
    for bad in (N, -2, 2 ** 32 + 5, -2 ** 32 + 5):
        ev.reset()
        ev.update((ids, None, None, None, None))
        ev.update((ids[:2], None, None, None, None), index=torch.tensor([5, bad], device=DEV))
        with pytest.raises(AnsweringError, match='index out of range'):
            ev.compute()
    c = credit().to(DEV)
    with pytest.raises(AnsweringError, match='index'):
        answer_batch(torch.zeros(2, A, device=DEV), torch.tensor([0, 2 ** 32 + 1], device=DEV), c)
    with pytest.raises(AnsweringError, match='index'):
        answer_targets(torch.tensor([[0, 2 ** 32 + 1]], device=DEV), A)
