"""CPU checks of mmnas_amd.answering: the credit table against the official VQA evaluation's own per-question accuracies
(tests/golden/vqa.npz, make_golden_vqa.py), VqaEvaluator.compute() against VQAEval's accuracy dicts, the numpy argmax and soft
targets against np.argmax and data.answer_targets, refusals, the sampler's positions over two and three gloo ranks, results()
order, the new entry points' host-side validation under the AddressSanitizer build, and (opt-in) the fixture's regeneration."""
import json
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.golden import cases
from tests.util import REPO, load

T = torch.from_numpy
Z = load('vqa.npz')
N, A = Z['acc'].shape
NANS = Z['answers'].shape[1]
PP = dict(zip(Z['pp_in'].tolist(), Z['pp_out'].tolist()))
PDA = dict(zip(Z['pda_in'].tolist(), Z['pda_out'].tolist()))
VOCAB = Z['vocab'].tolist()


def process_punctuation(s):
    return PP[s]


def process_digit_article(s):
    return PDA[s]


def split():
    """(questions in the loader's order, annotations in the file's order) as the reference's JSON holds them."""
    qids = Z['question_id'].tolist()
    questions = [{'question_id': q, 'image_id': int(i), 'question': 'q%d?' % k}
                 for k, (q, i) in enumerate(zip(qids, Z['image_id'].tolist()))]
    row = {q: k for k, q in enumerate(qids)}
    anns = []
    for q in Z['anno_order'].tolist():
        k = row[q]
        anns.append({'question_id': q, 'image_id': int(Z['image_id'][k]), 'question_type': str(Z['question_type'][k]),
                     'answer_type': str(Z['answer_type'][k]),
                     'answers': [{'answer': str(a), 'answer_confidence': str(c), 'answer_id': int(i)}
                                 for a, c, i in zip(Z['answers'][k], Z['answer_confidence'][k], Z['answer_id'][k])]})
    return questions, anns


def build_credit():
    from mmnas_amd.answering import AnswerCredit
    q, a = split()
    return AnswerCredit.build(q, a, VOCAB, process_punctuation, process_digit_article)


CREDIT = None


def credit():
    global CREDIT
    if CREDIT is None:
        CREDIT = build_credit()
    return CREDIT


def reference_k():
    """The fixture's avgGTAcc as integers k = 3n * acc (each is a sum of floats min(1, m / 3): within round-off of k / 3n)."""
    k = np.rint(Z['acc'] * 3 * NANS).astype(np.int64)
    assert np.abs(Z['acc'] * 3 * NANS - k).max() < 1e-9
    return k


def dense(c):
    q = np.repeat(np.arange(N), A)
    v = np.tile(np.arange(A), N)
    return c.lookup(q, v).reshape(N, A).astype(np.int64)


def pred_accuracy(p):
    pre = 'pred%d|' % p
    d = {'overall': float(Z[pre + 'overall'])}
    for kind in ('perQuestionType', 'perAnswerType'):
        d[kind] = dict(zip(Z[pre + kind + '_names'].tolist(), Z[pre + kind + '_values'].tolist()))
    return d


# ---- the credit table ------------------------------------------------------------------------------------------------------------
def test_credit_table_equals_the_reference_per_question_accuracy():
    from fractions import Fraction
    c = credit()
    assert c.num_questions == N and c.num_vocab == A and c.num_answers == NANS == 10
    k = dense(c)
    kr = reference_k()
    assert np.array_equal(k, kr)
    # as rationals: k / 3n is the reference's float up to its summation round-off, and nothing else
    for q, v in zip(*np.nonzero(k)):
        assert abs(Fraction(int(k[q, v]), 3 * NANS) - Fraction(float(Z['acc'][q, v]))) < Fraction(1, 10 ** 12)
    rp = c.row_ptr.numpy()
    assert rp[0] == 0 and rp[-1] == len(c.col) and (np.diff(rp) >= 0).all()
    assert (c.k.numpy() > 0).all() and (c.k.numpy() <= 3 * NANS).all()
    for q in range(N):     # columns ascending and distinct within a row
        assert (np.diff(c.col.numpy()[rp[q]:rp[q + 1]]) > 0).all()
    assert c.question_id.numpy().tolist() == Z['question_id'].tolist()
    assert [c.ans_type_names[i] for i in c.ans_type.numpy()] == Z['answer_type'].tolist()
    assert [c.ques_type_names[i] for i in c.ques_type.numpy()] == Z['question_type'].tolist()


def test_fixture_covers_the_quirks():
    k = reference_k()
    v = {s: VOCAB.index(s) for s in ('2', 'two', 'Two', 'dog', 'a dog', 't-shirt', 'tshirt', '1,000', '1000', 'yes', 'yes.',
                                     'red', 'red\t', 'blue', 'blue ', 'Yes')}
    ans = Z['answers']
    # entries that normalise alike score alike
    for a, b in (('2', 'two'), ('2', 'Two'), ('dog', 'a dog'), ('1,000', '1000'), ('yes', 'yes.'), ('yes', 'Yes'),
                 ('red', 'red\t'), ('blue', 'blue ')):
        assert np.array_equal(k[:, v[a]], k[:, v[b]]), (a, b)
    # a ground truth 'two' is never lower-cased nor mapped to '2': predicting 'two' (-> '2') does not match it
    only_two = np.array([set(r) == {'two'} for r in ans.tolist()])
    assert only_two.any() and not k[only_two, v['two']].any()
    # 't-shirt' unanimous: no punctuation pass on the ground truth, so the prediction ('t shirt') misses; with several
    # distinct raw answers the ground truth becomes 't shirt' and it matches
    uni = np.array([set(r) == {'t-shirt'} for r in ans.tolist()])
    several = np.array([('t-shirt' in r) and len(set(r)) > 1 for r in ans.tolist()])
    assert uni.any() and not k[uni, v['t-shirt']].any()
    assert several.any() and k[several, v['t-shirt']].all()
    assert not k[uni, v['tshirt']].any()
    # duplicated answer dicts drop out together: 4 x dog, 3 x 'a dog', 3 x cat with ids 1 / 2 / 3
    dup = np.array([r.tolist() == ['dog'] * 4 + ['a dog'] * 3 + ['cat'] * 3 for r in ans])
    assert dup.any()
    # dog: the 4 'dog' dicts see no other matching dict (equal dicts are excluded), the 6 others see 4 -> 6 * 3
    assert (k[dup, v['dog']] == 18).all()
    # answers outside the vocabulary: some questions give no credit to any entry
    assert (~k.any(1)).any()


def test_build_refusals():
    from mmnas_amd.answering import AnswerCredit
    q, a = split()
    args = (VOCAB, process_punctuation, process_digit_article)
    with pytest.raises(ValueError, match='empty'):
        AnswerCredit.build(q, a, [], process_punctuation, process_digit_article)
    with pytest.raises(ValueError, match='duplicate'):
        AnswerCredit.build(q + q[:1], a, *args)
    a2 = [dict(x) for x in a]
    a2[5] = dict(a2[5], answers=a2[5]['answers'][:9])
    with pytest.raises(ValueError, match='answers'):
        AnswerCredit.build(q, a2, *args)
    with pytest.raises(ValueError, match='no annotation'):
        AnswerCredit.build(q + [{'question_id': -7}], a, *args)
    # the file dicts and a JSON-style ix_to_ans (string keys) are accepted
    c = AnswerCredit.build({'questions': q[:50]}, {'annotations': a}, {str(i): s for i, s in enumerate(VOCAB)},
                           process_punctuation, process_digit_article)
    assert np.array_equal(c.lookup(np.repeat(np.arange(50), A), np.tile(np.arange(A), 50)), reference_k()[:50].reshape(-1))


# ---- one batch on the host -------------------------------------------------------------------------------------------------------
def test_answer_batch_fallback_is_np_argmax():
    from mmnas_amd.answering import AnsweringError, answer_batch
    rs = np.random.RandomState(3)
    x = rs.standard_normal((37, A)).astype(np.float32)
    x[1, [5, 9, 40]] = 7.0                    # ties: the lowest index
    x[2] = -np.inf                            # all -inf: index 0
    x[3, 11] = np.inf
    x[3, 70] = np.inf                         # +inf ties
    x[4, :] = 0.0
    x[5, 60:] = np.inf
    big = np.concatenate((x, rs.standard_normal((37, 13)).astype(np.float32)), 1)   # a row slice of a wider tensor
    c = credit()
    idx = rs.randint(0, N, 37)
    idx[7] = -1
    for t in (T(x), T(big)[:, :A]):
        r = answer_batch(t, T(idx), c)
        assert np.array_equal(r['pred'].numpy(), np.argmax(x, 1))
        k = reference_k()
        want = np.where(idx >= 0, k[np.maximum(idx, 0), np.argmax(x, 1)], -1)
        assert np.array_equal(r['credit'].numpy(), want)
    assert answer_batch(T(x))['credit'] is None
    y = x.copy()
    y[9, 3] = np.nan
    with pytest.raises(AnsweringError, match='NaN'):
        answer_batch(T(y))
    for bad in (N, -2):
        i2 = idx.copy()
        i2[0] = bad
        with pytest.raises(AnsweringError, match='index'):
            answer_batch(T(x), T(i2), c)
    with pytest.raises(TypeError):
        answer_batch(T(x).double())
    with pytest.raises(ValueError):
        answer_batch(T(x[:, :5].copy()), T(idx), c)      # vocabulary size mismatch
    with pytest.raises(ValueError):
        answer_batch(T(x), T(idx[:5]), c)


# ---- soft targets ----------------------------------------------------------------------------------------------------------------
def test_answer_targets_fallback_equals_the_loader_targets():
    from mmnas_amd import data
    from mmnas_amd.answering import AnsweringError, answer_indices, answer_targets
    a2i = {a: i for i, a in enumerate(cases.LOADER_ANSWERS)}
    sets = list(cases.LOADER_ANSWER_SETS)
    ix = answer_indices(sets, a2i)
    assert ix.dtype == torch.int32 and ix.shape == (len(sets), 10)
    t = answer_targets(ix, len(a2i))
    assert t.dtype == torch.float32
    assert np.array_equal(t.numpy(), data.answer_targets(sets, a2i))
    up = [[a.upper() for a in s] for s in sets]
    ix = answer_indices(up, a2i, normalize=str.lower, n=12)
    assert np.array_equal(answer_targets(ix, len(a2i)).numpy(), data.answer_targets(up, a2i, normalize=str.lower))
    # the fixture's answers through its own normaliser: every count 0..10
    a2i = {s: i for i, s in enumerate(VOCAB)}
    lists = Z['answers'].tolist()
    ix = answer_indices(lists, a2i, normalize=process_punctuation)
    assert np.array_equal(answer_targets(ix, A).numpy(), data.answer_targets(lists, a2i, normalize=process_punctuation))
    with pytest.raises(ValueError):
        answer_indices([['yes'] * 11], a2i)
    for bad in (A, -2):
        ix2 = ix.clone()
        ix2[3, 4] = bad
        with pytest.raises(AnsweringError, match='index'):
            answer_targets(ix2, A)


# ---- VqaEvaluator on the CPU -----------------------------------------------------------------------------------------------------
class _Replay(torch.nn.Module):
    """A stand-in VQA network for host tests: returns recorded logits for the sample ids it is given."""
    TASK = 'vqa'

    def __init__(self, logits):
        super().__init__()
        self.proj = torch.nn.Linear(4, 4)
        self.logits = logits

    def forward(self, inputs):
        return torch.index_select(self.logits, 0, inputs[0])


def logits_for(pred, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((len(pred), A)).astype(np.float32)
    x[np.arange(len(pred)), pred] = 10.0
    return T(x)


def sampler_positions(n, world, rank):
    """SubsetDistributedSampler (shuffle off): rank's positions, the wrap-around padding included."""
    per = -(-n // world)
    idx = list(range(n))
    idx += idx[:per * world - n]
    return idx[rank::world]


def _run(ev, n, world, rank, bs=64):
    pos = sampler_positions(n, world, rank)
    for s in range(0, len(pos), bs):
        ev.update((torch.tensor(pos[s:s + bs]), None, None, None, None))


@pytest.mark.parametrize('p', range(int(Z['n_preds'])))
def test_compute_reproduces_vqaeval(p):
    from mmnas_amd.answering import VqaEvaluator
    pred = Z['preds'][p]
    net = _Replay(logits_for(pred, p))
    net.train()
    ev = VqaEvaluator(net, credit())
    _run(ev, N, 1, 0, bs=100)
    r = ev.compute()
    ref = pred_accuracy(p)
    assert r['overall'] == ref['overall']
    assert r['perQuestionType'] == ref['perQuestionType']
    assert r['perAnswerType'] == ref['perAnswerType']
    K, C = r['exact']['overall']
    assert C == N and K == int(reference_k()[np.arange(N), pred].sum()) and r['exact']['scale'] == 30
    assert net.training and all(m.training for m in net.modules())
    res = ev.results(VOCAB)
    assert [x['question_id'] for x in res] == Z['question_id'].tolist()
    assert [x['answer'] for x in res] == [VOCAB[i] for i in pred]


def test_evaluator_subset_padding_and_coverage():
    from mmnas_amd.answering import AnsweringError, VqaEvaluator
    pred = Z['preds'][1]
    rs = np.random.RandomState(4)
    sub = sorted(rs.choice(N, 301, replace=False).tolist())
    net = _Replay(logits_for(pred)[sub])     # sample ids = positions in the subset
    ev = VqaEvaluator(net, credit(), subset_indices=sub)
    _run(ev, len(sub), 1, 0, bs=64)
    r = ev.compute()
    k = reference_k()[sub, pred[sub]]
    assert r['exact']['overall'] == (int(k.sum()), len(sub))
    at = Z['answer_type'][sub]
    for name, (kk, cc) in r['exact']['perAnswerType'].items():
        assert cc == int((at == name).sum()) and kk == int(k[at == name].sum())
    assert [x['question_id'] for x in ev.results(VOCAB)] == Z['question_id'][sub].tolist()
    # never / twice
    ev.reset()
    ev.update((torch.arange(300), None, None, None, None))
    with pytest.raises(AnsweringError, match='1 of 301 questions never'):
        ev.compute()
    ev.update((torch.tensor([300, 299]), None, None, None, None), index=torch.tensor([300, 299]))
    with pytest.raises(AnsweringError, match='1 more than once'):
        ev.compute()
    ev.reset()
    ev.update((torch.arange(301), None, None, None, None), index=torch.cat((torch.arange(300), torch.tensor([-1]))))
    with pytest.raises(AnsweringError, match='never'):
        ev.compute()
    ev.update((torch.tensor([300]), None, None, None, None), index=torch.tensor([300]))
    assert ev.compute()['exact']['overall'] == (int(k.sum()), len(sub))
    ev.reset()
    with pytest.raises(AnsweringError, match='index'):
        ev.update((torch.tensor([0]), None, None, None, None), index=torch.tensor([301]))
        ev.compute()
    # int64 positions that would wrap into range as int32, and positions below -1, are index errors
    for bad in (2 ** 32 + 5, -2 ** 32 + 5, -3):
        ev.reset()
        ev.update((torch.arange(301), None, None, None, None))
        ev.update((torch.tensor([0]), None, None, None, None), index=torch.tensor([bad]))
        with pytest.raises(AnsweringError, match='index'):
            ev.compute()


def test_evaluator_refusals_and_test_dev_results():
    from mmnas_amd.answering import AnsweringError, VqaEvaluator
    with pytest.raises(ValueError, match='VQA'):
        VqaEvaluator(torch.nn.Linear(2, 2), credit())
    x = logits_for(Z['preds'][0])
    with pytest.raises(ValueError, match='question_ids'):
        VqaEvaluator(_Replay(x))
    with pytest.raises(ValueError, match='subset'):
        VqaEvaluator(_Replay(x), credit(), subset_indices=[0, N])
    # no annotations (test-dev): results only
    ids = Z['question_id'][:40]
    ev = VqaEvaluator(_Replay(x[:40]), question_ids=ids, rank=1, world_size=3)
    for pos in np.array_split(np.array(sampler_positions(40, 3, 1)), 3):
        ev.update((torch.from_numpy(pos), None, None, None, None))
    with pytest.raises(AnsweringError, match='never'):     # ranks 0 and 2 are missing
        ev.results(VOCAB)
    ev = VqaEvaluator(_Replay(x[:40]), question_ids=ids)
    ev.update((torch.arange(40), None, None, None, None))
    assert ev.results(VOCAB) == [{'answer': VOCAB[int(a)], 'question_id': int(q)}
                                 for a, q in zip(Z['preds'][0][:40], ids)]
    with pytest.raises(ValueError, match='credit'):
        ev.compute()
    y = x[:40].clone()
    y[3, 5] = float('nan')
    ev = VqaEvaluator(_Replay(y), question_ids=ids)
    ev.update((torch.arange(40), None, None, None, None))
    with pytest.raises(AnsweringError, match='NaN'):
        ev.results(VOCAB)


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_rank(rank, world, port, out, mode):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from mmnas_amd.answering import AnsweringError, VqaEvaluator
        n = N - 7      # not a multiple of 2 or 3: the sampler pads
        pred = Z['preds'][2][:n]
        x = logits_for(pred, 9)
        if mode in ('nan', 'both'):     # a diverged model: every row of every rank holds a NaN
            x[:, 3] = float('nan')
        ev = VqaEvaluator(_Replay(x), credit(), subset_indices=list(range(n)))
        pos = sampler_positions(n, world, rank)
        if mode == 'never' and rank == world - 1:
            pos = pos[:-3]
        for s in range(0, len(pos), 50):
            ev.update((torch.tensor(pos[s:s + 50]), None, None, None, None))
        if mode == 'twice' and rank == 0:
            ev.update((torch.tensor([1]), None, None, None, None), index=torch.tensor([1]))
        if mode in ('index', 'both'):   # every rank: a position past the subset
            ev.update((torch.tensor([1]), None, None, None, None), index=torch.tensor([n + rank]))
        try:
            r = ev.compute()
            r['results'] = ev.results(VOCAB)
        except AnsweringError as e:
            r = {'error': str(e)}
        with open(os.path.join(out, 'rank%d.json' % rank), 'w') as f:
            json.dump(r, f)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_gloo_ranks_equal_one_rank(tmp_path, world):
    from mmnas_amd.answering import VqaEvaluator
    n = N - 7
    pred = Z['preds'][2][:n]
    ev = VqaEvaluator(_Replay(logits_for(pred, 9)), credit(), subset_indices=list(range(n)))
    _run(ev, n, 1, 0)
    one = json.loads(json.dumps(ev.compute()))
    one['results'] = ev.results(VOCAB)
    for mode in ('ok', 'never', 'twice'):
        d = tmp_path / mode
        d.mkdir()
        mp.spawn(_gloo_rank, args=(world, _port(), str(d), mode), nprocs=world, join=True)
        for rank in range(world):
            with open(os.path.join(str(d), 'rank%d.json' % rank)) as f:
                got = json.load(f)
            if mode == 'ok':
                assert got == one
            else:
                assert ('never' if mode == 'never' else 'more than once') in got.get('error', '')


# ---- the new entry points' host-side validation under the AddressSanitizer build ------------------------------------------------
ASAN_DRIVER = r"""
import ctypes as C, sys
sys.path.insert(0, %r)
from mmnas_amd import _lib as L
l = L.lib()
buf = (C.c_double * 64)()
p = C.cast(buf, C.c_void_p).value
E_SHAPE, E_ARG = -1, -2
assert l.mmnas_vqa_answer(p, -1, 10, 10, None, 0, 1, 4, None, p, p, p, 4, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vqa_answer(p, 4, 0, 10, None, 0, 1, 4, None, p, p, p, 4, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vqa_answer(p, 4, 10, 9, None, 0, 1, 4, None, p, p, p, 4, p, p, p, p, None) == E_SHAPE
assert l.mmnas_vqa_answer(p, 4, 10, 10, None, 0, 1, 4, None, None, p, p, 4, p, p, p, p, None) == E_ARG
assert b'vqa_answer: credit needs' in l.mmnas_last_error()
assert l.mmnas_vqa_answer(p, 4, 10, 10, None, 0, 1, 4, None, p, p, p, 4, None, p, p, p, None) == E_ARG
assert l.mmnas_vqa_answer(p, 0, 10, 10, None, 0, 1, 4, None, p, p, p, 4, p, p, p, p, None) == 0
assert l.mmnas_vqa_accuracy(p, None, p, p, 10, 10, 0, 3, p, p, None) == E_SHAPE
assert l.mmnas_vqa_accuracy(p, None, p, p, 10, 10, 3, 257, p, p, None) == E_SHAPE
assert l.mmnas_vqa_accuracy(p, None, None, p, 10, 10, 3, 3, p, p, None) == E_ARG
assert l.mmnas_vqa_accuracy(p, None, p, p, 0, 10, 3, 3, p, p, None) == 0
assert l.mmnas_vqa_answer_targets(p, 4, 65, 10, p, p, None) == E_SHAPE
assert l.mmnas_vqa_answer_targets(p, 4, 10, 0, p, p, None) == E_SHAPE
assert l.mmnas_vqa_answer_targets(p, 4, 10, 10, None, p, None) == E_ARG
assert l.mmnas_vqa_answer_targets(p, 0, 10, 10, p, p, None) == 0
print('VQA_HOST_OK')
"""


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='hipcc not on PATH')
def test_vqa_entry_points_validate_under_address_sanitizer():
    csrc = os.path.join(REPO, 'mmnas_amd', 'csrc')
    b = subprocess.run(['make', '-C', csrc, 'asan', '-j4'], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    lib = os.path.join(REPO, 'mmnas_amd', 'lib', 'libmmnas_hip_asan.so')
    rt = subprocess.run(['hipcc', '-print-file-name=libclang_rt.asan-x86_64.so'], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(rt) or not os.path.exists(rt):
        pytest.skip('ASan runtime of the ROCm clang not found')
    env = dict(os.environ, LD_PRELOAD=rt, MMNAS_LIB_PATH=lib,
               ASAN_OPTIONS='detect_leaks=0:verify_asan_link_order=0:abort_on_error=1:halt_on_error=1')
    p = subprocess.run([sys.executable, '-c', ASAN_DRIVER % REPO], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and 'VQA_HOST_OK' in p.stdout, (p.stdout[-1500:], p.stderr[-4000:])
    assert 'AddressSanitizer' not in p.stderr, p.stderr[-4000:]


# ---- the fixture's recipe (opt-in: needs the reference checkout) ------------------------------------------------------------------
REF = os.environ.get('MMNAS_REFERENCE', '/root/reference')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'mmnas')) or os.environ.get('MMNAS_REGEN_VQA') != '1',
                    reason='opt-in (MMNAS_REGEN_VQA=1, needs the reference tree)')
def test_vqa_golden_regenerates_bit_exact(tmp_path):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import tests.golden.make_golden_vqa as mg\n"
            "mg.HERE = %r\n"
            "mg.gen_vqa()\n" % (REPO, str(tmp_path)))
    r = subprocess.run([sys.executable, '-c', code], cwd=str(tmp_path), env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    new = np.load(os.path.join(str(tmp_path), 'vqa.npz'))
    assert sorted(new.files) == sorted(Z.files)
    for k in new.files:
        assert np.array_equal(new[k], Z[k]), k


@pytest.mark.parametrize('world', [2, 3, 4])
def test_gloo_error_flags_survive_the_reduction(tmp_path, world):
    """Every rank sets the same error bit: the reduced flags keep each cause, and only it (summed bit masks would carry:
    a NaN on two ranks would read as an index error, on four ranks as nothing)."""
    want = {'nan': ('a NaN logit',), 'index': ('an index out of range',), 'both': ('a NaN logit', 'an index out of range')}
    for mode, msgs in want.items():
        d = tmp_path / mode
        d.mkdir()
        mp.spawn(_gloo_rank, args=(world, _port(), str(d), mode), nprocs=world, join=True)
        for rank in range(world):
            with open(os.path.join(str(d), 'rank%d.json' % rank)) as f:
                err = json.load(f).get('error', '')
            for m in want['both']:
                assert (m in err) == (m in msgs), (mode, rank, err)
