"""VQA (configs[0] / [1], search_vqa / train_vqa) answer accuracy and soft answer targets, on the device.

* AnswerCredit -- built once per split on the host: for every question q and vocabulary entry v the integer credit
  k(q, v) = sum over the n annotator answers i of min(3, #{j : answer j != answer i as dicts, g_j == r(v)}), so that the
  official VQAEval accuracy of predicting v is k / (3 n) (vqaEval.py:68-120), with its quirks: r(v) is the vocabulary string with
  newlines / tabs made blanks, stripped, then process_punctuation and process_digit_article; the ground-truth answers g_j get
  process_punctuation only when the raw answers of the question are not all equal, never process_digit_article, never lower-case.
  Stored as CSR over the questions (only k > 0), with each question's id, answer type and question type.
* answer_batch -- one evaluation batch of train_vqa.py:379-393: pred = argmax of each logit row (np.argmax: the lowest index of
  the maximum) and, given a table, that prediction's credit.
* VqaEvaluator -- the whole evaluation of train_vqa.py:352-490: network forward in eval mode, one kernel per batch writing
  (pred, credit) into device buffers keyed by position in the evaluated subset, compute() all-reducing them once and summing the
  credits by answer and question type into VQAEval.accuracy; results() gives the result list the reference dumps.
* answer_indices / answer_targets -- the loader's proc_ans soft targets (load_data_vqa.py:299-333): the answer strings become
  [B, n] vocabulary indices on the host, the dense [B, A] rows are written on the device.
* soft_accuracy / SoftAccuracyReward -- the soft score of the predicted answer under those targets, target[b, argmax logits[b]],
  and its batch mean as a device scalar (mmnas_vqa_soft_accuracy): the reward of a REINFORCE architecture step.

The answer normalisers are arguments, not part of this package: with the reference checkout, pass
mmnas.utils.answer_punct.process_punctuation / process_digit_article, which use the same tables as VQAEval.

CUDA tensors run the HIP kernels of csrc/answering.hip (mmnas_vqa_answer / mmnas_vqa_accuracy / mmnas_vqa_answer_targets);
CPU tensors run a numpy restatement of the same integer arithmetic (the kernels are checked against it).
"""
import contextlib
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L

__all__ = ['AnswerCredit', 'VqaEvaluator', 'answer_batch', 'answer_indices', 'answer_targets', 'AnsweringError', 'soft_accuracy',
           'SoftAccuracyReward']

MAX_TYPES = 256
MAX_ANSWERS = 64       # annotator answers per question (n)
ERR_NAN, ERR_INDEX = 1, 2
_SCORE = np.array([0.0, 0.3, 0.6, 0.9], np.float32)
_I32_MAX = 2 ** 31 - 1


class AnsweringError(ValueError):
    """Invalid values found in the inputs (a NaN logit, an index out of range), or an evaluation that did not cover every
    question exactly once."""


def _raise_flag(flag, what):
    msgs = []
    if flag & ERR_NAN:
        msgs.append('a NaN logit')
    if flag & ERR_INDEX:
        msgs.append('an index out of range')
    if msgs:
        raise AnsweringError('%s: %s' % (what, ' and '.join(msgs)))


def _vocab(ix_to_ans):
    """ix_to_ans as a list: a list / tuple, or a dict keyed by 0..A-1 (ints or their strings, as JSON leaves them)."""
    if isinstance(ix_to_ans, dict):
        return [ix_to_ans[i] if i in ix_to_ans else ix_to_ans[str(i)] for i in range(len(ix_to_ans))]
    return list(ix_to_ans)


def _narrow(idx, device):
    """The int32 copy of an integer index tensor the kernels take.  A value below -1 or above 2^31 - 1 becomes 2^31 - 1, out of
    range for every kernel (which flags it), instead of wrapping into range; no host synchronisation."""
    idx = idx.to(device)
    if idx.dtype != torch.int32:
        wide = idx.to(torch.int64)
        idx = torch.where((wide < -1) | (wide > _I32_MAX), torch.full_like(wide, _I32_MAX), wide).to(torch.int32)
    return idx.contiguous()


def _items(x, key):
    return x[key] if isinstance(x, dict) else x


# ---- the credit table ------------------------------------------------------------------------------------------------------------
class AnswerCredit:
    """VQAEval's per-question scoring as an integer table.  Fields (torch tensors, on one device):
    row_ptr [N+1] int32, col [E] int32 (vocabulary index, ascending within a row), k [E] int32 (1..3n);
    question_id [N] int64, ans_type [N] int32, ques_type [N] int32; and on the host ans_type_names, ques_type_names,
    num_answers (n, the same for every question), num_vocab (A)."""

    FIELDS = ('row_ptr', 'col', 'k', 'question_id', 'ans_type', 'ques_type')

    def __init__(self, row_ptr, col, k, question_id, ans_type, ques_type, ans_type_names, ques_type_names, num_answers,
                 num_vocab):
        self.row_ptr, self.col, self.k = row_ptr, col, k
        self.question_id, self.ans_type, self.ques_type = question_id, ans_type, ques_type
        self.ans_type_names, self.ques_type_names = list(ans_type_names), list(ques_type_names)
        self.num_answers, self.num_vocab = int(num_answers), int(num_vocab)
        self._keys = None

    @property
    def num_questions(self):
        return int(self.question_id.shape[0])

    @property
    def device(self):
        return self.row_ptr.device

    def to(self, device):
        return AnswerCredit(*(getattr(self, f).to(device) for f in self.FIELDS), self.ans_type_names, self.ques_type_names,
                            self.num_answers, self.num_vocab)

    @classmethod
    def build(cls, questions, annotations, ix_to_ans, process_punctuation, process_digit_article):
        """questions: the split's question dicts in the loader's order (ques_list; or the question file's dict), each with a
        'question_id'; annotations: the annotation dicts (or the annotation file's dict), each with 'question_id', 'answers'
        (a list of answer dicts with an 'answer' string), 'answer_type' and 'question_type'; ix_to_ans: the answer vocabulary.
        Row q of the table is questions[q].  Raises ValueError for input the integer form cannot represent exactly: an empty
        vocabulary, a duplicate question id, a question without annotation, or answer counts that vary (or exceed 64)."""
        questions = _items(questions, 'questions')
        annotations = _items(annotations, 'annotations')
        vocab = _vocab(ix_to_ans)
        if not vocab:
            raise ValueError('AnswerCredit: empty answer vocabulary')
        norm = [process_digit_article(process_punctuation(a.replace('\n', ' ').replace('\t', ' ').strip())) for a in vocab]
        by_norm = {}
        for v, r in enumerate(norm):
            by_norm.setdefault(r, []).append(v)
        anns = {}
        for a in annotations:
            anns[a['question_id']] = a
        qids = [q['question_id'] for q in questions]
        if len(set(qids)) != len(qids):
            raise ValueError('AnswerCredit: duplicate question id')
        n = None
        punct = {}
        row_ptr = np.zeros(len(qids) + 1, np.int64)
        cols, ks = [], []
        at_ids, qt_ids, at, qt = {}, {}, [], []
        for q, qid in enumerate(qids):
            ann = anns.get(qid)
            if ann is None:
                raise ValueError('AnswerCredit: question %r has no annotation' % (qid,))
            answers = ann['answers']
            if n is None:
                n = len(answers)
                if not 1 <= n <= MAX_ANSWERS:
                    raise ValueError('AnswerCredit: %d answers per question (1..%d)' % (n, MAX_ANSWERS))
            elif len(answers) != n:
                raise ValueError('AnswerCredit: question %r has %d answers, others %d: the accuracy denominator 3n must be '
                                 'the same for every question' % (qid, len(answers), n))
            raw = [d['answer'] for d in answers]
            if len(set(raw)) > 1:     # vqaEval.py:89-91
                g = []
                for s in raw:
                    p = punct.get(s)
                    if p is None:
                        p = punct[s] = process_punctuation(s)
                    g.append(p)
            else:
                g = raw
            # the answer dicts as VQAEval compares them, after its in-place punctuation pass (item != gtAnsDatum)
            mult = _multiplicities([dict(d, answer=s) for d, s in zip(answers, g)])
            cnt = {}
            for s in g:
                cnt[s] = cnt.get(s, 0) + 1
            row = []
            for r, c in cnt.items():
                vs = by_norm.get(r)
                if not vs:
                    continue
                k = sum(min(3, c - (mult[i] if g[i] == r else 0)) for i in range(n))
                if k > 0:
                    row.extend((v, k) for v in vs)
            row.sort()
            cols.extend(v for v, _ in row)
            ks.extend(k for _, k in row)
            row_ptr[q + 1] = len(cols)
            for name, ids, out in ((ann['answer_type'], at_ids, at), (ann['question_type'], qt_ids, qt)):
                out.append(ids.setdefault(name, len(ids)))
        if len(at_ids) > MAX_TYPES or len(qt_ids) > MAX_TYPES:
            raise ValueError('AnswerCredit: %d answer types, %d question types (at most %d each)' % (len(at_ids), len(qt_ids),
                                                                                                     MAX_TYPES))
        if len(cols) >= 2 ** 31:
            raise ValueError('AnswerCredit: %d table entries' % len(cols))
        T = torch.from_numpy
        return cls(T(row_ptr.astype(np.int32)), T(np.asarray(cols, np.int32)), T(np.asarray(ks, np.int32)),
                   T(np.asarray(qids, np.int64)), T(np.asarray(at, np.int32)), T(np.asarray(qt, np.int32)), list(at_ids),
                   list(qt_ids), n or 0, len(vocab))

    def _host_keys(self):
        """q * A + col over all entries: ascending (rows in order, columns ascending within a row)."""
        if self._keys is None:
            rp = self.row_ptr.cpu().numpy().astype(np.int64)
            rows = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
            self._keys = (rows * self.num_vocab + self.col.cpu().numpy(), self.k.cpu().numpy())
        return self._keys

    def lookup(self, q, v):
        """k(q[i], v[i]) for integer arrays q (question rows) and v (vocabulary indices), on the host (numpy int32)."""
        keys, k = self._host_keys()
        want = np.asarray(q, np.int64) * self.num_vocab + np.asarray(v, np.int64)
        i = np.searchsorted(keys, want)
        hit = i < len(keys)
        hit[hit] = keys[i[hit]] == want[hit]
        return np.where(hit, k[np.minimum(i, len(keys) - 1)] if len(keys) else 0, 0).astype(np.int32)


def _multiplicities(dicts):
    """For each dict, how many of the list are equal to it (itself included)."""
    try:
        keys = [tuple(sorted(d.items())) for d in dicts]
        c = {}
        for key in keys:
            c[key] = c.get(key, 0) + 1
        return [c[key] for key in keys]
    except TypeError:     # unhashable or unorderable values: compare as VQAEval does
        return [sum(1 for e in dicts if e == d) for d in dicts]


# ---- one batch -------------------------------------------------------------------------------------------------------------------
def _logits_rows(logits):
    """(tensor, A, row stride): rows may be a slice of a wider tensor; anything else is made contiguous."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError('logits must be a [B, A] float32 tensor')
    B, A = logits.shape
    if A < 1:
        raise ValueError('logits: A = 0 answers')
    if B <= 1:
        return (logits.contiguous(), A, A)
    if logits.stride(1) != 1 or logits.stride(0) < A:
        logits = logits.contiguous()
    return logits, A, logits.stride(0)


def _table_ptrs(credit):
    if credit is None:
        return None, None, None, 0
    return L.ptr(credit.row_ptr), L.ptr(credit.col), L.ptr(credit.k), credit.num_questions


def _launch_answer(logits, A, ld, slot_idx, slot_base, slot_step, nslots, qmap, credit, pred, credit_out, count, flag):
    B = logits.shape[0]
    if not B:
        return
    rp, col, k, nq = _table_ptrs(credit)
    with torch.cuda.device(logits.device):
        L.check(L.lib().mmnas_vqa_answer(logits.data_ptr(), B, A, ld, L.ptr(slot_idx), int(slot_base), int(slot_step), nslots,
                                         L.ptr(qmap), rp, col, k, nq, L.ptr(pred), L.ptr(credit_out), L.ptr(count), L.ptr(flag),
                                         L.stream()))


def _check_table(credit, A, dev, what):
    if credit is None:
        return
    if not isinstance(credit, AnswerCredit):
        raise TypeError('%s: credit must be an AnswerCredit' % what)
    if credit.num_vocab != A:
        raise ValueError('%s: logits have %d answers, the credit table %d' % (what, A, credit.num_vocab))
    if credit.device != dev:
        raise ValueError('%s: the credit table is on %s, logits on %s (AnswerCredit.to(device))' % (what, credit.device, dev))


def answer_batch(logits, index=None, credit=None, check=True):
    """One evaluation batch: logits [B, A] float32 (row stride may exceed A), index [B] integer question rows of `credit`
    (-1: none).  Returns dict(pred [B] int64 = argmax of each row with np.argmax's tie rule (infinities are ordinary values),
    credit [B] int32 = k(index[b], pred[b]), 0 when not in the table, -1 when index[b] == -1; None without a table).  A NaN
    logit or an index outside -1..N-1 raises AnsweringError; check=False skips reading back the device's error flag (a host
    sync): the call then never synchronises."""
    logits, A, ld = _logits_rows(logits)
    B = logits.shape[0]
    dev = logits.device
    _check_table(credit, A, dev, 'answer_batch')
    if credit is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.shape[0] != B or index.is_floating_point():
            raise ValueError('answer_batch: index must be a [B] integer tensor')
        if index.device != dev:
            raise ValueError('answer_batch: index is on %s, logits on %s' % (index.device, dev))
    if not logits.is_cuda:
        x = logits.detach().numpy()
        if np.isnan(x).any():
            raise AnsweringError('answer_batch: a NaN logit')
        pred = np.argmax(x, axis=1).astype(np.int64) if B else np.zeros(0, np.int64)
        out = None
        if credit is not None:
            q = index.numpy().astype(np.int64)
            if ((q < -1) | (q >= credit.num_questions)).any():
                raise AnsweringError('answer_batch: an index out of range')
            out = np.where(q >= 0, credit.lookup(np.maximum(q, 0), pred), -1).astype(np.int32)
            out = torch.from_numpy(out)
        return dict(pred=torch.from_numpy(pred), credit=out)
    pred = torch.empty(B, dtype=torch.int64, device=dev)
    cr = torch.empty(B, dtype=torch.int32, device=dev) if credit is not None else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    qmap = _narrow(index, dev) if credit is not None else None
    _launch_answer(logits, A, ld, None, 0, 1, B, qmap, credit, pred, cr, None, flag)
    if check:
        _raise_flag(int(flag.item()), 'answer_batch')
    return dict(pred=pred, credit=cr)


def soft_accuracy(logits, target, per_row=False, check=True):
    """The VQA soft score of the predicted answers: logits, target [B, A] float32 (row strides may exceed A), target the loader's
    proc_ans rows.  score[b] = target[b, argmax_a logits[b, a]] (np.argmax's rule: the lowest index of the maximum, infinities
    ordinary values); returns their mean over the batch as a 0-dim tensor on the device of logits, summed in float64 in a
    fixed order -- one launch, nothing read back.  per_row=True returns (mean, score [B]).  A NaN logit raises AnsweringError;
    check=False skips reading back the device's flag (a host sync): the call then never synchronises."""
    logits, A, ld = _logits_rows(logits)
    if not isinstance(target, torch.Tensor) or target.dtype != torch.float32 or tuple(target.shape) != tuple(logits.shape):
        raise TypeError('soft_accuracy: target must be a float32 tensor of the logits\' shape %s' % (tuple(logits.shape),))
    if target.device != logits.device:
        raise ValueError('soft_accuracy: target is on %s, logits on %s' % (target.device, logits.device))
    target, _, ldt = _logits_rows(target)
    B = logits.shape[0]
    if B < 1:
        raise ValueError('soft_accuracy: an empty batch has no mean')
    if not logits.is_cuda:
        x = logits.detach().numpy()
        if np.isnan(x).any():
            raise AnsweringError('soft_accuracy: a NaN logit')
        rows = target.detach().numpy()[np.arange(B), np.argmax(x, axis=1)]
        mean = torch.tensor(np.float32(rows.astype(np.float64).sum() / B))
        return (mean, torch.from_numpy(rows.copy())) if per_row else mean
    dev = logits.device
    out = torch.empty(1, dtype=torch.float32, device=dev)
    rows = torch.empty(B, dtype=torch.float32, device=dev) if per_row else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().mmnas_vqa_soft_accuracy(logits.data_ptr(), ld, target.data_ptr(), ldt, B, A, L.ptr(rows), L.ptr(out),
                                                L.ptr(flag), L.stream()))
    if check:
        _raise_flag(int(flag.item()), 'soft_accuracy')
    return (out[0], rows) if per_row else out[0]


class SoftAccuracyReward:
    """reward(pred, target) of harness.SearchLoop(arch_mode='reinforce'): the batch's VQA soft accuracy as a device scalar,
    never synchronising (a NaN logit gives a NaN-free but meaningless score here; the update's own `err` flag guards the
    rewards it is fed)."""

    def __call__(self, pred, target):
        return soft_accuracy(pred, target, check=False)


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
def _rounded(num, den):
    """VQAEval.setAccuracy's round(100 * sum / count, 2) of the exact fraction."""
    return round(float(Fraction(100 * num, den)), 2)


def _accuracy_dicts(credit, totals):
    """totals: [at sums, at counts, qt sums, qt counts] (ints) -> VQAEval.accuracy plus the exact numbers."""
    na, nt = len(credit.ans_type_names), len(credit.ques_type_names)
    s3 = 3 * credit.num_answers
    at = {credit.ans_type_names[i]: (totals[i], totals[na + i]) for i in range(na) if totals[na + i]}
    qt = {credit.ques_type_names[i]: (totals[2 * na + i], totals[2 * na + nt + i]) for i in range(nt)
          if totals[2 * na + nt + i]}
    K, C = sum(v[0] for v in at.values()), sum(v[1] for v in at.values())
    return {'overall': _rounded(K, s3 * C) if C else float('nan'),
            'perQuestionType': {name: _rounded(k, s3 * c) for name, (k, c) in qt.items()},
            'perAnswerType': {name: _rounded(k, s3 * c) for name, (k, c) in at.items()},
            'exact': {'scale': s3, 'overall': (K, C), 'perQuestionType': qt, 'perAnswerType': at}}


def _totals_np(credit, cr, qrows):
    na, nt = len(credit.ans_type_names), len(credit.ques_type_names)
    a = credit.ans_type.cpu().numpy()[qrows]
    t = credit.ques_type.cpu().numpy()[qrows]
    c = cr.astype(np.int64)

    def hist(ids, m):
        s = np.zeros(m, np.int64)
        np.add.at(s, ids, c)
        return s, np.bincount(ids, minlength=m).astype(np.int64)
    sa, ca = hist(a, na)
    st, ct = hist(t, nt)
    return [int(x) for x in np.concatenate((sa, ca, st, ct))]


# ---- evaluator -------------------------------------------------------------------------------------------------------------------
class VqaEvaluator:
    """The evaluation of train_vqa.py:352-490 (search_vqa.py:401-540) for a VQA network (Net_Full / Net_Search, or DDP around
    one).

    Position p of the evaluated subset (subset_indices, default: every question of `credit` / `question_ids`) is its question
    row subset_indices[p].  Batches follow the reference's SubsetDistributedSampler with shuffle off: rank r's i-th sample is
    position r + world_size * i, and positions past the subset (the sampler's wrap-around padding) are dropped.  update() runs
    the network in eval mode under no_grad (every module's training flag restored afterwards) and launches one kernel that
    writes pred and credit into device buffers of length len(subset): no collective and no host synchronisation per batch.
    compute() all-reduces the buffers over a process group when one is up, raises AnsweringError unless every position was
    written exactly once (the reference's loadRes asserts the same) or a logit was NaN, and returns VQAEval.accuracy
    ({'overall', 'perQuestionType', 'perAnswerType'}, rounded to 2 places) plus 'exact': the integer credit sums and counts
    (accuracy = 100 * credit / (scale * count)).  results(ix_to_ans) gives the [{'answer', 'question_id'}] list the reference
    dumps (train_vqa.py:417-430); without a credit table (test-dev), pass question_ids (the split's, in the loader's order)."""

    def __init__(self, net, credit=None, subset_indices=None, rank=None, world_size=None, question_ids=None):
        if isinstance(net, torch.nn.parallel.DistributedDataParallel):
            net = net.module
        if getattr(net, 'TASK', None) != 'vqa':
            raise ValueError('VqaEvaluator: needs a VQA network, got %s' % type(net).__name__)
        if credit is not None and not isinstance(credit, AnswerCredit):
            raise TypeError('VqaEvaluator: credit must be an AnswerCredit')
        if credit is not None:
            ids = credit.question_id.cpu().numpy()
        elif question_ids is not None:
            ids = np.asarray(question_ids, np.int64).reshape(-1)
        else:
            raise ValueError('VqaEvaluator: give a credit table or, without annotations, the question_ids')
        nq = len(ids)
        sub = np.arange(nq, dtype=np.int64) if subset_indices is None else np.asarray(subset_indices, np.int64).reshape(-1)
        if sub.size and (sub.min() < 0 or sub.max() >= nq):
            raise ValueError('VqaEvaluator: subset index outside 0..%d' % (nq - 1))
        if len(sub) >= 2 ** 31:
            raise ValueError('VqaEvaluator: %d positions' % len(sub))
        import torch.distributed as dist
        up = dist.is_available() and dist.is_initialized()
        self.rank = int(rank if rank is not None else (dist.get_rank() if up else 0))
        self.world_size = int(world_size if world_size is not None else (dist.get_world_size() if up else 1))
        if not 0 <= self.rank < self.world_size:
            raise ValueError('VqaEvaluator: rank %d of world size %d' % (self.rank, self.world_size))
        p = next(iter(net.parameters()), None)
        self.device = p.device if p is not None else torch.device('cpu')
        if credit is not None and credit.device != self.device:
            credit = credit.to(self.device)
        self.net, self.credit = net, credit
        self.question_ids = ids[sub]
        self.N = len(sub)
        self._sub_host = sub
        self._qmap = None if subset_indices is None else torch.from_numpy(sub.astype(np.int32)).to(self.device)
        dev = self.device
        self._pred = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self._credit = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self._count = torch.zeros(self.N, dtype=torch.int32, device=dev)
        self._flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self._seen = 0
        self._reduced = None

    def reset(self):
        for t in (self._pred, self._credit, self._count, self._flag):
            t.zero_()
        self._seen = 0
        self._reduced = None

    @contextlib.contextmanager
    def _eval(self):
        flags = [(m, m.training) for m in self.net.modules()]
        try:
            self.net.eval()
            with torch.no_grad():
                yield
        finally:
            for m, t in flags:
                m.training = t

    def update(self, inputs, index=None):
        """One evaluation batch: inputs = the network's 5-tuple (frcn_feat, bbox_feat, rel_img, ques_ix, rel_ques).  index
        (optional, [B] integer): the samples' positions in the subset instead of the sampler's order (-1: skip the row); the
        sampler counter does not advance then.  Returns the logits.  No host synchronisation on the device."""
        with self._eval():
            logits = self.net(tuple(inputs))
        x, A, ld = _logits_rows(logits)
        B = x.shape[0]
        if x.device != self.device:
            raise ValueError('VqaEvaluator: logits on %s, buffers on %s' % (x.device, self.device))
        _check_table(self.credit, A, self.device, 'VqaEvaluator')
        if index is None:
            base, step, idx = self.rank + self.world_size * self._seen, self.world_size, None
            self._seen += B
        else:
            if not isinstance(index, torch.Tensor) or index.shape != (B,) or index.is_floating_point():
                raise ValueError('VqaEvaluator.update: index must be a [B] integer tensor')
            base, step, idx = 0, 1, _narrow(index, self.device)
        self._reduced = None
        if x.is_cuda:
            _launch_answer(x, A, ld, idx, base, step, self.N, self._qmap, self.credit, self._pred,
                           self._credit if self.credit is not None else None, self._count, self._flag)
            return logits
        self._update_np(x.detach().numpy(), base, step, idx)
        return logits

    def _update_np(self, x, base, step, idx):
        B = x.shape[0]
        slots = np.arange(B, dtype=np.int64) * step + base if idx is None else idx.numpy().astype(np.int64)
        bad = 0
        if (slots < -1).any() or (idx is not None and (slots >= self.N).any()):
            bad |= ERR_INDEX
        keep = (slots >= 0) & (slots < self.N)
        xs = x[keep]
        if np.isnan(xs).any():
            bad |= ERR_NAN
        s = slots[keep]
        pred = np.argmax(xs, axis=1) if len(s) else np.zeros(0, np.int64)
        self._pred.numpy()[s] = pred
        if self.credit is not None:
            self._credit.numpy()[s] = self.credit.lookup(self._sub_host[s], pred)
        np.add.at(self._count.numpy(), s, 1)
        self._flag |= bad

    def _gather(self, group=None):
        """(pred, credit, count) summed over the ranks; raises unless every position was written exactly once.  Each error bit
        is reduced as a count of its own (summed bit masks would carry into each other)."""
        if self._reduced is not None:
            return self._reduced
        bits = torch.cat((self._flag & ERR_NAN, (self._flag & ERR_INDEX) >> 1)).to(torch.int64)
        v = torch.cat((self._pred, self._credit.to(torch.int64), self._count.to(torch.int64), bits))
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            if dist.get_backend(group) == 'gloo':
                v = v.cpu()
            v = v.clone()
            dist.all_reduce(v, group=group)
        N = self.N
        pred, cr, cnt = v[:N], v[N:2 * N], v[2 * N:3 * N]
        nan, index = (int(x) for x in v[3 * N:].tolist())
        _raise_flag((ERR_NAN if nan else 0) | (ERR_INDEX if index else 0), 'VqaEvaluator')
        never, twice = int((cnt == 0).sum()), int((cnt > 1).sum())
        if never or twice:
            raise AnsweringError('VqaEvaluator: %d of %d questions never evaluated, %d more than once' % (never, N, twice))
        self._reduced = (pred, cr)
        return self._reduced

    def compute(self, group=None):
        """VQAEval.accuracy over every update() since construction / reset(), summed over the ranks of `group` (default: the
        default process group) when torch.distributed is initialised."""
        if self.credit is None:
            raise ValueError('VqaEvaluator.compute: no credit table (annotations) to score against')
        pred, cr = self._gather(group)
        c = self.credit
        na, nt = len(c.ans_type_names), len(c.ques_type_names)
        if self.device.type != 'cuda':
            return _accuracy_dicts(c, _totals_np(c, cr.cpu().numpy(), self._sub_host))
        cr = cr.to(device=self.device, dtype=torch.int32).contiguous()
        totals = torch.zeros(2 * (na + nt), dtype=torch.int64, device=self.device)
        flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        if self.N:
            with torch.cuda.device(self.device):
                L.check(L.lib().mmnas_vqa_accuracy(L.ptr(cr), L.ptr(self._qmap), L.ptr(c.ans_type), L.ptr(c.ques_type), self.N,
                                                   c.num_questions, na, nt, L.ptr(totals), L.ptr(flag), L.stream()))
        _raise_flag(int(flag.item()), 'VqaEvaluator.compute')
        return _accuracy_dicts(c, totals.cpu().tolist())

    def results(self, ix_to_ans, group=None):
        """[{'answer': ix_to_ans[pred], 'question_id': id}] in subset order (train_vqa.py:417-430): one device->host copy."""
        pred, _ = self._gather(group)
        vocab = _vocab(ix_to_ans)
        p = pred.cpu().numpy()
        return [{'answer': vocab[int(a)], 'question_id': int(q)} for a, q in zip(p, self.question_ids)]


# ---- soft targets ----------------------------------------------------------------------------------------------------------------
def answer_indices(answer_lists, ans_to_ix, normalize=None, n=10):
    """Host side of the loader's proc_ans: [B, n] int32 vocabulary indices of each question's annotator answers (after
    `normalize`, the loader's preprocess_answer when given), -1 for answers not in the vocabulary and for missing ones."""
    out = np.full((len(answer_lists), n), -1, np.int32)
    for b, answers in enumerate(answer_lists):
        if len(answers) > n:
            raise ValueError('answer_indices: %d answers in row %d (n = %d)' % (len(answers), b, n))
        for j, a in enumerate(answers):
            if normalize is not None:
                a = normalize(a)
            out[b, j] = ans_to_ix.get(a, -1)
    return torch.from_numpy(out)


def answer_targets(ans_ix, num_answers, check=True):
    """The loader's soft targets from answer indices: ans_ix [B, n] integer (-1: none) -> [B, num_answers] float32, each column
    0 / .3 / .6 / .9 / 1 by how often it occurs in the row (bit-equal to data.answer_targets on the same answers).  An index
    outside -1..num_answers-1 raises AnsweringError; check=False skips reading back the device's flag (a host sync)."""
    if not isinstance(ans_ix, torch.Tensor) or ans_ix.dim() != 2 or ans_ix.is_floating_point():
        raise TypeError('answer_targets: ans_ix must be a [B, n] integer tensor')
    B, n = ans_ix.shape
    A = int(num_answers)
    if A < 1 or not 1 <= n <= MAX_ANSWERS:
        raise ValueError('answer_targets: num_answers=%d, n=%d (A >= 1, 1 <= n <= %d)' % (A, n, MAX_ANSWERS))
    if not ans_ix.is_cuda:
        ix = ans_ix.numpy().astype(np.int64)
        if ((ix < -1) | (ix >= A)).any():
            raise AnsweringError('answer_targets: an index out of range')
        out = np.zeros((B, A), np.float32)
        for b in range(B):
            v, c = np.unique(ix[b][ix[b] >= 0], return_counts=True)
            out[b, v] = np.where(c < 4, _SCORE[np.minimum(c, 3)], np.float32(1.0))
        return torch.from_numpy(out)
    dev = ans_ix.device
    ix = _narrow(ans_ix, dev)
    out = torch.empty(B, A, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    if B:
        with torch.cuda.device(dev):
            L.check(L.lib().mmnas_vqa_answer_targets(L.ptr(ix), B, n, A, L.ptr(out), L.ptr(flag), L.stream()))
        if check:
            _raise_flag(int(flag.item()), 'answer_targets')
    return out
