"""Generate tests/golden/vqa.npz: the official VQA evaluation of the *imported reference* (the reference checkout, available in
the build container only) on a synthetic split, for mmnas_amd/answering.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vqa.py

The split (question / annotation JSON written to a temporary directory) has N questions of n = 10 answer dicts each and a
vocabulary of A entries built to hit every quirk of VQAEval.evaluate (vqaEval.py:68-120): 'two' / '2' / 'Two', 'a dog' / 'dog',
't-shirt' with one and with several distinct raw answers, '1,000', 'yes.', tabs and trailing blanks in vocabulary entries,
vocabulary entries that normalise alike, answers outside the vocabulary, and questions whose answer dicts are equal (before or
only after the punctuation pass).  Recorded, with the reference's vqa.py / vqaEval.py / answer_punct.py:

* acc [N, A]: the unrounded avgGTAcc of every (question, vocabulary entry), from setEvalQA of one VQAEval.evaluate() per entry;
* for a few prediction vectors, the accuracy dicts of VQAEval.evaluate() (flattened to name / value arrays);
* the outputs of answer_punct.process_punctuation / process_digit_article for every string the evaluation feeds them, after
  checking that they equal VQAEval's own methods on those strings (so the tests' normalisers are dict lookups).

It asserts that no percentage of those accuracy dicts lies within 1e-9 of a rounding boundary: there, rounding the exact rational and
rounding the reference's float sum could differ.  Only arrays are written (unicode arrays for strings) -- no reference source,
bytecode or pickled object.
"""
import importlib.util
import json
import math
import os
import sys
import tempfile
from types import SimpleNamespace

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('MMNAS_REFERENCE', '/root/reference')

import numpy as np

N_QUESTIONS = 1200
N_ANS = 10

# vocabulary: plain entries, then the quirks (raw strings as ix_to_ans holds them)
VOCAB = (['yes', 'no', 'red', 'blue', 'green', 'white', 'black', 'dog', 'cat', 'frisbee', 'tennis', 'left', 'right', 'kitchen',
          'pizza', 'table', '0', '1', '3', '4', '5', '10', 'wood', 'grass', 'snow', 'water', 'bus', 'train', 'man', 'woman',
          'skateboarding', 'surfing', 'brown', 'orange', 'yellow', 'pink', 'gray', 'sunny', 'night', 'baseball', 'soccer',
          'elephant', 'giraffe', 'horse', 'umbrella', 'car', 'phone', 'laptop', 'bed', 'couch', 'ice cream', 'hot dog',
          'stop sign', 'fire hydrant', "don't know", 'nothing', 'eating', 'sitting', 'standing', 'playing'] +
         ['2', 'two', 'Two', 'a dog', 't-shirt', 'tshirt', '1,000', '1000', 'yes.', 'red\t', 'blue ', ' green', 'none',
          'the cat', 'dont', 'hes', 'left side', 'e-mail', 'ice-cream', 'Yes'])
# answer strings annotators give (beyond the vocabulary): case / punctuation / article variants and out-of-vocabulary words
EXTRA = ['Two', 'two', 'a dog', 'Dog', 'dog!', 'dog?', 't-shirt', 'T-shirt', 't shirt', '1,000', '1000', '1 000', 'yes.', 'Yes',
         'YES', 'yes!', 'red ', ' red', 'none', 'zero', 'the cat', "don't", 'dont', "he's", 'e-mail', 'email', 'ice-cream',
         'xylophone', 'purple', 'maroon', 'nope', 'yeah', '7', 'seven', 'left-side', 'left, side', 'a', 'an', 'the', '',
         '(none)', 'dog, cat', '3.5', '3 .5', 'yes;', 'e mail', 'hot-dog', 'stop-sign']
ANS_TYPES = ['yes/no', 'number', 'other']
QUES_TYPES = ['what is the', 'how many', 'is the', 'what color is the', 'are there', 'what', 'why', 'none of the above',
              'is this a', 'what sport is']


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    u = os.path.join(REF, 'mmnas', 'utils')
    return (_module(os.path.join(u, 'vqa.py'), 'ref_vqa'), _module(os.path.join(u, 'vqaEval.py'), 'ref_vqa_eval'),
            _module(os.path.join(u, 'answer_punct.py'), 'ref_answer_punct'))


# ---- the synthetic split -----------------------------------------------------------------------------------------------------------
def split(rs):
    """(questions, annotations): the question file's list in the loader's order, the annotation list in another order."""
    pool = VOCAB + EXTRA
    qids = rs.choice(10 ** 8, N_QUESTIONS, replace=False).astype(np.int64) + 10 ** 8
    questions, annotations = [], []
    for q in range(N_QUESTIONS):
        kind = q % 12
        if kind == 0:       # unanimous (one distinct raw answer: no punctuation pass)
            answers = [pool[rs.randint(len(pool))]] * N_ANS
        elif kind == 1:     # a few distinct plain answers
            base = [VOCAB[i] for i in rs.randint(0, 60, 3)]
            answers = [base[i] for i in rs.choice(3, N_ANS, p=[0.6, 0.3, 0.1])]
        elif kind == 2:     # the 'two' family
            answers = [['two', '2', 'Two', 'seven', '7'][i] for i in rs.randint(0, 5, N_ANS)]
        elif kind == 3:     # the dog family
            answers = [['a dog', 'dog', 'Dog', 'dog!', 'dog?', 'the cat', 'cat'][i] for i in rs.randint(0, 7, N_ANS)]
        elif kind == 4:     # t-shirt, several distinct raw answers
            answers = [['t-shirt', 'T-shirt', 't shirt', 'tshirt', 'e-mail', 'email', 'e mail'][i] for i in rs.randint(0, 7, N_ANS)]
        elif kind == 5:     # numbers with commas, yes with punctuation
            answers = [['1,000', '1000', '1 000', 'yes.', 'yes', 'Yes', 'yes!', 'YES', 'yes;', '3.5', '3 .5'][i]
                       for i in rs.randint(0, 11, N_ANS)]
        elif kind == 6:     # out of the vocabulary mostly
            answers = [['xylophone', 'purple', 'maroon', 'nope', 'yeah', '', '(none)', 'none', 'zero', '0'][i]
                       for i in rs.randint(0, 10, N_ANS)]
        elif kind == 7:     # t-shirt / tabs / blanks: one distinct raw answer of a punctuated form
            answers = [['t-shirt', 'red ', ' red', 'dog!', '1,000', 'yes.', "don't", 'left-side'][q // 12 % 8]] * N_ANS
        else:               # anything
            answers = [pool[i] for i in rs.randint(0, len(pool), N_ANS)]
        conf = [['yes', 'maybe', 'no'][i] for i in rs.randint(0, 3, N_ANS)]
        ids = list(range(1, N_ANS + 1))
        if q % 50 == 13:     # duplicated answer dicts: equal answer, confidence and id
            answers = ['dog'] * 4 + ['a dog'] * 3 + ['cat'] * 3
            conf = ['yes'] * N_ANS
            ids = [1] * 4 + [2] * 3 + [3] * 3
        if q % 50 == 27:     # dicts equal only after the punctuation pass ('dog!' and 'dog?' both become 'dog')
            answers = ['dog!', 'dog?', 'dog!', 'dog?', 'dog', 'yes', 'yes.', 'two', '2', 'dog']
            conf = ['yes'] * N_ANS
            ids = [5, 5, 5, 6, 6, 7, 7, 8, 9, 9]
        at = ANS_TYPES[rs.randint(len(ANS_TYPES))]
        qt = QUES_TYPES[rs.randint(len(QUES_TYPES))]
        qid = int(qids[q])
        img = int(rs.randint(1, 10 ** 6))
        questions.append({'question_id': qid, 'image_id': img, 'question': 'q%d?' % q})
        annotations.append({'question_id': qid, 'image_id': img, 'question_type': qt, 'answer_type': at,
                            'multiple_choice_answer': answers[0],
                            'answers': [{'answer': a, 'answer_confidence': c, 'answer_id': i}
                                        for a, c, i in zip(answers, conf, ids)]})
    order = rs.permutation(N_QUESTIONS)
    return questions, [annotations[i] for i in order]


def write_files(d, questions, annotations):
    meta = {'info': {'description': 'synthetic'}, 'task_type': 'Open-Ended', 'data_type': 'mscoco', 'data_subtype': 'val2014',
            'license': {'name': 'none'}}
    qf, af = os.path.join(d, 'ques.json'), os.path.join(d, 'anno.json')
    with open(qf, 'w') as f:
        json.dump(dict(meta, questions=questions), f)
    with open(af, 'w') as f:
        json.dump(dict(meta, annotations=annotations), f)
    return qf, af


def evaluate(vqa_mod, eval_mod, d, qf, af, qids, answers, record_qa=False):
    """One VQAEval run of a result list; returns (accuracy dict, {qid: avgGTAcc} or None, unrounded percentages)."""
    rf = os.path.join(d, 'res.json')
    with open(rf, 'w') as f:
        json.dump([{'answer': a, 'question_id': int(q)} for q, a in zip(qids, answers)], f)
    out = sys.stdout
    sys.stdout = open(os.devnull, 'w')
    try:
        vqa = vqa_mod.VQA(af, qf)
        res = vqa.loadRes(rf, qf)
        ev = eval_mod.VQAEval(vqa, res, n=2)
        rec, raw = {}, []
        if record_qa:
            set_qa = ev.setEvalQA

            def wrapped(quesId, acc):
                rec[quesId] = acc
                set_qa(quesId, acc)
            ev.setEvalQA = wrapped
        set_acc = ev.setAccuracy

        def acc_wrapped(accQA, accQuesType, accAnsType):
            raw.append(100 * float(sum(accQA)) / len(accQA))
            for lst in list(accQuesType.values()) + list(accAnsType.values()):
                raw.append(100 * float(sum(lst)) / len(lst))
            set_acc(accQA, accQuesType, accAnsType)
        ev.setAccuracy = acc_wrapped
        ev.evaluate()
    finally:
        sys.stdout.close()
        sys.stdout = out
    return ev.accuracy, (rec if record_qa else None), raw


def on_boundary(raw):
    """Does any unrounded percentage lie within 1e-9 (in units of the last kept place) of a rounding boundary?"""
    return any(abs(x * 100 - math.floor(x * 100) - 0.5) <= 1e-9 for x in raw)


def gen_vqa():
    vqa_mod, eval_mod, punct = load_reference()
    rs = np.random.RandomState(20261016)
    questions, annotations = split(rs)
    qids = [q['question_id'] for q in questions]
    A = len(VOCAB)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        qf, af = write_files(d, questions, annotations)
        acc = np.zeros((N_QUESTIONS, A), np.float64)
        for v in range(A):
            _, rec, _ = evaluate(vqa_mod, eval_mod, d, qf, af, qids, [VOCAB[v]] * N_QUESTIONS, record_qa=True)
            acc[:, v] = [rec[q] for q in qids]
        # prediction vectors: uniform random; the best entry per question (lowest index on a tie); the most frequent raw
        # answer when it is in the vocabulary (else entry 0); the quirk entries cycled
        quirks = [VOCAB.index(s) for s in ('Two', 'two', '2', 't-shirt', 'a dog', 'yes.', '1,000', 'red\t', 'blue ', 'the cat',
                                           'Yes', 'none')]
        ans_of = {a['question_id']: [x['answer'] for x in a['answers']] for a in annotations}
        freq = []
        for q in qids:
            vals, cnt = np.unique(ans_of[q], return_counts=True)
            top = str(vals[np.argmax(cnt)])
            freq.append(VOCAB.index(top) if top in VOCAB else 0)
        preds = np.stack([rs.randint(0, A, N_QUESTIONS), np.argmax(acc, 1), np.asarray(freq),
                          np.asarray([quirks[i % len(quirks)] for i in range(N_QUESTIONS)])]).astype(np.int32)
        for p, pred in enumerate(preds):
            for attempt in range(50):
                accuracy, _, raw = evaluate(vqa_mod, eval_mod, d, qf, af, qids, [VOCAB[i] for i in pred])
                if not on_boundary(raw):
                    break
                pred[rs.randint(N_QUESTIONS)] = rs.randint(A)     # a percentage on a boundary: move one prediction
            assert not on_boundary(raw)
            pre = 'pred%d|' % p
            out[pre + 'overall'] = np.float64(accuracy['overall'])
            for kind in ('perQuestionType', 'perAnswerType'):
                names = sorted(accuracy[kind])
                out[pre + kind + '_names'] = np.asarray(names, dtype=np.str_)
                out[pre + kind + '_values'] = np.asarray([accuracy[kind][k] for k in names], np.float64)
    # the normalisers: answer_punct's functions are VQAEval's methods
    ev = eval_mod.VQAEval(SimpleNamespace(getQuesIds=lambda: []), None)
    pp_in = sorted({a.replace('\n', ' ').replace('\t', ' ').strip() for a in VOCAB} |
                   {x['answer'] for a in annotations for x in a['answers']})
    pp_out = [punct.process_punctuation(s) for s in pp_in]
    assert pp_out == [ev.processPunctuation(s) for s in pp_in]
    pda_in = sorted(set(pp_out))
    pda_out = [punct.process_digit_article(s) for s in pda_in]
    assert pda_out == [ev.processDigitArticle(s) for s in pda_in]
    ann = {a['question_id']: a for a in annotations}
    out.update({
        'vocab': np.asarray(VOCAB, dtype=np.str_),
        'question_id': np.asarray(qids, np.int64),
        'image_id': np.asarray([q['image_id'] for q in questions], np.int64),
        'anno_order': np.asarray([a['question_id'] for a in annotations], np.int64),
        'answers': np.asarray([[x['answer'] for x in ann[q]['answers']] for q in qids], dtype=np.str_),
        'answer_confidence': np.asarray([[x['answer_confidence'] for x in ann[q]['answers']] for q in qids], dtype=np.str_),
        'answer_id': np.asarray([[x['answer_id'] for x in ann[q]['answers']] for q in qids], np.int32),
        'answer_type': np.asarray([ann[q]['answer_type'] for q in qids], dtype=np.str_),
        'question_type': np.asarray([ann[q]['question_type'] for q in qids], dtype=np.str_),
        'acc': acc, 'preds': preds, 'n_preds': np.int32(len(preds)),
        'pp_in': np.asarray(pp_in, dtype=np.str_), 'pp_out': np.asarray(pp_out, dtype=np.str_),
        'pda_in': np.asarray(pda_in, dtype=np.str_), 'pda_out': np.asarray(pda_out, dtype=np.str_)})
    np.savez_compressed(os.path.join(HERE, 'vqa.npz'), **out)
    return out


if __name__ == '__main__':
    gen_vqa()
    print('wrote', os.path.join(HERE, 'vqa.npz'), os.path.getsize(os.path.join(HERE, 'vqa.npz')), 'bytes')
