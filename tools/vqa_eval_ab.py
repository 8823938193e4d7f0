"""A/B of the VQA evaluation and soft targets at the train_vqa batch (B = 64, 3129 answers), random inputs.

  eval     A  the reference's per-batch path at world 1 (train_vqa.py:379-393) on logits that are on the device: the
              device->host copy and np.argmax;
           B  what VqaEvaluator.update adds behind the shared forward: one mmnas_vqa_answer launch writing pred / credit /
              count into the device buffers (no host synchronisation; timed as --inner back-to-back calls closed by one
              synchronize).
  targets  A  data.answer_targets (the loader's proc_ans restated, dense [64, 3129] float32 rows) + the host->device copy;
           B  answer_indices on the host, the [64, 10] int32 upload and answer_targets on the device (check=False).

A and B alternate, --rounds each; the median microseconds per batch of each and their ratio are printed, then one JSON line.

  python tools/vqa_eval_ab.py [--rounds 7 --inner 50]

--host-split instead times the host side of a VQA-v2-val-sized synthetic split (214 354 questions of 10 answers, 3129
vocabulary entries), with the reference checkout's normalisers (--reference, default $MMNAS_REFERENCE): AnswerCredit.build, and
the reference's own per-epoch evaluation (result JSON dump, VQA / loadRes reload, VQAEval.evaluate).  No GPU is used.

  python tools/vqa_eval_ab.py --host-split [--reference DIR]
"""
import argparse
import importlib.util
import io
import json
import os
import statistics
import sys
import tempfile
import time
from contextlib import redirect_stdout

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_split(nq, A, seed=3):
    """A split shaped like VQA v2 val: 10 answers per question drawn around a per-question favourite (with case and
    punctuation variants and out-of-vocabulary strings), three answer types, 65 question types."""
    rs = np.random.RandomState(seed)
    words = ['ans%d' % i for i in range(A - 4)] + ['two', 'a dog', 't-shirt', 'yes.']
    variants = lambda w: [w, w.upper(), w + '.', w + '!', 'the ' + w, 'oov' + w]     # noqa: E731
    questions, annotations = [], []
    fav = rs.randint(0, A, nq)
    kinds = rs.randint(0, 10, (nq, 10))
    alt = rs.randint(0, A, (nq, 10))
    var = rs.randint(0, 6, (nq, 10))
    at = rs.randint(0, 3, nq)
    qt = rs.randint(0, 65, nq)
    for q in range(nq):
        ans = []
        for j in range(10):
            w = words[fav[q]] if kinds[q, j] < 6 else words[alt[q, j]]
            ans.append(w if kinds[q, j] < 8 else variants(w)[var[q, j]])
        questions.append({'question_id': 1000 + q, 'image_id': q // 5, 'question': 'q?'})
        annotations.append({'question_id': 1000 + q, 'image_id': q // 5, 'question_type': 'qt%d' % qt[q],
                            'answer_type': ('yes/no', 'number', 'other')[at[q]],
                            'answers': [{'answer': a, 'answer_confidence': 'yes', 'answer_id': j + 1}
                                        for j, a in enumerate(ans)]})
    return questions, annotations, words


def _module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_split(args):
    from mmnas_amd.answering import AnswerCredit
    ref = args.reference
    if not ref or not os.path.isdir(os.path.join(ref, 'mmnas', 'utils')):
        sys.exit('--host-split needs the reference checkout (--reference or MMNAS_REFERENCE): the normalisers and VQAEval')
    sys.dont_write_bytecode = True
    u = os.path.join(ref, 'mmnas', 'utils')
    punct = _module(os.path.join(u, 'answer_punct.py'), 'ref_answer_punct')
    vqa_mod = _module(os.path.join(u, 'vqa.py'), 'ref_vqa')
    eval_mod = _module(os.path.join(u, 'vqaEval.py'), 'ref_vqa_eval')
    t0 = time.perf_counter()
    questions, annotations, vocab = synthetic_split(args.questions, args.answers)
    t_gen = time.perf_counter() - t0
    builds = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        table = AnswerCredit.build(questions, annotations, vocab, punct.process_punctuation, punct.process_digit_article)
        builds.append(time.perf_counter() - t0)
    pred = np.random.RandomState(4).randint(0, args.answers, args.questions)
    meta = {'info': {}, 'task_type': 'Open-Ended', 'data_type': 'mscoco', 'data_subtype': 'val2014', 'license': {}}
    evals, epochs, acc = [], [], None
    with tempfile.TemporaryDirectory() as d:
        qf, af, rf = (os.path.join(d, n) for n in ('q.json', 'a.json', 'r.json'))
        with open(qf, 'w') as f:
            json.dump(dict(meta, questions=questions), f)
        with open(af, 'w') as f:
            json.dump(dict(meta, annotations=annotations), f)
        for _ in range(args.rounds):
            with redirect_stdout(io.StringIO()):
                t0 = time.perf_counter()
                with open(rf, 'w') as f:      # train_vqa.py:417-434
                    json.dump([{'answer': vocab[p], 'question_id': q['question_id']} for p, q in zip(pred, questions)], f)
                vqa = vqa_mod.VQA(af, qf)
                res = vqa.loadRes(rf, qf)
                ev = eval_mod.VQAEval(vqa, res, n=2)
                t1 = time.perf_counter()
                ev.evaluate()
                t2 = time.perf_counter()
            evals.append(t2 - t1)
            epochs.append(t2 - t0)
            acc = ev.accuracy['overall']
    # the table gives the same overall accuracy
    k = table.lookup(np.arange(args.questions), pred)
    mine = round(100 * float(k.sum()) / (3 * table.num_answers * args.questions), 2)
    assert mine == acc, (mine, acc)
    med = lambda v: statistics.median(v)    # noqa: E731
    print('synthetic split: %d questions x 10 answers, %d vocabulary entries (generated in %.1f s)' % (args.questions, args.answers,
                                                                                                      t_gen))
    print('  AnswerCredit.build (host, once per split)       median %.2f s  (%d entries)' % (med(builds), len(table.k)))
    print('  VQAEval.evaluate() (host, per epoch)            median %.2f s' % med(evals))
    print('  dump + reload + loadRes + evaluate (per epoch)  median %.2f s' % med(epochs))
    print(json.dumps(dict(tool='vqa_eval_ab', mode='host_split', questions=args.questions, answers=args.answers, rounds=args.rounds,
                          build_s=builds, vqaeval_evaluate_s=evals, vqaeval_epoch_s=epochs, overall=acc)))


def device_ab(args):
    from mmnas_amd import answering as Q
    from mmnas_amd import data
    dev = 'cuda:0'
    B, A, N = args.batch, args.answers, 64 * args.batch
    rs = np.random.RandomState(5)
    questions, annotations, vocab = synthetic_split(N, A)
    ident = lambda s: s     # noqa: E731   (the synthetic vocabulary needs no normalising for this timing)
    table = Q.AnswerCredit.build(questions, annotations, vocab, ident, ident).to(dev)
    logits = torch.from_numpy(rs.standard_normal((B, A)).astype(np.float32)).to(dev)
    pred = torch.zeros(N, dtype=torch.int64, device=dev)
    cr = torch.zeros(N, dtype=torch.int32, device=dev)
    cnt = torch.zeros(N, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    a2i = {w: i for i, w in enumerate(vocab)}
    lists = [[x['answer'] for x in a['answers']] for a in annotations[:B]]

    def eval_a():
        return np.argmax(logits.cpu().data.numpy(), axis=1)

    def eval_b():
        for i in range(args.inner):
            Q._launch_answer(logits, A, A, None, (i % 64) * B, 1, N, None, table, pred, cr, cnt, flag)
        torch.cuda.synchronize()

    def tgt_a():
        t = torch.from_numpy(data.answer_targets(lists, a2i)).to(dev)
        torch.cuda.synchronize()
        return t

    def tgt_b():
        for _ in range(args.inner):
            t = Q.answer_targets(Q.answer_indices(lists, a2i).to(dev), A, check=False)
        torch.cuda.synchronize()
        return t

    # agreement first
    ref = eval_a()
    Q._launch_answer(logits, A, A, None, 0, 1, N, None, table, pred, cr, cnt, flag)
    assert np.array_equal(pred[:B].cpu().numpy(), ref) and int(flag.item()) == 0
    assert np.array_equal(cr[:B].cpu().numpy(), table.lookup(np.arange(B), ref))
    assert torch.equal(tgt_a(), tgt_b())
    for f in (eval_a, eval_b, tgt_a, tgt_b):   # warm-up
        f()
    res = {'eval_ref_us': [], 'eval_dev_us': [], 'targets_ref_us': [], 'targets_dev_us': []}
    for _ in range(args.rounds):
        for key, f, reps in (('eval_ref_us', eval_a, 1), ('eval_dev_us', eval_b, args.inner), ('targets_ref_us', tgt_a, 1),
                             ('targets_dev_us', tgt_b, args.inner)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            res[key].append((time.perf_counter() - t0) * 1e6 / reps)
    med = {k: statistics.median(v) for k, v in res.items()}
    print('B=%d A=%d, median of %d alternating rounds (us per batch):' % (B, A, args.rounds))
    print('  eval     reference host %9.1f   device %7.1f   ratio %6.1fx' % (med['eval_ref_us'], med['eval_dev_us'],
                                                                          med['eval_ref_us'] / med['eval_dev_us']))
    print('  targets  reference host %9.1f   device %7.1f   ratio %6.1fx' % (med['targets_ref_us'], med['targets_dev_us'],
                                                                          med['targets_ref_us'] / med['targets_dev_us']))
    rec = dict(tool='vqa_eval_ab', B=B, A=A, rounds=args.rounds, inner=args.inner, median_us=med,
               eval_ratio=med['eval_ref_us'] / med['eval_dev_us'], targets_ratio=med['targets_ref_us'] / med['targets_dev_us'],
               all_us={k: [round(x, 2) for x in v] for k, v in res.items()}, device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--answers', type=int, default=3129)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--host-split', action='store_true')
    ap.add_argument('--questions', type=int, default=214354)
    ap.add_argument('--reference', default=os.environ.get('MMNAS_REFERENCE'))
    args = ap.parse_args()
    if args.host_split:
        host_split(args)
    else:
        device_ab(args)


if __name__ == '__main__':
    main()
