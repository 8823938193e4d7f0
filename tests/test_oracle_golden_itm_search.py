"""Pin the case of tests/golden/itm_search_traj.npz (the reference's ITM search statements, make_golden_itm_search.py) from the
CPU oracle's side: the generated inputs are the recorded ones, and the oracle restates the first weight step -- three forwards
under the injected sample, BCE_Loss with the positive term twice -- and the two modes share their weight steps."""
import numpy as np
import torch

from oracle import mmnas_oracle as O
from tests.golden import cases
from tests.golden import cases_itm_search as CS
from tests.util import load

T = torch.from_numpy


def test_inputs_and_recorded_plans_are_the_generated_ones():
    npz = load('itm_search_traj.npz')
    c, batches, plans = CS.setup()
    arrs = {}
    for name, pairs in (('t0', batches['train'][0]), ('t1', batches['train'][1]), ('e', batches['eval'])):
        for j, tup in enumerate(pairs):
            for i, a in enumerate(tup):
                arrs['%s%d%d' % (name, j, i)] = a
    assert cases.checksum(arrs) == float(npz['inputs_checksum'])
    assert [str(k) for k in npz['weight_keys']] == list(CS.weight_keys(plans))
    for mode in CS.MODES:
        for r in range(CS.ROUNDS):
            for s, plan in enumerate(plans[mode][r]):
                rec = npz['%s|plan%d_%d' % (mode, r, s)]
                want = [[a[0], i[0] if len(i) == 1 else -1] for a, i in CS.flat(plan)]
                assert rec.tolist() == want
    # live lengths: 7 / 4 / 1 tokens and 9 / 5 / 1 regions in every batch, the one-token caption on every image length
    for pos, neg in batches['train'] + [batches['eval']]:
        assert (pos[3] != 0).sum(1).tolist() == [7, 4, 1]
        assert sorted((neg[3] != 0).sum(1).tolist()) == [1, 4, 7]
        for t in (pos, neg):
            assert (np.abs(t[0]).sum(-1) != 0).sum(1).tolist() == [9, 5, 1]
    # every operator class of the ITM space is sampled within the first round
    seen = {('enc', a[0]) for p in plans['full'][0][:2] for a, _ in p['enc']} | \
           {('dec', a[0]) for p in plans['full'][0][:2] for a, _ in p['dec']}
    assert seen == {('enc', 0), ('enc', 1), ('dec', 0), ('dec', 1), ('dec', 2), ('dec', 3)}


def test_oracle_restates_the_first_weight_step():
    npz = load('itm_search_traj.npz')
    c, batches, plans = CS.setup()
    P = {k: T(v) for k, v in c['P'].items()}
    pos, neg = (tuple(T(a) for a in t) for t in batches['train'][0])
    negc = (pos[0], pos[1], pos[2], neg[3], neg[4])
    negi = (neg[0], neg[1], neg[2], pos[3], pos[4])
    plan = plans['full'][0][0]
    with torch.no_grad():
        s = [O.net_forward('itm', P, c['cfg'], inp, search=plan) for inp in (pos, negc, negi)]
        loss = float(O.itm_bce_loss(*s))
    for mode in CS.MODES:                          # the weight steps do not depend on the mode
        want = float(npz[mode + '|losses'][0])
        assert abs(loss - want) <= 2e-4 * abs(want), (mode, loss, want)      # (check_trajectory's bar for a loss)
    assert npz['full|losses'][1] == npz['two|losses'][1]
    for k in CS.weight_keys(plans):
        assert np.array_equal(npz['full|P:' + k], npz['two|P:' + k])
        assert np.abs(npz['full|P:' + k] - c['P'][k]).max() > 0
