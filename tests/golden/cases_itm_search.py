"""The case of the ITM search trajectory (tests/golden/itm_search_traj.npz): shared by the generator
(make_golden_itm_search.py, which needs the reference tree) and by the replays (tests/test_itm_search_gpu.py,
tests/test_oracle_golden_itm_search.py), which do not.  No reference import here.

Dimensions: HSIZE 128 (two heads of 64), B = 3 triplets, 7 tokens with captions of 7, 4 and 1 live tokens, 9 regions with 9, 5
and 1 live regions -- the smallest at which head indexing, padded tails, a one-key row and every operator class of the ITM
search space occur.  Dropout 0.  The optimizer settings are the script's own (search_itm.py:141-166: NET_LR_BASE 1e-4 under
warm-up, betas (0.9, 0.98), eps 1e-9, clip 1.0; alphas: lr 0.1, betas (0, 0.999)) with epoch_steps = 1, so that the four
weight steps run at the four warm-up rates 1/4, 2/4, 3/4 and 1.  (At the 20x rate of cases.TRAJ_HYPER the reference's own
float32 and float64 runs of this case part by 6e-4 in the loss and 3e-2 in an alpha within the two rounds: Adam turns the
round-off of gradients that are zero up to round-off into full steps.  At the script's rate they agree to 3e-7 and 2e-5.)"""
import numpy as np

from tests.golden import cases

SEED = 9400
B, SX, SY = 3, 7, 9
LIVE_TOKENS = (7, 4, 1)
LIVE_REGIONS = (9, 5, 1)
MODES = ('full', 'two')
ROUNDS = 2
ALPHA_EVERY = 2          # one bilevel round: 2 weight steps + 1 arch step (search_itm.py:381-447 with ALPHA_EVERY = 2)
HYPER = dict(net_lr=1e-4, net_betas=(0.9, 0.98), net_eps=1e-9, clip=1.0, epoch_steps=1,
             alpha_lr=0.1, alpha_betas=(0.0, 0.999))


def batch(rs, cfg, token_size, shift=0):
    """One 5-tuple (frcn, bbox, rel_img, cap_ix, rel_cap) of B samples with the live lengths above, rotated by `shift`
    samples (so that the one-token caption meets every image length across the batches)."""
    frcn = np.maximum(rs.standard_normal((B, SY, cfg.FRCNFEAT_SIZE)), 0).astype(np.float32) + 0.01
    y_rel = rs.standard_normal((B, SY, SY, 4)).astype(np.float32)
    ques = rs.randint(1, token_size, size=(B, SX)).astype(np.int64)
    x_rel = rs.standard_normal((B, SX, SX, 3)).astype(np.float32)
    for b in range(B):
        ny = LIVE_REGIONS[b]
        nx = LIVE_TOKENS[(b + shift) % B]
        frcn[b, ny:] = 0
        y_rel[b, ny:] = 0
        y_rel[b, :, ny:] = 0
        ques[b, nx:] = 0
        x_rel[b, nx:] = 0
        x_rel[b, :, nx:] = 0
    return frcn, np.zeros((B, SY, 5), np.float32), y_rel, ques, x_rel


def setup(seed=SEED):
    """(case, batches, plans): case = cases.net_case of the ITM supernet (its P and cfg; its own inputs are not used);
    batches = {'train': [(pos, neg), (pos, neg)], 'eval': (pos, neg)} -- the weight steps of a round take train[0] and
    train[1], the arch step takes eval; plans[mode] = one list per round of three injected samples (weight, weight, arch), the
    weight samples (MODE None) shared by the two modes."""
    c = cases.net_case('itm', None, seed, search=True, HSIZE=128, B=B, Sx=SX, Sy=SY)
    rs = np.random.RandomState(seed + 1)
    mk = lambda shift: (batch(rs, c['cfg'], c['token_size'], 0), batch(rs, c['cfg'], c['token_size'], shift))
    batches = {'train': [mk(1), mk(2)], 'eval': mk(1)}
    prs = np.random.RandomState(seed + 50000)
    weight = [[cases.search_plan(prs, None), cases.search_plan(prs, None)] for _ in range(ROUNDS)]
    plans = {}
    for mode in MODES:
        plans[mode] = [weight[r] + [cases.search_plan(prs, mode)] for r in range(ROUNDS)]
    return c, batches, plans


def flat(plan):
    return plan['enc'] + plan['dec']


def weight_keys(plans):
    """The three recorded weight tensors: the image stem, the merge projection of the first encoder node whose self-attention
    candidate the first weight step samples, and of the first decoder node whose guided-attention candidate it samples."""
    p0 = plans[MODES[0]][0][0]
    enc = next(i for i, (a, _) in enumerate(p0['enc']) if a[0] == 0)
    dec = next(i for i, (a, _) in enumerate(p0['dec']) if a[0] == 2)
    return ('imgfeat_linear.weight',
            'backnone.cells_enc.0.dag.%d.0.candidate_ops.0.mhatt.linear_merge.weight' % enc,
            'backnone.cells_dec.0.dag.%d.0.candidate_ops.2.mhatt.linear_merge.weight' % dec)
