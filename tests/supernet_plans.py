"""Injected architectures for the SupernetItmScorer tests (host and GPU): three plans over the ITM supernet, each as operator
names per node, the (active, inactive) lists Net_Search.set_sampled takes, and the decoder split those names imply.

The ITM supernet's own candidate lists (`enc_safe` / `dec_safe`) hold neither `none` nor a `uniimg_att`; a plan that names one
swaps the registry operator into the candidate slot it is given (`swaps`: (decoder node, candidate index, name)) -- a MixedOp
scores whatever candidate is active."""
import numpy as np
import torch

from tests.golden import cases

ENC = ['self_att_64', 'feed_forward']
DEC = ['self_att_64', 'rel_self_att_64', 'guided_att_64', 'feed_forward']

PRIOR = dict(enc=['self_att_64', 'feed_forward'] * 6, dec=['rel_self_att_64', 'guided_att_64', 'feed_forward'] * 6, swaps=())
# a guided operator as the first decoder node (empty prefix) and `none` in the guided slot of node 4
GUIDED_FIRST = dict(enc=['feed_forward', 'self_att_64', 'self_att_64', 'feed_forward'] * 3,
                    dec=['guided_att_64', 'feed_forward', 'rel_self_att_64', 'guided_att_64', 'none', 'self_att_64',
                         'guided_att_64', 'feed_forward', 'feed_forward', 'rel_self_att_64', 'guided_att_64', 'self_att_64',
                         'feed_forward', 'guided_att_64', 'rel_self_att_64', 'feed_forward', 'self_att_64', 'guided_att_64'],
                    swaps=((4, 2, 'none'),))
# no guided operator at all: the whole decoder is image-only
NO_GUIDED = dict(enc=['self_att_64'] * 4 + ['feed_forward'] * 8,
                 dec=['self_att_64', 'feed_forward', 'rel_self_att_64'] * 6, swaps=())
PLANS = {'prior': PRIOR, 'guided_first_none': GUIDED_FIRST, 'no_guided': NO_GUIDED}


def sampled(plan):
    """The (active, inactive) list of set_sampled: encoder nodes, then decoder nodes."""
    swapped = {node: (idx, name) for node, idx, name in plan['swaps']}
    out = []
    for name in plan['enc']:
        a = ENC.index(name)
        out.append(([a], [i for i in range(len(ENC)) if i != a]))
    for node, name in enumerate(plan['dec']):
        a = swapped[node][0] if node in swapped and swapped[node][1] == name else DEC.index(name)
        out.append(([a], [i for i in range(len(DEC)) if i != a]))
    return out


def install(net, plan):
    """Swap the plan's registry operators into their candidate slots and install the plan."""
    from mmnas.utils.ops_adapter import OpsAdapter
    cfg = net._cfg
    dev = net.imgfeat_linear.weight.device
    for node, idx, name in plan['swaps']:
        mop = net.backnone.cells_dec[0].dag[node][0]
        mop.candidate_ops[idx] = OpsAdapter().OPS[name](cfg, norm=cfg.OPS_NORM, residual=cfg.OPS_RESIDUAL).to(dev)
    net.set_sampled(sampled(plan))


def implied_split(plan):
    """(prefix_nodes, guided_ops, pair_nodes) as (cell, node) positions, from the decoder's operator names alone."""
    names = plan['dec']
    guided = [i for i, n in enumerate(names) if n.startswith('guided_att')]
    first = guided[0] if guided else len(names)
    return ([(0, i) for i in range(first)], [(0, i) for i in guided],
            [(0, i) for i in range(first, len(names)) if i not in guided])


def full_genotype_and_params(plan, P):
    """The fixed network the plan stands for: (genotype, state_dict) -- every node's active candidate under the key Net_Full
    gives it (`...dag.N.0.<param>` for `...dag.N.0.candidate_ops.K.<param>`), everything outside the cells as it is."""
    act = sampled(plan)
    chosen = {}
    for i, (a, _) in enumerate(act):
        kind, node = ('enc', i) if i < len(plan['enc']) else ('dec', i - len(plan['enc']))
        chosen['backnone.cells_%s.0.dag.%d.0.' % (kind, node)] = 'candidate_ops.%d.' % a[0]
    swapped = {'backnone.cells_dec.0.dag.%d.0.candidate_ops.%d.' % (node, idx) for node, idx, _ in plan['swaps']}
    out = {}
    for k, v in P.items():
        if 'alpha_' in k:
            continue
        if '.candidate_ops.' not in k:
            out[k] = v
            continue
        base = k[:k.index('candidate_ops.')]
        pick = chosen[base]
        if k.startswith(base + pick) and (base + pick) not in swapped:
            out[base + k[len(base + pick):]] = v
    return {'enc': [[n] for n in plan['enc']], 'dec': [[n] for n in plan['dec']]}, out


N_IMG, N_CAP = 5, 7        # the scoring tests' images and captions; the mining test draws six distinct candidates of SEVEN images
ONE_REGION_IMAGE, ONE_TOKEN_CAPTION = 4, 6
# The mining test's precondition -- on the float64 oracle's scores every anchor's four best candidates lie at least 1e-2 apart,
# on both anchor sides -- picked on the CPU over case seeds 9950.. and draw seeds 0..299: with random weights the image side moves
# a score far less than the caption side (under the prior genotype the seven images of one caption span 1e-2 in all), the
# image-only plan spreads them most; case 9956 with draw 146 has a smallest gap of 1.6e-2
MINING_CASE_SEED, MINING_SEED, MINING_PLAN = 9956, 146, 'no_guided'


def retrieval_case(seed=9950, Sx=7, Sy=9):
    """The supernet case of the GPU tests: weights of cases.net_case, 7 images and 7 captions with ragged live lengths, image
    ONE_REGION_IMAGE with one live region and caption ONE_TOKEN_CAPTION with one live token.  Returns (case, images, captions)
    as numpy tuples (frcn, bbox, rel_img) / (cap_ix, rel_cap)."""
    c = cases.net_case('itm', None, seed, search=True, HSIZE=128, B=7, Sx=Sx, Sy=Sy)
    frcn, bbox, rel_img, cap_ix, rel_cap = (np.array(a) for a in c['inputs'])
    i, j = ONE_REGION_IMAGE, ONE_TOKEN_CAPTION
    frcn[i, 1:] = 0
    rel_img[i, 1:] = 0
    rel_img[i, :, 1:] = 0
    cap_ix[j, 1:] = 0
    rel_cap[j, 1:] = 0
    rel_cap[j, :, 1:] = 0
    assert (np.abs(frcn[i]).sum(-1) > 0).sum() == 1 and (cap_ix[j] != 0).sum() == 1
    return c, (frcn, bbox, rel_img), (cap_ix, rel_cap)


def mining_draw(anchor, seed=MINING_SEED, n_anchor=5, n_cand=6):
    """(anchor_idx [5], cand_idx [5, 6]) of the mining test: distinct anchors, per anchor six distinct candidates of the other
    side's seven items."""
    rs = np.random.RandomState(1000 * seed + (0 if anchor == 'image' else 1))
    anchors = rs.permutation(7)[:n_anchor]
    cand = np.stack([rs.permutation(7)[:n_cand] for _ in range(n_anchor)])
    return torch.from_numpy(anchors).long(), torch.from_numpy(cand).long()


def oracle_scores(c, plan, images, captions, img_idx, cap_idx):
    """Float64 oracle scores of the pairs (img_idx[p], cap_idx[p]) under the plan."""
    from oracle import mmnas_oracle as O
    ii, ci = np.asarray(img_idx), np.asarray(cap_idx)
    ins = [torch.from_numpy(a[ii]) for a in images] + [torch.from_numpy(a[ci]) for a in captions]
    ins = tuple(t.double() if t.dtype == torch.float32 else t for t in ins)
    if plan['swaps']:        # the oracle's supernet knows the search space's own candidates only: the fixed network the plan stands for
        genotype, P = full_genotype_and_params(plan, c['P'])
        P64 = {k: torch.from_numpy(v).double() for k, v in P.items()}
        with torch.no_grad():
            return O.net_forward('itm', P64, c['cfg'], ins, genotype=genotype).numpy()
    P64 = {k: torch.from_numpy(v).double() for k, v in c['P'].items()}
    act = sampled(plan)
    search = {'mode': None, 'enc': act[:len(plan['enc'])], 'dec': act[len(plan['enc']):]}
    with torch.no_grad():
        return O.net_forward('itm', P64, c['cfg'], ins, search=search).numpy()


def build_supernet(c, device='cpu'):
    from mmnas.model.hygr_itm import Net_Search
    init = {'token_size': c['token_size'], 'ans_size': c['ans_size'],
            'pretrained_emb': np.zeros((c['token_size'], c['cfg'].WORD_EMBED_SIZE), np.float32)}
    net = Net_Search(c['cfg'], init)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in c['P'].items()}, strict=True)
    return net.to(device)
