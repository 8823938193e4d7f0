"""Factored ITM retrieval scoring: the evaluation of train_itm.py:437-546 (a [n_img, n_cap] score matrix, then i2t / t2i
R@1/5/10, medr, meanr) and the hard-negative mining of train_itm.py:299-363, without a full network forward per pair.

In the ITM Net_Full (full_itm.py) most of a pair forward does not depend on the pair:

* caption only -- embedding, LSTM, every encoder cell, attflat_x, and the key / value projections of every GuidedAtt in the
  decoder (K = V = the final encoder state);
* image only -- the image stem and every decoder node in front of the first operator that reads `pre`;
* pair -- the rest of the decoder and the head.

ItmScorer splits the network along these lines.  encode_captions() runs the caption side once per caption, with the K / V
projections of all guided operators as ONE product over their concatenated weights; encode_images() runs the image side once
per image; score_pairs() runs only the pair side: per-operator forwards for the non-guided nodes, and for each guided
operator Q projection -> indexed attention core (mmnas_mha_core_fwd_indexed: pair p reads caption cap_idx[p]'s cached
K / V) -> merge -> residual / LayerNorm; then attflat_y and the pair head kernel (mmnas_itm_pair_head).

Memory of a CaptionCache: per caption Sx * (2 * sum of the guided operators' inner sizes) floats of K / V -- at the train_itm
dimensions (50 tokens, 10 guided operators of 512) 50 * 10240 * 4 B = 2 MB -- plus the mask and attflat_x's output.  That is
why score_matrix() encodes the captions in chunks.  An ImageCache holds per image the decoder state after the image-only
prefix (Sy * HSIZE floats), the mask and the raw relation tensor.

Tie rule.  The reference ranks by numpy argsort, whose order among equal scores is unspecified, and the sigmoid scores of a
trained net do saturate to 1.0f.  Here a rank is the number of candidates with a STRICTLY greater score, and a top-k orders
equal scores by the lower candidate position.  The results are those of the reference whenever the relevant scores are
distinct; recall_at_k reports how many queries a tie touched.  NaN scores raise.

Batch invariance: captions and images are encoded, and pairs are scored, in batches of a fixed size (the last one padded
by repeating its last row), so an entry of the score matrix does not depend on how the work was chunked or sharded.

The search supernet (search_itm.py).  SupernetItmScorer scores an ITM Net_Search under the architecture that is installed when
a method is called -- the sampled one of the mining pass (search_itm.py:267-348, MixedOp.MODE None, between
unused_modules_off() and unused_modules_back()) or the chosen one of the evaluation (set_chosen_op_active()).  It is ItmScorer
with each MixedOp standing for its active candidate: the same planner, the same kernels on the pair side.  The architecture is
part of a cache: the scorer plans again when the installed indices changed, and refuses caches made under another architecture.
mine_hard_negatives() is one mining pass over a scorer's caches for either anchor side, gather_mined() the script's all_gather,
reordering and trim (search_itm.py:296-305).  The triplet steps of the search loop are harness.triplet_batch / BatchedTriplet.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import switches
from .model import modules as M
from .model import nets
from .model.mixed import MixedOp

__all__ = ['ItmScorer', 'SupernetItmScorer', 'CaptionCache', 'ImageCache', 'recall_at_k', 'rank_matrix', 'hard_negative_indices',
           'topk_positions', 'mine_hard_negatives', 'gather_mined', 'interleave_ranks']

# decoder operators that never read `pre` (the language state): they run on the image side before the first guided operator
# and per pair behind it
_PRE_FREE = (M.Identity, M.Zero, M.ReLU, M.LeakyReLU, M.GELU, M.GLU, M.SelfAtt, M.RelSelfAtt, M.FeedForward,
             M.FeedForward_deep, M.SepConv, M.StdConv)
MAX_KEYS = 64   # the indexed attention core is the <= 64-key forward


class CaptionCache:
    """Caption side of Net_Full for Nc captions.  x_mask [Nc,1,1,Sx] bool; mask8 [Nc,Sx] uint8 (the core's key mask);
    xflat [Nc, ATTFLAT_OUT] = attflat_x output; kv [Nc*Sx, ld]: the K / V of every guided operator, operator g's K in columns
    kv_cols[g][0] .. + di_g, its V in kv_cols[g][1] .. + di_g (kv is None when the decoder holds no guided operator).
    arch: the architecture the cache was computed under (SupernetItmScorer.arch); None for a fixed network's."""
    arch = None

    def __init__(self, x_mask, xflat, kv, kv_cols):
        self.x_mask, self.xflat, self.kv, self.kv_cols = x_mask, xflat, kv, kv_cols
        self.mask8 = ops._mask_u8(x_mask, x_mask.shape[0], x_mask.shape[-1])
        self.n, self.Sx = x_mask.shape[0], x_mask.shape[-1]

    def __len__(self):
        return self.n


class ImageCache:
    """Image side of Net_Full for Ni images: y_mask [Ni,1,1,Sy] bool, rel [Ni,Sy,Sy,4] the raw relation tensor, state
    [Ni,Sy,HSIZE] the decoder state after the image-only prefix nodes.  arch: as CaptionCache's."""
    arch = None

    def __init__(self, y_mask, rel, state):
        self.y_mask, self.rel, self.state = y_mask, rel, state
        self.n = state.shape[0]

    def __len__(self):
        return self.n

    def rows(self, start, end):
        out = ImageCache(self.y_mask[start:end], self.rel[start:end], self.state[start:end])
        out.arch = self.arch
        return out


def _pad_rows(t, n):
    """t with its first dimension padded to n by repeating its last row (fixed batch shapes: see the module docstring)."""
    k = t.shape[0]
    if k == n:
        return t
    return torch.cat((t, t[k - 1:k].expand((n - k,) + tuple(t.shape[1:]))), 0)


class ItmScorer:
    """Factored scoring of an ITM Net_Full (mmnas.model.full_itm.Net_Full / mmnas_amd.model.full_itm.Net_Full).

    The decoder genotype is planned at construction: `prefix_nodes` (image only: in front of the first operator that reads
    `pre`), `guided_ops` (GuidedAtt: K / V cached per caption) and `pair_nodes` (the non-guided nodes behind the first guided
    one), as (cell, node) positions.  Every decoder node must hold a single operator, and the only decoder operator that may
    read `pre` is GuidedAtt; anything else raises ValueError naming the cause.

    Every call runs the network in eval mode under torch.no_grad() (dropout off, as after net.eval()), restores each module's
    previous `training` flag and touches no .grad.  pair_batch: pairs per pair-side pass; encode_batch: captions / images per
    encoder pass."""

    def __init__(self, net, pair_batch=1024, encode_batch=256):
        if isinstance(net, torch.nn.parallel.DistributedDataParallel):
            net = net.module
        if getattr(net, 'SEARCH', False):
            raise ValueError('ItmScorer: a search supernet (Net_Search) is not supported -- its nodes are MixedOps over several '
                             'candidates; scoring the supernet (search_itm.py) is a separate feature')
        if not isinstance(net, nets.NetFullBase):
            raise ValueError('ItmScorer: needs an ITM Net_Full, got %s' % type(net).__name__)
        if net.TASK != 'itm':
            raise ValueError("ItmScorer: needs an ITM Net_Full, got a '%s' network (%s)" % (net.TASK, type(net).__name__))
        if int(pair_batch) < 1 or int(encode_batch) < 1:
            raise ValueError('ItmScorer: pair_batch and encode_batch must be positive')
        self.net = net
        self.pair_batch, self.encode_batch = int(pair_batch), int(encode_batch)
        self._plan()

    def _node_op(self, ci, ni, node):
        """The one operator decoder cell ci's node ni stands for."""
        if len(node) != 1:
            raise ValueError('%s: decoder cell %d node %d holds %d operators; the scorer needs single-operator '
                             'nodes' % (type(self).__name__, ci, ni, len(node)))
        return node[0]

    def _plan(self):
        """Split the decoder into prefix_nodes / guided_ops / pair_nodes (class docstring)."""
        name = type(self).__name__
        self.prefix_nodes, self.guided_ops, self.pair_nodes = [], [], []
        self._steps = []   # pair side in order: ('guided', op, g) / ('op', op)
        self._prefix = []
        seen_guided = False
        for ci, cell in enumerate(self.net.backnone.cells_dec):
            for ni, node in enumerate(cell.dag):
                op = self._node_op(ci, ni, node)
                if isinstance(op, M.UniimgAtt):
                    raise ValueError('%s: decoder cell %d node %d is UniimgAtt, whose keys and values are cat(x, pre) -- '
                                     'only GuidedAtt may read pre' % (name, ci, ni))
                if type(op) is M.GuidedAtt:
                    seen_guided = True
                    self._steps.append(('guided', op, len(self.guided_ops)))
                    self.guided_ops.append((ci, ni))
                elif isinstance(op, _PRE_FREE):
                    if seen_guided:
                        self._steps.append(('op', op, None))
                        self.pair_nodes.append((ci, ni))
                    else:
                        self._prefix.append(op)
                        self.prefix_nodes.append((ci, ni))
                else:
                    raise ValueError('%s: decoder cell %d node %d holds %s, which the scorer does not know to be '
                                     'independent of pre' % (name, ci, ni, type(op).__name__))

    # ---- mode handling ---------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _eval(self):
        flags = [(m, m.training) for m in self.net.modules()]
        self.net.eval()
        try:
            with torch.no_grad():
                yield
        finally:
            for m, t in flags:
                m.training = t

    def _device(self):
        return self.net.imgfeat_linear.weight.device

    # ---- caption side ------------------------------------------------------------------------------------------------------
    def _kv_weights(self):
        ws, cols, off = [], [], 0
        for kind, op, _ in self._steps:
            if kind != 'guided':
                continue
            mh = op.mhatt
            di = mh.linear_k.weight.shape[0]
            ws += [mh.linear_k.weight, mh.linear_v.weight]
            cols.append((off, off + di))
            off += 2 * di
        return (torch.cat(ws, 0) if ws else None), cols, off

    def encode_captions(self, cap_ix, rel_cap=None):
        """Caption side for cap_ix [Nc, Sx] token indices (rel_cap [Nc, Sx, Sx, 3] or None, as the network takes it)."""
        net = self.net
        Nc, Sx = cap_ix.shape
        if Sx > MAX_KEYS:
            raise ValueError('ItmScorer: captions of %d tokens; the indexed attention core serves at most %d keys' % (Sx, MAX_KEYS))
        with self._eval():
            W, cols, ld = self._kv_weights()
            bs = self.encode_batch
            kv = torch.empty(Nc * Sx, ld, dtype=torch.float32, device=cap_ix.device) if W is not None else None
            masks, flats = [], []
            for s in range(0, Nc, bs):
                n = min(bs, Nc - s)
                ix = _pad_rows(cap_ix[s:s + n], bs)
                rc = _pad_rows(rel_cap[s:s + n], bs) if rel_cap is not None else None
                x_mask, x, xflat = self._caption_batch(ix, rc)
                masks.append(x_mask[:n])
                flats.append(xflat[:n])
                if W is not None:   # the K / V projections of every guided operator: ONE product
                    kv[s * Sx:(s + n) * Sx] = ops.linear(x, W)[:n].reshape(n * Sx, ld)
            return CaptionCache(torch.cat(masks, 0), torch.cat(flats, 0).contiguous(), kv, cols)

    def _caption_batch(self, ques_ix, x_rel):
        """The language half of _Net.forward (nets.py): mask, embedding, LSTM, encoder cells, attflat_x."""
        net = self.net
        x_mask = nets.make_mask(ques_ix.unsqueeze(2))
        emb = ops.embedding(ques_ix, net.embedding)
        x = ops.lstm(emb, net.lstm) if (ops.lstm_enabled() and ops.lstm_supported(emb, net.lstm)) else net.lstm(emb)[0]
        if x_rel is not None and hasattr(net, 'linear_x_rel'):
            x_rel = (M.RelHandle(x_rel, net.linear_x_rel.weight, net.linear_x_rel.bias) if nets.LAZY_REL else
                     ops.linear(x_rel, net.linear_x_rel.weight, net.linear_x_rel.bias, relu=True))
        for cell in net.backnone.cells_enc:
            x = cell(s=x, s_mask=x_mask, rel_embed=x_rel)
        return x_mask, x, net.attflat_x(x, x_mask)

    # ---- image side ------------------------------------------------------------------------------------------------------
    def _rel_handle(self, raw):
        net = self.net
        if nets.LAZY_REL:
            return M.RelHandle(raw, net.linear_y_rel.weight, net.linear_y_rel.bias)
        return ops.linear(raw, net.linear_y_rel.weight, net.linear_y_rel.bias, relu=True)

    def encode_images(self, frcn_feat, bbox_feat, rel_img):
        """Image side for frcn_feat [Ni, Sy, F], bbox_feat [Ni, Sy, 5], rel_img [Ni, Sy, Sy, 4]."""
        net = self.net
        Ni = frcn_feat.shape[0]
        with self._eval():
            bs = self.encode_batch
            masks, states = [], []
            for s in range(0, Ni, bs):
                n = min(bs, Ni - s)
                f = _pad_rows(frcn_feat[s:s + n], bs)
                y_mask = nets.make_mask(f)
                if net._cfg.BBOX_FEATURE:
                    bb = ops.linear(_pad_rows(bbox_feat[s:s + n], bs), net.bboxfeat_linear.weight, net.bboxfeat_linear.bias)
                    f = torch.cat((f, bb), dim=-1)
                y = ops.linear(f, net.imgfeat_linear.weight, net.imgfeat_linear.bias)
                rel = self._rel_handle(_pad_rows(rel_img[s:s + n], bs).contiguous())
                for op in self._prefix:
                    y = op(y, None, y_mask, None, rel)
                masks.append(y_mask[:n])
                states.append(y[:n])
            return ImageCache(torch.cat(masks, 0), rel_img.contiguous(), torch.cat(states, 0).contiguous())

    # ---- pair side -------------------------------------------------------------------------------------------------------
    def _guided(self, op, g, y, cap, kv_idx):
        """GuidedAtt over the cached K / V: Q projection -> indexed core -> merge -> residual / LayerNorm (modules.py:301-325)."""
        mh = op.mhatt
        P, Sy, d = y.shape
        di, dh = mh.linear_q.weight.shape[0], mh.HBASE
        Q = ops.linear(y, mh.linear_q.weight)
        O = torch.empty_like(Q)
        lse = torch.empty(P, di // dh, Sy, 2, dtype=torch.float32, device=y.device)
        kc, vc = cap.kv_cols[g]
        desc = L.MhaDesc()
        desc.B, desc.H, desc.Sq, desc.Sk, desc.dh = P, di // dh, Sy, cap.Sx, dh
        desc.ldq = desc.ldo = di
        desc.ldk = desc.ldv = cap.kv.shape[1]
        base = cap.kv.data_ptr()
        desc.Q, desc.K, desc.V, desc.mask = L.fptr(Q), base + 4 * kc, base + 4 * vc, L.ptr(cap.mask8)
        desc.O, desc.lse = L.fptr(O), L.fptr(lse)
        L.check(L.lib().mmnas_mha_core_fwd_indexed(C.byref(desc), L.ptr(kv_idx), L.stream()))
        z = torch.empty_like(y)
        Wm = ops._f32c(mh.linear_merge.weight)
        ops.gemm(L.GEMM_NT, [dict(M=P * Sy, A=[O], B=[Wm], C=z, residual=(y if op.residual else None))],
                 d, di, di, di, d, ldres=d)
        return ops.layer_norm(z, op.ln.a_2, op.ln.b_2, op.ln.eps) if op.norm else z

    def _pair_batch(self, images, captions, ii, ci, n, logits, out=None, rows=None, cols=None):
        """Score n pairs (ii, ci padded to pair_batch).  Returns [n] (scores or logits) or writes into out[rows, cols]."""
        net = self.net
        y = images.state.index_select(0, ii)
        y_mask = images.y_mask.index_select(0, ii)
        rel = self._rel_handle(images.rel.index_select(0, ii))
        kv_idx = ci.to(torch.int32).contiguous()
        for kind, op, g in self._steps:
            if kind == 'guided':
                y = self._guided(op, g, y, captions, kv_idx)
            else:
                y = op(y, None, y_mask, None, rel)
        yflat = net.attflat_y(y, y_mask).contiguous()
        Wp, bp = ops._f32c(net.proj.weight), ops._f32c(net.proj.bias)
        a, b = ops._f32c(net.proj_norm.a_2), ops._f32c(net.proj_norm.b_2)
        D = yflat.shape[1]
        lib = L.lib()
        if out is not None:
            L.check(lib.mmnas_itm_pair_head(L.fptr(captions.xflat), L.ptr(kv_idx), L.fptr(yflat), L.fptr(a), L.fptr(b), L.fptr(Wp),
                                            L.fptr(bp), None, L.fptr(out), L.ptr(rows), L.ptr(cols), out.stride(0), n, D,
                                            net.proj_norm.eps, L.stream()))
            return None
        res = torch.empty(n, dtype=torch.float32, device=y.device)
        L.check(lib.mmnas_itm_pair_head(L.fptr(captions.xflat), L.ptr(kv_idx), L.fptr(yflat), L.fptr(a), L.fptr(b), L.fptr(Wp),
                                        L.fptr(bp), L.fptr(res) if logits else None, None if logits else L.fptr(res), None, None,
                                        0, n, D, net.proj_norm.eps, L.stream()))
        return res

    def _check(self, images, captions, img_idx, cap_idx):
        if not isinstance(images, ImageCache) or not isinstance(captions, CaptionCache):
            raise TypeError('ItmScorer: score_pairs takes the ImageCache / CaptionCache of encode_images / encode_captions')
        if img_idx.shape != cap_idx.shape or img_idx.dim() != 1:
            raise ValueError('ItmScorer: img_idx and cap_idx must be 1-D of the same length')
        for idx, n, what in ((img_idx, images.n, 'img_idx'), (cap_idx, captions.n, 'cap_idx')):
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
                raise IndexError('ItmScorer: %s outside 0..%d' % (what, n - 1))

    def score_pairs(self, images, captions, img_idx, cap_idx, logits=False):
        """[P] scores (sigmoid; logits=True: the logits before it) of the pairs (img_idx[p], cap_idx[p]) -- arbitrary index
        vectors, repeats and any order allowed.  Equals net((frcn[img_idx], bbox[img_idx], rel_img[img_idx], cap_ix[cap_idx],
        rel_cap[cap_idx])) in eval mode."""
        dev = self._device()
        img_idx = torch.as_tensor(img_idx, device=dev).long().reshape(-1)
        cap_idx = torch.as_tensor(cap_idx, device=dev).long().reshape(-1)
        self._check(images, captions, img_idx, cap_idx)
        P, bs = img_idx.numel(), self.pair_batch
        outs = []
        with self._eval():
            for s in range(0, P, bs):
                n = min(bs, P - s)
                outs.append(self._pair_batch(images, captions, _pad_rows(img_idx[s:s + n], bs), _pad_rows(cap_idx[s:s + n], bs),
                                             n, logits))
        return torch.cat(outs) if outs else torch.empty(0, dtype=torch.float32, device=dev)

    def score_matrix(self, images, captions, rows=None, caption_chunk=1000, out=None):
        """The [Ni, Nc] score matrix of train_itm.py:463-491: images = (frcn_feat, bbox_feat, rel_img) or an ImageCache,
        captions = (cap_ix, rel_cap) or a CaptionCache (raw captions are encoded caption_chunk at a time).
        rows = (start, end): only those image rows are filled (train_itm.py:471-473's per-rank split; the caller all-reduces);
        the other rows are zero in a fresh matrix and left untouched in `out`."""
        dev = self._device()
        Ni = images.n if isinstance(images, ImageCache) else images[0].shape[0]
        Nc = captions.n if isinstance(captions, CaptionCache) else captions[0].shape[0]
        r0, r1 = (0, Ni) if rows is None else (int(rows[0]), int(rows[1]))
        if not 0 <= r0 <= r1 <= Ni:
            raise ValueError('ItmScorer: rows %r outside 0..%d' % (rows, Ni))
        if out is None:
            out = torch.zeros(Ni, Nc, dtype=torch.float32, device=dev)
        elif tuple(out.shape) != (Ni, Nc) or out.dtype != torch.float32 or out.stride(1) != 1:
            raise ValueError('ItmScorer: out must be a float32 [%d, %d] matrix with unit column stride' % (Ni, Nc))
        if r0 == r1 or Nc == 0:
            return out
        img = images.rows(r0, r1) if isinstance(images, ImageCache) else self.encode_images(*(t[r0:r1] for t in images))
        nr, bs = r1 - r0, self.pair_batch
        chunk = Nc if isinstance(captions, CaptionCache) else max(1, int(caption_chunk))
        with self._eval():
            for c0 in range(0, Nc, chunk):
                c1 = min(Nc, c0 + chunk)
                cap = captions if isinstance(captions, CaptionCache) else self.encode_captions(
                    captions[0][c0:c1], captions[1][c0:c1] if captions[1] is not None else None)
                nc = c1 - c0
                ii = torch.arange(nr, device=dev).repeat_interleave(nc)
                ci = torch.arange(nc, device=dev).repeat(nr)
                if cap is captions:
                    ci = ci + c0
                row = (ii + r0).to(torch.int32)
                col = (torch.arange(c0, c1, device=dev, dtype=torch.int32)).repeat(nr)
                for s in range(0, nr * nc, bs):
                    n = min(bs, nr * nc - s)
                    self._pair_batch(img, cap, _pad_rows(ii[s:s + n], bs), _pad_rows(ci[s:s + n], bs), n, False, out=out,
                                     rows=row[s:s + n].contiguous(), cols=col[s:s + n].contiguous())
        return out


def _whole_tile_products():
    """mmnas_gemm on whole output tiles only (its scheduling row MMNAS_GEMM_SK at 0) while the block runs, the previous setting
    afterwards.  The automatic schedule cuts the K sum of a product with few output tiles and a long K into runs (stream-K): the
    same rows then get other bits at M = 36 than at M = 9216 (measured: 1.9e-6 on values of 4 at K = 512).  Whole tiles sum K in
    one order whatever M and whichever tile shape (measured bit-equal from M = 36 to M = 147456, 64^2 and 128^2 tiles), which
    is what makes a score independent of pair_batch and encode_batch."""
    return switches.gemm_schedule({'MMNAS_GEMM_SK': 0})


class SupernetItmScorer(ItmScorer):
    """ItmScorer for the ITM search supernet (mmnas.model.hygr_itm.Net_Search, or DistributedDataParallel of one): factored
    scoring of the architecture that is INSTALLED when a method is called -- every node's active_index[0], as
    reset_binary_gates() / set_sampled(plan) / set_chosen_op_active() left it.  The planner is ItmScorer's, each MixedOp standing
    for its active candidate; the same rules hold (only GuidedAtt may read pre, UniimgAtt raises; `none` is an ordinary pre-free
    operator).  With no guided operator active the whole decoder is image-only: the caption cache has no K / V block and the pair
    side is attflat_y plus the pair head.

    `arch` is the tuple of the active indices of all encoder and decoder nodes the current plan was made for.  Every public
    call compares it with the net's installed indices (a tuple comparison, no device work) and plans again when they differ;
    the caches carry the `arch` they were computed under, and scoring with caches of another architecture raises ValueError.
    A node without active_index (nothing sampled yet) raises ValueError.

    Calls run in eval mode under no_grad with MixedOp.MODE = None and restore the training flags and MODE afterwards; indices,
    gates, alphas and .grad are not written.  Only active candidates are read, so the scorer works between
    unused_modules_off() and unused_modules_back() (search_itm.py:271-348 mines in that state).

    While a call runs the products are scheduled on whole output tiles (_whole_tile_products), so a score has the same bits
    whatever pair_batch and encode_batch are -- not only however the work was chunked at one batch size."""

    def __init__(self, net, pair_batch=1024, encode_batch=256):
        if isinstance(net, torch.nn.parallel.DistributedDataParallel):
            net = net.module
        if not isinstance(net, nets.NetSearchBase) or net.TASK != 'itm':
            raise ValueError('SupernetItmScorer: needs an ITM Net_Search, got %s%s' % (
                type(net).__name__, " for task '%s'" % net.TASK if isinstance(net, nets.NetSearchBase) else ''))
        if int(pair_batch) < 1 or int(encode_batch) < 1:
            raise ValueError('SupernetItmScorer: pair_batch and encode_batch must be positive')
        self.net = net
        self.pair_batch, self.encode_batch = int(pair_batch), int(encode_batch)
        self.arch = None
        self._sync()

    def _installed(self):
        arch = []
        for i, m in enumerate(self.net.redundant_modules):
            if not m.active_index:
                raise ValueError('SupernetItmScorer: node %d has no active_index -- no architecture was sampled '
                                 '(reset_binary_gates / set_sampled / set_chosen_op_active)' % i)
            arch.append(int(m.active_index[0]))
        return tuple(arch)

    def _sync(self):
        arch = self._installed()
        if arch != self.arch:
            self.arch = None      # (a plan that raises leaves no stale plan behind)
            self._plan()
            self.arch = arch

    def _node_op(self, ci, ni, node):
        mop = super()._node_op(ci, ni, node)
        op = mop.candidate_ops[mop.active_index[0]]
        if op is None:
            raise ValueError('SupernetItmScorer: decoder cell %d node %d: the active candidate %d was taken out by '
                             'unused_modules_off() under another architecture' % (ci, ni, mop.active_index[0]))
        return op

    @contextlib.contextmanager
    def _eval(self):
        mode = MixedOp.MODE
        MixedOp.MODE = None
        try:
            with _whole_tile_products(), super()._eval():
                yield
        finally:
            MixedOp.MODE = mode

    def _same_arch(self, *caches):
        for c in caches:
            if isinstance(c, (ImageCache, CaptionCache)) and c.arch != self.arch:
                raise ValueError('SupernetItmScorer: the %s was computed under architecture %r, the net now holds %r -- encode '
                                 'again after a re-sample' % (type(c).__name__, c.arch, self.arch))

    def encode_captions(self, cap_ix, rel_cap=None):
        self._sync()
        out = super().encode_captions(cap_ix, rel_cap)
        out.arch = self.arch
        return out

    def encode_images(self, frcn_feat, bbox_feat, rel_img):
        self._sync()
        out = super().encode_images(frcn_feat, bbox_feat, rel_img)
        out.arch = self.arch
        return out

    def score_pairs(self, images, captions, img_idx, cap_idx, logits=False):
        self._sync()
        self._same_arch(images, captions)
        return super().score_pairs(images, captions, img_idx, cap_idx, logits)

    def score_matrix(self, images, captions, rows=None, caption_chunk=1000, out=None):
        self._sync()
        self._same_arch(images, captions)
        return super().score_matrix(images, captions, rows, caption_chunk, out)


# ---- ranks, recall, mining -------------------------------------------------------------------------------------------------
def _rank_numpy(S, G):
    Ni, Nc = S.shape
    gt = np.zeros((Ni, Nc), bool)
    for g in range(G):
        gt[np.arange(Ni), G * np.arange(Ni) + g] = True
    t = S[gt].reshape(Ni, G).max(1)
    i2t_rank = (S > t[:, None]).sum(1)
    i2t_tie = ((S == t[:, None]) & ~gt).sum(1)
    own = np.arange(Nc) // G
    tc = S[own, np.arange(Nc)]
    t2i_rank = (S > tc[None, :]).sum(0)
    t2i_tie = ((S == tc[None, :]) & (np.arange(Ni)[:, None] != own[None, :])).sum(0)
    return i2t_rank, i2t_tie, t2i_rank, t2i_tie


def rank_matrix(scores, caps_per_image=5):
    """(i2t_rank [Ni], i2t_tie [Ni], t2i_rank [Nc], t2i_tie [Nc]) as int64 numpy arrays for a score matrix [Ni, Nc] with
    Nc = caps_per_image * Ni (caption j belongs to image j // caps_per_image).  i2t_rank[i] = the number of captions scoring
    strictly above image i's best own caption; t2i_rank[j] = the number of images scoring strictly above caption j's own image;
    *_tie = the number of other candidates scoring exactly the same as that threshold.  The rank is the reference's argsort
    position (train_itm.py:505-546) whenever the tie count is 0.  CUDA tensors: mmnas_rank_matrix; otherwise numpy.
    Raises ValueError on NaN."""
    G = int(caps_per_image)
    Ni, Nc = scores.shape
    if Ni == 0 or Nc != G * Ni:
        raise ValueError('rank_matrix: %d captions for %d images is not %d per image' % (Nc, Ni, G))
    if isinstance(scores, torch.Tensor) and scores.is_cuda:
        S = ops._f32c(scores)
        dev = S.device
        i2t = torch.empty(2, Ni, dtype=torch.int32, device=dev)
        t2i = torch.empty(2, Nc, dtype=torch.int32, device=dev)
        nan = torch.empty(1, dtype=torch.int32, device=dev)
        L.check(L.lib().mmnas_rank_matrix(L.fptr(S), Ni, Nc, S.stride(0), L.ptr(i2t[0]), L.ptr(i2t[1]), L.ptr(t2i[0]),
                                          L.ptr(t2i[1]), L.ptr(nan), L.stream()))
        if int(nan.item()):
            raise ValueError('rank_matrix: the score matrix holds NaN')
        i2t, t2i = i2t.cpu().numpy().astype(np.int64), t2i.cpu().numpy().astype(np.int64)
        return i2t[0], i2t[1], t2i[0], t2i[1]
    S = scores.detach().cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
    if np.isnan(S).any():
        raise ValueError('rank_matrix: the score matrix holds NaN')
    return _rank_numpy(S, G)


def recall_at_k(scores, caps_per_image=5):
    """i2t / t2i R@1, R@5, R@10, medr and meanr of a score matrix [Ni, Nc] with the formulas of train_itm.py:505-546,
    plus i2t_ties / t2i_ties: the number of queries whose rank a tie touched (see rank_matrix for the tie rule; with distinct
    scores the numbers are the reference's).  Raises ValueError on NaN."""
    i2t, i2t_tie, t2i, t2i_tie = rank_matrix(scores, caps_per_image)
    res = {}
    for name, r, tie in (('i2t', i2t, i2t_tie), ('t2i', t2i, t2i_tie)):
        r = r.astype(np.float64)
        res[name + '_r1'] = 100.0 * len(np.where(r < 1)[0]) / len(r)
        res[name + '_r5'] = 100.0 * len(np.where(r < 5)[0]) / len(r)
        res[name + '_r10'] = 100.0 * len(np.where(r < 10)[0]) / len(r)
        res[name + '_medr'] = float(np.floor(np.median(r)) + 1)
        res[name + '_meanr'] = float(r.mean() + 1)
        res[name + '_ties'] = int((tie > 0).sum())
    return res


def topk_positions(scores, k):
    """[N, k] int64 positions of each row's k largest scores, descending, equal scores by the lower position.
    CUDA tensors: mmnas_row_topk (C <= 1024 columns); otherwise torch.sort(stable=True).  Raises ValueError on NaN."""
    if scores.dim() != 2 or not 1 <= k <= scores.shape[1]:
        raise ValueError('topk_positions: scores [N, C] with 1 <= k <= C; got %s, k=%d' % (tuple(scores.shape), k))
    if scores.is_cuda:
        S = ops._f32c(scores)
        N, Cn = S.shape
        out = torch.empty(N, k, dtype=torch.int32, device=S.device)
        nan = torch.empty(1, dtype=torch.int32, device=S.device)
        L.check(L.lib().mmnas_row_topk(L.fptr(S), N, Cn, S.stride(0), int(k), L.ptr(out), L.ptr(nan), L.stream()))
        if int(nan.item()):
            raise ValueError('topk_positions: the scores hold NaN')
        return out.long()
    if torch.isnan(scores).any():
        raise ValueError('topk_positions: the scores hold NaN')
    return torch.sort(scores, dim=-1, descending=True, stable=True)[1][:, :k]


def hard_negative_indices(scores, neg_idx, hard_size):
    """The selection step of the ITM hard-negative mining pass (train_itm.py:315-320), with the contract of
    harness.hard_negative_indices: `scores` are the matching scores of every anchor against its NEG_RANDSIZE candidates
    (flattened), `neg_idx` [N, NEG_RANDSIZE] the candidates' dataset indices; returns [N, hard_size], per anchor the indices
    of its highest-scoring candidates.  Equal scores go by the lower candidate position (the reference's torch.argsort leaves
    their order unspecified: identical results whenever the scores are distinct).  Raises ValueError on NaN."""
    scores = scores.reshape(-1, neg_idx.shape[1])
    top = topk_positions(scores, int(hard_size))
    rows = torch.arange(top.size(0), device=top.device).unsqueeze(1).expand_as(top)
    return neg_idx.to(scores.device)[rows, top]


def mine_hard_negatives(scorer, images, captions, anchor_idx, cand_idx, hard_size, anchor='image'):
    """One hard-negative mining pass as search_itm.py / train_itm.py run it: [N, hard_size] int64 dataset indices, row n the
    `hard_size` highest-scoring candidates among cand_idx[n, :] for anchor anchor_idx[n].  anchor='image': the anchors are
    images and the candidates captions (search_itm.py:278-294); anchor='caption': the anchors are captions and the candidates
    images (search_itm.py:313-333).  `images` / `captions` are the scorer's caches over the whole dataset (an ItmScorer or a
    SupernetItmScorer); anchor_idx [N] and cand_idx [N, NEG_RANDSIZE] index into them.  Scores come from score_pairs, the
    selection from hard_negative_indices (equal scores by the lower candidate position)."""
    if anchor not in ('image', 'caption'):
        raise ValueError("mine_hard_negatives: anchor is 'image' or 'caption', got %r" % (anchor,))
    cand_idx = torch.as_tensor(cand_idx).long()
    anchor_idx = torch.as_tensor(anchor_idx).long().reshape(-1)
    if cand_idx.dim() != 2 or cand_idx.shape[0] != anchor_idx.numel():
        raise ValueError('mine_hard_negatives: cand_idx must be [N, NEG_RANDSIZE] for anchor_idx [N]; got %s and %s'
                         % (tuple(cand_idx.shape), tuple(anchor_idx.shape)))
    own = anchor_idx.to(cand_idx.device).repeat_interleave(cand_idx.shape[1])
    other = cand_idx.reshape(-1)
    if anchor == 'image':
        scores = scorer.score_pairs(images, captions, own, other)
    else:
        scores = scorer.score_pairs(images, captions, other, own)
    return hard_negative_indices(scores, cand_idx, hard_size)


def interleave_ranks(parts):
    """The per-rank mining results [n, hard_size] of a SubsetDistributedSampler's shards in dataset order: rank r's i-th row
    lands at r + world * i (search_itm.py:300: cat(dim=1) of the unsqueezed results, viewed as [-1, hard_size])."""
    hard = parts[0].shape[-1]
    return torch.cat([p.unsqueeze(1) for p in parts], dim=1).view(-1, hard)


def gather_mined(local, world, rest, group=None):
    """search_itm.py:296-305: all_gather the ranks' mining results `local` [n, hard_size], put them in the sampler's order
    (interleave_ranks) and drop the last `rest` rows (the sampler's padding, `sampler.rest_data_num`).  Returns a CPU tensor,
    as the script hands it to the datasets.  world == 1, or no initialised process group: only the trim."""
    import torch.distributed as dist
    if int(world) > 1 and dist.is_available() and dist.is_initialized():
        parts = [torch.zeros_like(local) for _ in range(int(world))]
        dist.all_gather(parts, local.contiguous(), group=group)
        local = interleave_ranks(parts)
    local = local.cpu()
    return local[:-int(rest)] if rest else local
