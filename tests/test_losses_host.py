"""mmnas_amd.losses without a GPU: the module imports, CPU tensors take the torch composition itself (bit-equal to
harness.vgd_loss / BCE_Loss / Margin_Loss), fused() maps the two ITM loss classes, the cfg fields are read, wrong shapes raise,
and the new C entries are declared in the header and bound in _lib.SYMBOLS."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.util import REPO

T = torch.from_numpy

NEW_SYMBOLS = ('mmnas_vgd_loss_fwd', 'mmnas_itm_triplet_loss_fwd', 'mmnas_loss_grad_scale')


def _vgd_inputs(B=5, S=7, smask='full', bmask='full', seed=3):
    rs = np.random.RandomState(seed)
    ps = T(np.log(rs.dirichlet(np.ones(S), B)).astype(np.float32)).requires_grad_()
    pr = T(rs.standard_normal((B, S, 4)).astype(np.float32) * 1.5).requires_grad_()
    sc = rs.dirichlet(np.ones(S), B).astype(np.float32)
    sc[:, 1] = 0
    bb = rs.standard_normal((B, S, 4)).astype(np.float32)
    sm = (rs.uniform(size=(B, S) if smask == 'full' else (B, 1)) < 0.7).astype(np.float32)
    sm[0] = 1
    bm = (rs.uniform(size=(B, S, 1)) < 0.4).astype(np.float32)
    bm[0, 0] = 1
    if bmask == 'full':
        bm = bm * np.ones((1, 1, 4), np.float32)
    return ps, pr, T(sc), T(sm), T(bb), T(bm)


def test_module_imports_and_exports():
    from mmnas_amd import losses
    for name in ('VgdLoss', 'vgd_loss_fused', 'TripletBCELoss', 'TripletMarginLoss', 'fused'):
        assert hasattr(losses, name) and name in losses.__all__


@pytest.mark.parametrize('mode', ['kld', 'bce'])
@pytest.mark.parametrize('smask', ['full', 'row'])
@pytest.mark.parametrize('bmask', ['full', 'region'])
def test_vgd_loss_on_cpu_is_the_torch_composition(mode, smask, bmask):
    from mmnas_amd.harness import vgd_loss
    from mmnas_amd.losses import VgdLoss, vgd_loss_fused
    ps, pr, sc, sm, bb, bm = _vgd_inputs(smask=smask, bmask=bmask)
    ref = vgd_loss(ps, pr, sc, sm, bb, bm, lam=0.7, scores_loss=mode, loss_avg=True, batch_size=9)
    ref.backward()
    g_ref = (ps.grad.clone(), pr.grad.clone())
    ps.grad = pr.grad = None
    mod = VgdLoss(lam=0.7, scores_loss=mode, batch_size=9)
    for targets in (dict(scores=sc, scores_mask=sm, bbox=bb, bbox_mask=bm), (sc, sm, bb, bm)):
        loss = mod((ps, pr), targets)
        assert torch.equal(loss, ref)
        assert mod.parts is None                    # the torch composition has no parts vector
    loss.backward()
    assert torch.equal(ps.grad, g_ref[0]) and torch.equal(pr.grad, g_ref[1])
    assert torch.equal(vgd_loss_fused(ps, pr, sc, sm, bb, bm, lam=0.7, scores_loss=mode, batch_size=9), ref)
    assert torch.equal(vgd_loss_fused(ps, pr, sc, sm, bb, bm, loss_avg=False, scores_loss=mode),
                       vgd_loss(ps, pr, sc, sm, bb, bm, loss_avg=False, scores_loss=mode))


@pytest.mark.parametrize('reduction', ['sum', 'mean'])
def test_triplet_losses_on_cpu_are_the_torch_compositions(reduction):
    from mmnas_amd.harness import BCE_Loss
    from mmnas_amd.losses import TripletBCELoss, TripletMarginLoss
    from mmnas_amd.utils.itm_loss import Margin_Loss
    rs = np.random.RandomState(4)
    s = [T(rs.uniform(0.01, 0.99, 11).astype(np.float32)).requires_grad_() for _ in range(3)]
    cfg = SimpleNamespace(REDUCTION=reduction)
    for mine, ref in ((TripletBCELoss(cfg), BCE_Loss(cfg)), (TripletMarginLoss(cfg), Margin_Loss(cfg))):
        a = ref(*s)
        a.backward()
        g = [t.grad.clone() for t in s]
        for t in s:
            t.grad = None
        b = mine(*s)
        b.backward()
        assert torch.equal(a, b)
        for t, gr in zip(s, g):
            assert torch.equal(t.grad, gr)
            t.grad = None


def test_fused_maps_the_itm_losses_and_passes_others_through():
    from mmnas.utils.itm_loss import BCE_Loss as AliasBCE
    from mmnas_amd.harness import BCE_Loss
    from mmnas_amd.losses import TripletBCELoss, TripletMarginLoss, fused
    from mmnas_amd.utils.itm_loss import Margin_Loss
    f = fused(BCE_Loss(SimpleNamespace(REDUCTION='mean')))
    assert isinstance(f, TripletBCELoss) and f.reduction == 'mean'
    assert fused(BCE_Loss()).reduction == 'sum'
    assert isinstance(fused(AliasBCE()), TripletBCELoss)
    m = fused(Margin_Loss())
    assert isinstance(m, TripletMarginLoss) and m.margin == 0.2
    other = torch.nn.BCEWithLogitsLoss(reduction='sum')
    assert fused(other) is other
    assert fused(f) is f
    assert fused(None) is None


def test_cfg_fields_are_read():
    from mmnas_amd.losses import TripletBCELoss, VgdLoss
    v = VgdLoss(SimpleNamespace(LOSS_LAMBDA=0.25, SCORES_LOSS='bce', LOSS_AVG=False, BATCH_SIZE=48))
    assert (v.lam, v.scores_loss, v.loss_avg, v.batch_size) == (0.25, 'bce', False, 48)
    v = VgdLoss()
    assert (v.lam, v.scores_loss, v.loss_avg, v.batch_size) == (0.5, 'kld', True, None)
    v = VgdLoss(SimpleNamespace(LOSS_LAMBDA=2.0), scores_loss='bce')       # fields the cfg lacks come from the arguments
    assert (v.lam, v.scores_loss) == (2.0, 'bce')
    assert TripletBCELoss(SimpleNamespace(REDUCTION='mean')).reduction == 'mean'
    with pytest.raises(ValueError, match='SCORES_LOSS'):
        VgdLoss(SimpleNamespace(SCORES_LOSS='mse'))
    # the cfg's values reach the arithmetic
    from mmnas_amd.harness import vgd_loss
    ps, pr, sc, sm, bb, bm = _vgd_inputs()
    cfg = SimpleNamespace(LOSS_LAMBDA=0.25, SCORES_LOSS='bce', LOSS_AVG=True, BATCH_SIZE=48)
    assert torch.equal(VgdLoss(cfg)((ps, pr), (sc, sm, bb, bm)),
                       vgd_loss(ps, pr, sc, sm, bb, bm, lam=0.25, scores_loss='bce', loss_avg=True, batch_size=48))


def test_wrong_shapes_raise_naming_the_argument():
    from mmnas_amd.losses import TripletBCELoss, TripletMarginLoss, VgdLoss, vgd_loss_fused
    ps, pr, sc, sm, bb, bm = _vgd_inputs(B=4, S=6)
    with pytest.raises(ValueError, match='pred_scores'):
        vgd_loss_fused(ps[0], pr, sc, sm, bb, bm)
    with pytest.raises(ValueError, match='pred_reg'):
        vgd_loss_fused(ps, pr[:, :, :3], sc, sm, bb, bm)
    with pytest.raises(ValueError, match='scores must'):
        vgd_loss_fused(ps, pr, sc[:, :5], sm, bb, bm)
    with pytest.raises(ValueError, match='scores_mask'):
        vgd_loss_fused(ps, pr, sc, sm[:3], bb, bm)
    with pytest.raises(ValueError, match='bbox must'):
        vgd_loss_fused(ps, pr, sc, sm, bb[:, :5], bm)
    with pytest.raises(ValueError, match='bbox_mask'):
        vgd_loss_fused(ps, pr, sc, sm, bb, bm[:, :, :2])
    with pytest.raises(ValueError, match='targets'):
        VgdLoss()((ps, pr), (sc, sm, bb))
    with pytest.raises(ValueError, match='bbox_mask'):
        VgdLoss()((ps, pr), dict(scores=sc, scores_mask=sm, bbox=bb))
    with pytest.raises(ValueError, match='pred'):
        VgdLoss()(ps, (sc, sm, bb, bm))
    with pytest.raises(ValueError, match="'kld' or 'bce'"):
        vgd_loss_fused(ps, pr, sc, sm, bb, bm, scores_loss='mse')
    a, b = torch.rand(5), torch.rand(4)
    for cls in (TripletBCELoss, TripletMarginLoss):
        with pytest.raises(ValueError, match='scores_negc'):
            cls()(a, b, a)
        with pytest.raises(ValueError, match='scores_negi'):
            cls()(a, a, b)
    # a mask that broadcasts but is none of the kernel's layouts is the torch composition's business, not an error
    from mmnas_amd.harness import vgd_loss
    assert torch.equal(vgd_loss_fused(ps, pr, sc, sm[:1], bb, bm), vgd_loss(ps, pr, sc, sm[:1], bb, bm))


def test_new_symbols_are_declared_and_bound():
    from mmnas_amd import _lib as L
    src = open(os.path.join(REPO, 'include', 'mmnas_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, code), name
        assert name in L.SYMBOLS
    # each entry's comment cites the reference lines it replaces
    assert 'train_vgd.py:320-334' in src and 'mmnas/utils/itm_loss.py' in src
    assert 'losses.hip' in open(os.path.join(REPO, 'mmnas_amd', 'csrc', 'Makefile')).read()
    # argument counts of the binding follow the header
    for name in NEW_SYMBOLS:
        decl = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, code, flags=re.S).group(1)
        assert len(L.SYMBOLS[name][1]) == len(decl.split(',')), name


def test_host_side_argument_checks():
    """The C entries refuse bad arguments before any launch (no GPU needed: they return first)."""
    import ctypes
    from mmnas_amd import _lib as L
    l = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) & ~15
    assert l.mmnas_vgd_loss_fwd(p, p, p, p, p, p, 0, 5, 1, 1, 0, 1, 1.0, 0.5, p, p, None, None, None) == -1
    assert l.mmnas_vgd_loss_fwd(p, p, p, p, p, p, 2, 5, 1, 1, 2, 1, 1.0, 0.5, p, p, None, None, None) == -2
    assert l.mmnas_vgd_loss_fwd(p, None, p, p, p, p, 2, 5, 1, 1, 0, 1, 1.0, 0.5, p, p, None, None, None) == -2
    assert b'null pointer' in l.mmnas_last_error()
    assert l.mmnas_vgd_loss_fwd(p, p, p, p, p, p, 2, 5, 1, 1, 0, 1, 1.0, 0.5, p, p, p, None, None) == -2
    assert l.mmnas_vgd_loss_fwd(p, p + 4, p, p, p, p, 2, 5, 1, 1, 0, 1, 1.0, 0.5, p, p, None, None, None) == -2
    assert b'16-byte' in l.mmnas_last_error()
    assert l.mmnas_itm_triplet_loss_fwd(p, p, p, -1, 0, 0.2, 0, p, None, None) == -1
    assert l.mmnas_itm_triplet_loss_fwd(p, p, p, 4, 2, 0.2, 0, p, None, None) == -2
    assert l.mmnas_itm_triplet_loss_fwd(p, None, p, 4, 0, 0.2, 0, p, None, None) == -2
    assert l.mmnas_loss_grad_scale(None, None, None, 0, None) == 0        # nothing to do: nothing launched
    assert l.mmnas_loss_grad_scale(p, None, p, 4, None) == -2
