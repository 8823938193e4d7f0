"""Plain float64 references of the kernel-level operations, shared by tests/test_kernels_gpu.py and the child-process case
runner tests/fallback_cases.py.  CPU torch only: nothing here touches the GPU or the native library."""
import math

import numpy as np
import torch


def mha_ref(Q, K, V, mask, biasT, H, dh, dmask=None):
    """Multi-head attention core on [B, S, H * dh] tensors: softmax(q k^T / sqrt(dh) + biasT^T, masked keys at -1e9),
    optionally times a (scaled) dropout mask, times v."""
    B, Sq, _ = Q.shape
    Sk = K.shape[1]
    q = Q.reshape(B, Sq, H, dh).permute(0, 2, 1, 3)
    k = K.reshape(B, Sk, H, dh).permute(0, 2, 1, 3)
    v = V.reshape(B, Sk, H, dh).permute(0, 2, 1, 3)
    z = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if biasT is not None:
        z = z + biasT.permute(0, 1, 3, 2)
    if mask is not None:
        z = z.masked_fill(mask.reshape(B, 1, 1, Sk), -1e9)
    a = torch.softmax(z, -1)
    if dmask is not None:
        a = a * dmask
    return (a @ v).permute(0, 2, 1, 3).reshape(B, Sq, H * dh)


def _leaf(a):
    return torch.from_numpy(np.asarray(a)).double().requires_grad_(True)


def rel_fused_ref(raw, Wy, by, Wr, br, gb):
    """linear_y_rel -> relu -> linear_r -> relu -> log(clamp(., 1e-6)), transposed to [B, H, Sk, Sq]; backward of `gb`.
    -> (biasT, dWy, dby, dWr, dbr) as float64 numpy arrays."""
    Wyt, byt, Wrt, brt = _leaf(Wy), _leaf(by), _leaf(Wr), _leaf(br)
    rel = torch.relu(torch.from_numpy(raw).double() @ Wyt.t() + byt)
    r = torch.relu(rel @ Wrt.t() + brt)
    bias = torch.log(torch.clamp(r, min=1e-6)).permute(0, 3, 2, 1)
    bias.backward(torch.from_numpy(gb).double())
    return tuple(t.detach().numpy() for t in (bias, Wyt.grad, byt.grad, Wrt.grad, brt.grad))


def rel_multi_pre(raw, Wy, by, Wr, br):
    """The second layer's pre-activation of one relation operator, [B, H, Sk, Sq] (float64 numpy)."""
    T = lambda a: torch.from_numpy(a).double()
    rel = torch.relu(T(raw) @ T(Wy).t() + T(by))
    return (rel @ T(Wr).t() + T(br)).permute(0, 3, 2, 1).numpy()


def rel_multi_ref(raw, Wy, by, Wrs, brs, gbs, valid):
    """n operators sharing the stem layer: -> ([max(r, 1e-6) per operator], [dWr], [dbr], dWy, dby), float64 numpy; the bias
    gradients `gbs` count inside `valid` ([B, 1, S, S]) only."""
    Wyt, byt = _leaf(Wy), _leaf(by)
    rel = torch.relu(torch.from_numpy(raw).double() @ Wyt.t() + byt)
    vm = torch.from_numpy(valid).double()
    rs, dWr, dbr = [], [], []
    for Wr, br, gb in zip(Wrs, brs, gbs):
        Wrt, brt = _leaf(Wr), _leaf(br)
        r = torch.clamp(torch.relu(rel @ Wrt.t() + brt), min=1e-6).permute(0, 3, 2, 1)      # [B, H, S_k, S_q]
        (torch.log(r) * torch.from_numpy(gb).double() * vm).sum().backward(retain_graph=True)
        rs.append(r.detach().numpy()); dWr.append(Wrt.grad.numpy()); dbr.append(brt.grad.numpy())
    return rs, dWr, dbr, Wyt.grad.numpy(), byt.grad.numpy()
