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


def _T(a):
    return torch.from_numpy(np.asarray(a)).double()


def gemm_ref(layout, A, B):
    """op(A) op(B) of mmnas_gemm's three layouts (NT: A [M,K], B [N,K]; NN: B [K,N]; TN: A [K,M], B [K,N]) in float64."""
    A, B = _T(A), _T(B)
    return {'NT': lambda: A @ B.t(), 'NN': lambda: A @ B, 'TN': lambda: A.t() @ B}[layout]()


def gemm_epilogue_ref(acc, bias=None, relu=False, dmask=None, gate=None, gate_scale=1.0, residual=None):
    """mmnas_gemm's epilogue in its order: + bias; relu; * dropout multiplier; * (gate > 0 ? gate_scale : 0); + residual."""
    r = acc if bias is None else acc + _T(bias)
    if relu:
        r = torch.relu(r)
    if dmask is not None:
        r = r * _T(dmask)
    if gate is not None:
        r = torch.where(_T(gate) > 0, r * gate_scale, torch.zeros_like(r))
    return r if residual is None else r + _T(residual)


def layer_norm_ref(x, a, b, eps=1e-6):
    """modules.py:52-56: Bessel-corrected std, eps added to the std."""
    x = _T(x)
    return _T(a) * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + _T(b)


def layer_norm_bwd_ref(x, a, gy, eps=1e-6):
    """-> (dx, da, db) of layer_norm_ref by autograd in float64."""
    xt, at, bt = _leaf(x), _leaf(a), _leaf(np.zeros_like(np.asarray(a)))
    y = at * (xt - xt.mean(-1, keepdim=True)) / (xt.std(-1, keepdim=True) + eps) + bt
    y.backward(_T(gy))
    return xt.grad, at.grad, bt.grad


def rel_bias_ref(rel, Wr, br, gb):
    """log(clamp(relu(rel Wr^T + br), 1e-6)) transposed to [B, H, Sk, Sq] and the backward of `gb`:
    -> (biasT, drel, dWr, dbr) as float64 tensors."""
    relt, Wt, bt = _leaf(rel), _leaf(Wr), _leaf(br)
    r = torch.relu(relt @ Wt.t() + bt)                      # [B,Sq,Sk,H]
    bias = torch.log(torch.clamp(r, min=1e-6)).permute(0, 3, 2, 1)  # -> [B,H,Sk,Sq]
    bias.backward(_T(gb))
    return bias.detach(), relt.grad, Wt.grad, bt.grad


def attflat_pool_ref(logits, x, mask, gp):
    """Pooling stage of AttFlat (modules.py:78-84): masked softmax over the sequence + weighted sum; mask [B, S] bool or None.
    -> (pooled, dlogits, dx) for the output gradient gp."""
    lt, xt = _leaf(logits), _leaf(x)
    att = lt
    if mask is not None:
        att = att.masked_fill(torch.from_numpy(np.asarray(mask)).bool().unsqueeze(2), -1e9)
    att = torch.softmax(att, dim=1)
    G = lt.shape[2]
    ref = torch.cat([(att[:, :, g_:g_ + 1] * xt).sum(1) for g_ in range(G)], dim=1)
    ref.backward(_T(gp))
    return ref.detach(), lt.grad, xt.grad, att.detach()


def eltwise_ref(kind, x, gy):
    """kind 0 zero, 1 relu, 2 leaky-relu(0.01), 3 gelu-tanh (modules.py:96-119) -> (y, dx)."""
    xt = _leaf(x)
    if kind == 3:
        y = 0.5 * xt * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xt + 0.044715 * xt ** 3)))
    else:
        y = {0: lambda: xt * 0., 1: lambda: torch.relu(xt), 2: lambda: torch.nn.functional.leaky_relu(xt, 0.01)}[kind]()
    y.backward(_T(gy))
    return y.detach(), xt.grad


def glu_ref(h, gy, relu=False, dmask=None):
    """nn.GLU over the last dim, optional relu and dropout multiplier behind it -> (y, dh)."""
    ht = _leaf(h)
    a, b = ht.chunk(2, -1)
    r = a * torch.sigmoid(b)
    if relu:
        r = torch.relu(r)
    if dmask is not None:
        r = r * _T(dmask)
    r.backward(_T(gy))
    return r.detach(), ht.grad
