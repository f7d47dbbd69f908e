"""Ops of the less common layers: batch_norm, prelu, insanity, insanity_max_pooling, and of the
extensions batch_norm_ma, group_norm, add, ch_scale, relu6 / hsigmoid / hswish, silu, drop_path,
layer_norm, gelu, attention, window_attention, kv_attention, neighborhood_attention.

GPU: csrc/kernels/layer_kernels.hip.  CPU: the same formulas in fp32 torch, with the SAME
counter-hash random draws as the kernels (element index of the NHWC buffer, seed
hash(step counter, layer seed)), so the CPU executor is an exact oracle for the GPU one.
"""
from __future__ import annotations

import torch

from .. import native
from .mode import native as _native_t
from .gemm import _stream
from .nn import _hash_u32, effective_seed


def _k():
    return native.kernels()


def _ctr(counter):
    return counter.data_ptr() if counter is not None else None


def uniform_ref(n: int, seed: int, device="cpu") -> torch.Tensor:
    """u01 of layer_kernels.hip: hash_u32(i, seed) (csrc/kernels/common.h) * 2^-32 in fp32."""
    idx = torch.arange(n, dtype=torch.int64, device=device)
    return _hash_u32(idx, seed & 0xFFFFFFFF).to(torch.float32) * 2.3283064365386963e-10


def rand_fill(t: torch.Tensor, seed: int, dist: str, a: float, b: float):
    """Fill fp32 tensor t in place: dist "uniform" a + (b - a) u, "normal" a + b z.  On the
    GPU one rand_fill launch (layer_kernels.hip); on the host the same counter hash in int64
    arithmetic and the same float32 Box-Muller, chunked to bound the index arrays."""
    assert t.dtype == torch.float32 and t.is_contiguous()
    n = t.numel()
    d = 0 if dist == "uniform" else 1
    seed &= 0xFFFFFFFF
    if t.is_cuda:  # fp32 kernel: also in reference-precision mode
        native.check(_k().cxn_rand_fill(t.data_ptr(), n, seed, d, float(a), float(b), _stream()), "rand_fill")
        return t
    flat = t.view(-1)
    step = 1 << 24
    scale = torch.tensor(5.9604644775390625e-08, dtype=torch.float32)
    for lo in range(0, n, step):
        idx = torch.arange(lo, min(n, lo + step), dtype=torch.int64)
        u1 = (_hash_u32(2 * idx, seed) >> 8).to(torch.float32) * scale
        if d == 0:
            v = torch.tensor(a, dtype=torch.float32) + torch.tensor(b - a, dtype=torch.float32) * u1
        else:
            u2 = (_hash_u32(2 * idx + 1, seed) >> 8).to(torch.float32) * scale
            z = torch.sqrt(-2.0 * torch.log(1.0 - u1)) * torch.cos(6.283185307179586 * u2)
            v = torch.tensor(a, dtype=torch.float32) + torch.tensor(b, dtype=torch.float32) * z
        flat[lo:lo + idx.numel()] = v
    return t


# ----------------------------------------------------------------------------- batch norm
class BNState:
    """Per-layer device buffers: mean, inv (fp32 [C]), workspaces, the saved input copy."""

    def __init__(self, C, device):
        self.mean = torch.zeros(C, dtype=torch.float32, device=device)
        self.inv = torch.zeros(C, dtype=torch.float32, device=device)
        self.ws = torch.zeros(3 * C, dtype=torch.float32, device=device)
        self.coef = torch.zeros(3 * C, dtype=torch.float32, device=device)
        self.xsave = None


def bn_forward(x2d, y2d, slope, bias, eps, st: BNState, is_train: bool):
    """Reference BatchNormLayer::Forward (batch_norm_layer-inl.hpp:98-137): batch statistics in
    train AND test; in training the input node is overwritten with x-hat and a copy of x is
    kept for backward."""
    rows, C = x2d.shape
    if not _native_t(x2d):
        x = x2d.float()
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        inv = 1.0 / torch.sqrt(var + eps)
        xh = (x - mean) * inv
        st.mean.copy_(mean)
        st.inv.copy_(inv)
        if is_train:
            st.xsave = x2d.clone()
            x2d.copy_(xh)
        y2d.copy_(xh * slope + bias)
        return
    k = _k()
    native.check(k.cxn_bn_stats(x2d.data_ptr(), st.ws.data_ptr(), st.mean.data_ptr(), st.inv.data_ptr(), rows, C,
                                float(eps), _stream()), "bn_stats")
    xsave = None
    if is_train:
        if st.xsave is None or st.xsave.shape != x2d.shape:
            st.xsave = torch.empty_like(x2d)
        xsave = st.xsave
    # xhat overwrites x in place (element-wise: safe with y distinct)
    native.check(k.cxn_bn_fwd(x2d.data_ptr(), y2d.data_ptr(), x2d.data_ptr() if is_train else None,
                              xsave.data_ptr() if xsave is not None else None, st.mean.data_ptr(), st.inv.data_ptr(),
                              slope.data_ptr(), bias.data_ptr(), rows, C, _stream()), "bn_fwd")


def affine_forward(x2d, y2d, mean, inv, slope, bias):
    """y = (x - mean) * inv * slope + bias per channel (GPU; the bias layer uses it with 0/1/1)."""
    rows, C = x2d.shape
    native.check(_k().cxn_bn_fwd(x2d.data_ptr(), y2d.data_ptr(), None, None, mean.data_ptr(), inv.data_ptr(),
                                 slope.data_ptr(), bias.data_ptr(), rows, C, _stream()), "affine")


def bn_backward(g2d, dx2d, slope, gslope, gbias, st: BNState, prop_grad: bool):
    """Reference BatchNormLayer::Backprop (batch_norm_layer-inl.hpp:138-179)."""
    rows, C = g2d.shape
    if not _native_t(g2d):
        x = st.xsave.float()
        g = g2d.float()
        mean, inv = st.mean, st.inv
        scale = 1.0 / rows
        d = x - mean
        ve = 1.0 / (inv * inv)
        gvar = (g * slope * d).sum(0) * -0.5 * inv / ve
        gexp = (g * slope).sum(0) * -inv + gvar * scale * (-2.0 * d).sum(0)
        gslope.add_((g * d).sum(0) * inv)
        gbias.add_(g.sum(0))
        if prop_grad:
            dx2d.copy_(g * slope * inv + gvar * scale * 2.0 * d + gexp * scale)
        return
    if not prop_grad:
        # weight gradients only: the coefficient kernel also accumulates gslope/gbias
        dx2d = torch.empty_like(g2d)
    native.check(_k().cxn_bn_bwd(g2d.data_ptr(), st.xsave.data_ptr(), dx2d.data_ptr(), st.mean.data_ptr(),
                                 st.inv.data_ptr(), slope.data_ptr(), gslope.data_ptr(), gbias.data_ptr(),
                                 st.ws.data_ptr(), st.coef.data_ptr(), rows, C, _stream()), "bn_bwd")


# ----------------------------------------------------------------------------- batch norm (running statistics)
class BNMAState:
    """Per-layer device buffers of batch_norm_ma, sized once for max_rows: stat [5][C] =
    mean | var | inv | a | b of the last forward, the backward coefficients, the partial
    workspace of the fixed-order reductions (csrc/kernels/bn_ma_kernels.hip), and -- self-loop
    only -- the saved input."""

    def __init__(self, C, max_rows, device, dtype, keep_x):
        self.stat = torch.zeros(5, C, dtype=torch.float32, device=device)
        self.coef = torch.zeros(3, C, dtype=torch.float32, device=device)
        self.ws = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_bn_ma_ws_floats(int(max_rows), int(C)))
            self.ws = torch.zeros(max(n, 1), dtype=torch.float32, device=device)
        self.xsave = torch.zeros(max_rows, C, dtype=dtype, device=device) if keep_x else None


def bn_ma_forward(x2d, y2d, slope, bias, eps, momentum, st: BNMAState, rmean, rvar, is_train: bool):
    """Training: normalise with the batch's mean and biased variance and move the running
    statistics towards them (running <- m running + (1 - m) batch).  Inference: normalise with
    the running statistics alone.  y may alias x when st.xsave keeps the input (self-loop)."""
    rows, C = x2d.shape
    xsave = st.xsave[:rows] if (st.xsave is not None and is_train) else None
    if not _native_t(x2d):
        x = x2d.float()
        if is_train:
            mean = x.mean(0)
            var = ((x - mean) ** 2).mean(0)
            rmean.copy_(momentum * rmean + (1.0 - momentum) * mean)
            rvar.copy_(momentum * rvar + (1.0 - momentum) * var)
            if xsave is not None:
                xsave.copy_(x2d)
        else:
            mean, var = rmean, rvar
        inv = 1.0 / torch.sqrt(var + eps)
        if is_train:
            st.stat[0].copy_(mean)
            st.stat[1].copy_(var)
            st.stat[2].copy_(inv)
        y2d.copy_((x - mean) * inv * slope + bias)
        return
    k = _k()
    if is_train:
        native.check(k.cxn_bn_ma_fwd_train(x2d.data_ptr(), y2d.data_ptr(), xsave.data_ptr() if xsave is not None else None,
                                           slope.data_ptr(), bias.data_ptr(), st.stat.data_ptr(), rmean.data_ptr(),
                                           rvar.data_ptr(), st.ws.data_ptr(), st.ws.numel(), rows, C, float(eps),
                                           float(momentum), _stream()), "bn_ma_fwd_train")
    else:
        native.check(k.cxn_bn_ma_fwd_infer(x2d.data_ptr(), y2d.data_ptr(), slope.data_ptr(), bias.data_ptr(),
                                           rmean.data_ptr(), rvar.data_ptr(), st.stat.data_ptr(), rows, C, float(eps),
                                           _stream()), "bn_ma_fwd_infer")


def bn_ma_backward(g2d, x2d, dx2d, slope, gslope, gbias, st: BNMAState, prop_grad: bool):
    """gslope += sum g xhat, gbias += sum g, dx = a (g - sum g / R - xhat sum(g xhat) / R) with
    xhat = (x - mean) inv, a = slope inv of the last training forward.  dx may alias x or g."""
    rows, C = g2d.shape
    if not _native_t(g2d):
        g, x = g2d.float(), x2d.float()
        mean, inv = st.stat[0], st.stat[2]
        xh = (x - mean) * inv
        sg, sgx = g.sum(0), (g * xh).sum(0)
        gslope.add_(sgx)
        gbias.add_(sg)
        if prop_grad:
            dx2d.copy_(slope * inv * (g - sg / rows - xh * sgx / rows))
        return
    native.check(_k().cxn_bn_ma_bwd(g2d.data_ptr(), x2d.data_ptr(), dx2d.data_ptr() if prop_grad else None,
                                    slope.data_ptr(), gslope.data_ptr(), gbias.data_ptr(), st.stat.data_ptr(),
                                    st.coef.data_ptr(), st.ws.data_ptr(), st.ws.numel(), rows, C, _stream()),
                 "bn_ma_bwd")


# ----------------------------------------------------------------------------- group norm
class GNState:
    """Per-layer device buffers of group_norm, sized once for max_batch: mean and rstd [B][groups]
    of the last forward, the backward's per-group coefficients (s1 / m, s2 / m), and the partial
    workspace of the fixed-order reductions (csrc/kernels/gn_kernels.hip).  A smaller batch uses
    their leading rows."""

    def __init__(self, max_batch, HW, C, groups, device):
        self.groups = int(groups)
        self.mean = torch.zeros(max_batch, groups, dtype=torch.float32, device=device)
        self.rstd = torch.zeros(max_batch, groups, dtype=torch.float32, device=device)
        self.coef = torch.zeros(max_batch, groups, 2, dtype=torch.float32, device=device)
        self.ws = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_gn_ws_floats(int(max_batch), int(HW), int(C)))
            self.ws = torch.zeros(max(n, 1), dtype=torch.float32, device=device)


def _gn_dims(x, st, who):
    B, HW, C = x.shape
    if C % st.groups != 0 or B > st.mean.shape[0]:
        raise ValueError("%s: x [B][HW][C] with C a multiple of the %d groups and B <= %d expected, not %s"
                         % (who, st.groups, st.mean.shape[0], tuple(x.shape)))
    return B, HW, C, st.groups


def gn_forward(x, y, slope, bias, eps, st: GNState):
    """x, y [B][HW][C].  Per sample b and group g (channels [g Cg, (g + 1) Cg), m = HW Cg
    elements): mean, biased var, rstd = (var + eps)^-1/2 into st.mean / st.rstd [b][g], and
    y = (x - mean) rstd slope[c] + bias[c].  The same in training and inference.  y must not
    alias x."""
    B, HW, C, G = _gn_dims(x, st, "gn_forward")
    if x.data_ptr() == y.data_ptr():
        raise ValueError("gn_forward: y must not alias x (backward reads x again)")
    if not _native_t(x):
        xg = x.float().reshape(B, HW, G, C // G)
        mean = xg.mean((1, 3), keepdim=True)
        d = xg - mean
        var = (d * d).mean((1, 3), keepdim=True)
        rstd = 1.0 / torch.sqrt(var + eps)
        st.mean[:B].copy_(mean.reshape(B, G))
        st.rstd[:B].copy_(rstd.reshape(B, G))
        y.copy_((d * rstd).reshape(B, HW, C) * slope + bias)
        return
    _flat_bf16(x, y, who="gn_forward")
    native.check(_k().cxn_gn_fwd(x.data_ptr(), y.data_ptr(), slope.data_ptr(), bias.data_ptr(), st.mean.data_ptr(),
                                 st.rstd.data_ptr(), st.ws.data_ptr(), st.ws.numel(), B, HW, C, G, float(eps),
                                 _stream()), "gn_fwd")


def gn_backward(g, x, dx, slope, gslope, gbias, st: GNState, prop_grad: bool):
    """With xhat = (x - mean) rstd of the last forward: gbias[c] += sum g, gslope[c] += sum g xhat
    (over the batch and the map), and with prop_grad dx = rstd (slope[c] g - s1 / m - xhat s2 / m),
    s1 = sum slope g and s2 = sum slope g xhat over the m elements of the (sample, group).  dx may
    alias x or g; without prop_grad it is not written."""
    B, HW, C, G = _gn_dims(g, st, "gn_backward")
    if not _native_t(g):
        Cg = C // G
        mean, rstd = st.mean[:B].reshape(B, 1, G, 1), st.rstd[:B].reshape(B, 1, G, 1)
        g32 = g.float().reshape(B, HW, G, Cg)
        xh = (x.float().reshape(B, HW, G, Cg) - mean) * rstd
        gbias.add_(g32.sum((0, 1)).reshape(C))
        gslope.add_((g32 * xh).sum((0, 1)).reshape(C))
        if prop_grad:
            sg = g32 * slope.reshape(G, Cg)
            m = float(HW * Cg)
            s1 = sg.sum((1, 3), keepdim=True)
            s2 = (sg * xh).sum((1, 3), keepdim=True)
            dx.copy_((rstd * (sg - s1 / m - xh * s2 / m)).reshape(B, HW, C))
        return
    _flat_bf16(g, x, who="gn_backward")
    if prop_grad:
        _flat_bf16(dx, who="gn_backward")
    native.check(_k().cxn_gn_bwd(g.data_ptr(), x.data_ptr(), dx.data_ptr() if prop_grad else None, slope.data_ptr(),
                                 gslope.data_ptr(), gbias.data_ptr(), st.mean.data_ptr(), st.rstd.data_ptr(),
                                 st.coef.data_ptr(), st.ws.data_ptr(), st.ws.numel(), B, HW, C, G, _stream()),
                 "gn_bwd")


# ----------------------------------------------------------------------------- layer norm
class LNState:
    """Per-layer device buffers of layer_norm, sized once for the largest batch: mean and rstd
    [rows] of the last forward and the slab workspace of the backward's fixed-order column sums
    (csrc/kernels/ln_kernels.hip).  A smaller batch uses their leading rows."""

    def __init__(self, max_rows, C, device):
        self.mean = torch.zeros(max_rows, dtype=torch.float32, device=device)
        self.rstd = torch.zeros(max_rows, dtype=torch.float32, device=device)
        self.ws = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_ln_ws_floats(int(max_rows), int(C)))
            self.ws = torch.zeros(max(n, 1), dtype=torch.float32, device=device)


def ln_rows_per_block(C: int) -> int:
    """Rows one block of the layer_norm kernels holds at C channels."""
    return int(_k().cxn_ln_rows_per_block(int(C)))


def ln_forward(x, y, slope, bias, eps, st: LNState):
    """x, y [rows][C].  Per row: mean, biased var over C, rstd = (var + eps)^-1/2 into st.mean /
    st.rstd, and y = (x - mean) rstd slope[c] + bias[c].  y must not alias x."""
    rows, C = x.shape
    if rows > st.mean.shape[0]:
        raise ValueError("ln_forward: %d rows, state sized for %d" % (rows, st.mean.shape[0]))
    if x.data_ptr() == y.data_ptr():
        raise ValueError("ln_forward: y must not alias x (backward reads x again)")
    if not _native_t(x):
        v = x.float()
        mean = v.mean(1, keepdim=True)
        d = v - mean
        rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
        st.mean[:rows].copy_(mean.reshape(rows))
        st.rstd[:rows].copy_(rstd.reshape(rows))
        y.copy_(d * rstd * slope + bias)
        return
    _flat_bf16(x, y, who="ln_forward")
    native.check(_k().cxn_ln_fwd(x.data_ptr(), y.data_ptr(), slope.data_ptr(), bias.data_ptr(), st.mean.data_ptr(),
                                 st.rstd.data_ptr(), rows, C, float(eps), _stream()), "ln_fwd")


def ln_backward(g, x, dx, slope, gslope, gbias, st: LNState, prop_grad: bool):
    """With xhat = (x - mean) rstd of the last forward: gbias[c] += sum g, gslope[c] += sum g xhat
    over the rows, and with prop_grad dx = rstd (slope[c] g - s1 / C - xhat s2 / C), s1 = sum
    slope g and s2 = sum slope g xhat over the row.  dx may alias x or g; without prop_grad it is
    not written."""
    rows, C = g.shape
    if not _native_t(g):
        mean, rstd = st.mean[:rows].reshape(rows, 1), st.rstd[:rows].reshape(rows, 1)
        g32 = g.float()
        xh = (x.float() - mean) * rstd
        gbias.add_(g32.sum(0))
        gslope.add_((g32 * xh).sum(0))
        if prop_grad:
            sg = g32 * slope
            s1 = sg.sum(1, keepdim=True)
            s2 = (sg * xh).sum(1, keepdim=True)
            dx.copy_(rstd * (sg - s1 / C - xh * s2 / C))
        return
    _flat_bf16(g, x, who="ln_backward")
    if prop_grad:
        _flat_bf16(dx, who="ln_backward")
    native.check(_k().cxn_ln_bwd(g.data_ptr(), x.data_ptr(), dx.data_ptr() if prop_grad else None, slope.data_ptr(),
                                 gslope.data_ptr(), gbias.data_ptr(), st.mean.data_ptr(), st.rstd.data_ptr(),
                                 st.ws.data_ptr(), st.ws.numel(), rows, C, _stream()), "ln_bwd")


# ----------------------------------------------------------------------------- attention
class AttnState:
    """Per-layer device buffers of attention, sized once for the largest batch: the fp32
    log-sum-exp of every softmax row and the backward's row term D, [B nhead T] each, and the
    [B T][C] staging buffer dQ passes through when the gradient overwrites qkv in place
    (csrc/kernels/attn_kernels.hip).  A smaller batch uses their leading part."""

    def __init__(self, max_batch, T, C, nhead, device, dtype=torch.bfloat16):
        self.lse = torch.zeros(max_batch * nhead * T, dtype=torch.float32, device=device)
        self.lse2 = torch.zeros(max_batch * nhead * T, dtype=torch.float32, device=device)  # lse in log2 units (HIP path)
        self.dsum = torch.zeros(max_batch * nhead * T, dtype=torch.float32, device=device)
        self.dq = torch.zeros(max_batch * T, C, dtype=dtype, device=device) if dtype == torch.bfloat16 else None


def attn_tile(d: int):
    """(rows a block owns, keys per streamed chunk) of the attention kernels at head width d."""
    import ctypes
    r, k = ctypes.c_int(0), ctypes.c_int(0)
    native.check(_k().cxn_attn_tile(int(d), ctypes.byref(r), ctypes.byref(k)), "attn_tile")
    return r.value, k.value


def _attn_heads(qkv, B, nhead):
    """q, k, v as [B, nhead, T, d] fp32 views-turned-copies of qkv [B T][3 C]."""
    rows, C3 = qkv.shape
    T, C = rows // B, C3 // 3
    v = qkv.float().view(B, T, 3, nhead, C // nhead).permute(2, 0, 3, 1, 4)
    return v[0], v[1], v[2]


def _bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def attn_forward(qkv, out, B, nhead, st: AttnState, bf16_products=False):
    """qkv [B T][3 C] (channel s C + h d + j: component j of head h of q, k, v for s = 0, 1, 2),
    out [B T][C].  Per sample and head O = softmax(Q K^T / sqrt(d)) V with the softmax in fp32;
    st.lse receives every row's log-sum-exp.  out must not alias qkv.  bf16_products (torch path
    only): round P to bf16 before P V as the HIP kernels do, to measure what that rounding adds."""
    rows, C3 = qkv.shape
    T, C = rows // B, C3 // 3
    if B * nhead * T > st.lse.shape[0]:
        raise ValueError("attn_forward: batch %d, state sized for %d rows" % (B, st.lse.shape[0]))
    if qkv.data_ptr() == out.data_ptr():
        raise ValueError("attn_forward: out must not alias qkv (backward reads qkv again)")
    if not _native_t(qkv):
        q, k, v = _attn_heads(qkv, B, nhead)
        s = q @ k.transpose(-1, -2) / (C // nhead) ** 0.5
        lse = torch.logsumexp(s, -1, keepdim=True)
        st.lse[:B * nhead * T].copy_(lse.reshape(-1))
        p = torch.exp(s - lse)
        o = (_bf16_round(p) if bf16_products else p) @ v
        out.copy_(o.permute(0, 2, 1, 3).reshape(rows, C))
        return
    _flat_bf16(qkv, out, who="attn_forward")
    native.check(_k().cxn_attn_fwd(qkv.data_ptr(), out.data_ptr(), st.lse.data_ptr(), st.lse2.data_ptr(), B, T, C, nhead,
                                   _stream()), "attn_fwd")


def attn_backward(g, qkv, dqkv, B, nhead, st: AttnState, prop_grad: bool, bf16_products=False):
    """g [B T][C] = dO.  With P = exp(S - lse) of the last forward, dP = dO V^T and
    D_i = sum_j P_ij dP_ij (into st.dsum): dV = P^T dO, dS = P (dP - D), dQ = dS K / sqrt(d),
    dK = dS^T Q / sqrt(d), written as [B T][3 C] into dqkv, which may be qkv.  Without prop_grad
    nothing is computed or written.  bf16_products (torch path only): P and dS are rounded to bf16
    before the three products that take them, as in the HIP kernels."""
    if not prop_grad:
        return
    rows, C3 = qkv.shape
    T, C = rows // B, C3 // 3
    if not _native_t(g):
        q, k, v = _attn_heads(qkv, B, nhead)
        sc = 1.0 / (C // nhead) ** 0.5
        do = g.float().view(B, T, nhead, C // nhead).permute(0, 2, 1, 3)
        p = torch.exp(q @ k.transpose(-1, -2) * sc - st.lse[:B * nhead * T].view(B, nhead, T, 1))
        dp = do @ v.transpose(-1, -2)
        d = (p * dp).sum(-1, keepdim=True)
        st.dsum[:B * nhead * T].copy_(d.reshape(-1))
        ds = p * (dp - d)
        if bf16_products:
            p, ds = _bf16_round(p), _bf16_round(ds)
        grads = torch.stack([ds @ k * sc, ds.transpose(-1, -2) @ q * sc, p.transpose(-1, -2) @ do])
        dqkv.copy_(grads.permute(1, 3, 0, 2, 4).reshape(rows, C3))
        return
    _flat_bf16(g, qkv, dqkv, who="attn_backward")
    native.check(_k().cxn_attn_bwd(qkv.data_ptr(), g.data_ptr(), st.lse2.data_ptr(), st.dsum.data_ptr(),
                                   dqkv.data_ptr(), st.dq.data_ptr(), B, T, C, nhead, _stream()), "attn_bwd")


# ----------------------------------------------------------------------------- window attention
class WAttnState:
    """Per-layer device buffers of window_attention, sized once for the largest batch: the fp32
    log-sum-exp of every softmax row, [B nhead H W] at the row's map position (lse2: the same in the
    kernels' log2 units), and the slab workspace of the bias gradient
    (csrc/kernels/wattn_kernels.hip).  A smaller batch uses their leading part."""

    def __init__(self, max_batch, H, W, C, nhead, ws, shift, device, dtype=torch.float32):
        self.geom = (int(H), int(W), int(ws), int(shift))
        self.lse = torch.zeros(max_batch * nhead * H * W, dtype=dtype, device=device)  # (fp64: the torch path's tests)
        self.lse2 = torch.zeros(max_batch * nhead * H * W, dtype=torch.float32, device=device)
        self.ws = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_wattn_ws_floats(int(max_batch), int(H), int(W), int(C), int(nhead), int(ws), int(shift)))
            self.ws = torch.zeros(max(n, 1), dtype=torch.float32, device=device)
        self._index = None

    def index(self, device):
        """pos [nwin][n]: the map position y W + x of token t = wy ws + wx of every window; rel
        [n][n]: the bias index of (query, key); on [nwin][n][n]: the key is attended (equal wrap
        flags).  Index arithmetic on the map, computed once."""
        if self._index is None:
            H, W, ws, shift = self.geom
            win = torch.arange((H // ws) * (W // ws), device=device)[:, None]
            t = torch.arange(ws * ws, device=device)
            wy, wx = t // ws, t % ws
            yr, xr = win // (W // ws) * ws + wy + shift, win % (W // ws) * ws + wx + shift
            fy, fx = yr >= H, xr >= W
            pos = (yr % H) * W + xr % W
            rel = (wy[:, None] - wy[None] + ws - 1) * (2 * ws - 1) + wx[:, None] - wx[None] + ws - 1
            on = (fy[:, :, None] == fy[:, None, :]) & (fx[:, :, None] == fx[:, None, :])
            self._index = pos, rel, on
        return self._index


def _wattn_logits(qkv, bias, B, nhead, st):
    """the windows' q, k, v [B, nwin, nhead, n, d] gathered from qkv [B H W][3 C] and the masked,
    biased logits [B, nwin, nhead, n, n], in qkv's precision (fp32 at least)"""
    pos, rel, on = st.index(qkv.device)
    d = qkv.shape[1] // (3 * nhead)
    x = qkv if qkv.dtype == torch.float64 else qkv.float()
    x = x.view(B, -1, 3, nhead, d)[:, pos].permute(3, 0, 1, 4, 2, 5)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) / d ** 0.5 + bias.to(x.dtype)[:, rel]
    return q, k, v, s.masked_fill(~on[:, None], float("-inf")), pos, rel


def wattn_forward(qkv, out, bias, B, nhead, st: WAttnState, bf16_products=False):
    """qkv [B H W][3 C] in attention's channel layout, out [B H W][C], bias [nhead][(2 ws - 1)^2]
    fp32.  Per sample, window and head O = softmax(Q K^T / sqrt(d) + bias, keys across a wrap of the
    cyclic shift excluded) V, written back to the tokens' map positions; st.lse receives every
    row's log-sum-exp.  out must not alias qkv.  bf16_products: as attn_forward."""
    H, W, ws, shift = st.geom
    rows, C3 = qkv.shape
    C = C3 // 3
    if rows != B * H * W or B * nhead * H * W > st.lse.shape[0]:
        raise ValueError("wattn_forward: %d rows at batch %d, state sized for %d" % (rows, B, st.lse.shape[0]))
    if qkv.data_ptr() == out.data_ptr():
        raise ValueError("wattn_forward: out must not alias qkv (backward reads qkv again)")
    if not _native_t(qkv):
        q, k, v, s, pos, _ = _wattn_logits(qkv, bias, B, nhead, st)
        lse = torch.logsumexp(s, -1, keepdim=True)
        st.lse[:B * nhead * H * W].view(B, nhead, H * W)[:, :, pos.reshape(-1)] = \
            lse.permute(0, 2, 1, 3, 4).reshape(B, nhead, -1).to(st.lse.dtype)
        p = torch.exp(s - lse)
        o = (_bf16_round(p) if bf16_products else p) @ v
        out.view(B, H * W, C)[:, pos.reshape(-1)] = o.permute(0, 1, 3, 2, 4).reshape(B, H * W, C).to(out.dtype)
        return
    _flat_bf16(qkv, out, who="wattn_forward")
    native.check(_k().cxn_wattn_fwd(qkv.data_ptr(), out.data_ptr(), bias.data_ptr(), st.lse.data_ptr(),
                                    st.lse2.data_ptr(), B, H, W, C, nhead, ws, shift, _stream()), "wattn_fwd")


def wattn_backward(g, qkv, dqkv, bias, gbias, B, nhead, st: WAttnState, prop_grad: bool, bf16_products=False):
    """g [B H W][C] = dO.  With P of the last forward, dP = dO V^T, D_i = sum_j P_ij dP_ij and
    dS = P (dP - D): gbias[h][r] += sum of dS over the batch, the windows and the pairs at relative
    index r (always), and with prop_grad dV = P^T dO, dQ = dS K / sqrt(d), dK = dS^T Q / sqrt(d) into
    dqkv [B H W][3 C], which may be qkv.  bf16_products: as attn_backward (gbias takes the unrounded
    dS either way, as in the kernels)."""
    H, W, ws, shift = st.geom
    rows, C3 = qkv.shape
    C = C3 // 3
    if not _native_t(g):
        q, k, v, s, pos, rel = _wattn_logits(qkv, bias, B, nhead, st)
        n, d = ws * ws, C // nhead
        sc = 1.0 / d ** 0.5
        do = (g if g.dtype == torch.float64 else g.float()).view(B, H * W, nhead, d)[:, pos].permute(0, 1, 3, 2, 4)
        lse = st.lse[:B * nhead * H * W].view(B, nhead, H * W)[:, :, pos].permute(0, 2, 1, 3).unsqueeze(-1)
        p = torch.exp(s - lse.to(s.dtype))
        dp = do @ v.transpose(-1, -2)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        gbias.index_add_(1, rel.reshape(-1), ds.sum((0, 1)).reshape(nhead, n * n).to(gbias.dtype))
        if not prop_grad:
            return
        if bf16_products:
            p, ds = _bf16_round(p), _bf16_round(ds)
        grads = torch.stack([ds @ k * sc, ds.transpose(-1, -2) @ q * sc, p.transpose(-1, -2) @ do])
        dqkv.view(B, H * W, 3, nhead, d)[:, pos.reshape(-1)] = \
            grads.permute(1, 2, 4, 0, 3, 5).reshape(B, H * W, 3, nhead, d).to(dqkv.dtype)
        return
    _flat_bf16(g, qkv, who="wattn_backward")
    if prop_grad:
        _flat_bf16(dqkv, who="wattn_backward")
    native.check(_k().cxn_wattn_bwd(qkv.data_ptr(), g.data_ptr(), bias.data_ptr(), st.lse2.data_ptr(),
                                    dqkv.data_ptr() if prop_grad else None, gbias.data_ptr(), st.ws.data_ptr(),
                                    st.ws.numel(), B, H, W, C, nhead, ws, shift, _stream()), "wattn_bwd")


# ----------------------------------------------------------------------------- neighborhood attention
class NAttnState:
    """Per-layer device buffers of neighborhood_attention, sized once for the largest batch: the
    fp32 log-sum-exp of every softmax row, [B nhead H W] (lse2: the same in the kernels' log2
    units), the backward's row term D, the [B H W][C] staging buffer dQ passes through when the
    gradient overwrites qkv in place (allocated by the first such call), and the slab workspace of
    the bias gradient, sized for every batch up to the largest (csrc/kernels/nattn_kernels.hip).  A
    smaller batch uses their leading part."""

    def __init__(self, max_batch, H, W, C, nhead, kernel, device, dtype=torch.float32):
        self.geom = (int(H), int(W), int(kernel))
        n = max_batch * nhead * H * W
        self.lse = torch.zeros(n, dtype=dtype, device=device)  # (fp64: the torch path's tests)
        self.lse2 = torch.zeros(n, dtype=torch.float32, device=device)
        self.dsum = torch.zeros(n, dtype=torch.float32, device=device)
        self.ws = self.dq = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_nattn_ws_floats(int(max_batch), int(H), int(W), int(C), int(nhead), int(kernel)))
            self.ws = torch.zeros(max(n, 1), dtype=torch.float32, device=device)
        self._dq_shape = (max_batch * H * W, C)
        self._index = None

    def stage(self, device):
        """the dQ staging buffer of an in-place backward"""
        if self.dq is None:
            self.dq = torch.zeros(self._dq_shape, dtype=torch.bfloat16, device=device)
        return self.dq

    def index(self, device):
        """nbr [H W][k k]: the map positions y' W + x' of the keys of every query, NAT's clamped
        neighbourhood (rows clamp(y - k // 2, 0, H - k) .., columns likewise); rel [H W][k k]: their
        bias indices (y' - y + k - 1) (2 k - 1) + x' - x + k - 1.  Computed once."""
        if self._index is None:
            H, W, k = self.geom
            ys, xs, kk = torch.arange(H, device=device), torch.arange(W, device=device), torch.arange(k, device=device)
            ky = (ys - k // 2).clamp(0, H - k)[:, None] + kk  # [H, k]
            kx = (xs - k // 2).clamp(0, W - k)[:, None] + kk  # [W, k]
            nbr = ky[:, None, :, None] * W + kx[None, :, None, :]
            rel = (ky - ys[:, None] + k - 1)[:, None, :, None] * (2 * k - 1) + (kx - xs[:, None] + k - 1)[None, :, None, :]
            self._index = nbr.reshape(H * W, k * k), rel.reshape(H * W, k * k)
        return self._index


def _nattn_logits(qkv, bias, B, nhead, st):
    """q [B, HW, nhead, d], the gathered k and v [B, HW, k k, nhead, d] of qkv [B H W][3 C] and the
    biased logits [B, nhead, HW, k k], in qkv's precision (fp32 at least)"""
    nbr, rel = st.index(qkv.device)
    d = qkv.shape[1] // (3 * nhead)
    x = (qkv if qkv.dtype == torch.float64 else qkv.float()).view(B, -1, 3, nhead, d)
    q, k, v = x[:, :, 0], x[:, :, 1][:, nbr], x[:, :, 2][:, nbr]
    s = torch.einsum("bphd,bpjhd->bhpj", q, k) / d ** 0.5 + bias.to(x.dtype)[:, rel]
    return q, k, v, s, nbr, rel


def nattn_forward(qkv, out, bias, B, nhead, st: NAttnState, bf16_products=False):
    """qkv [B H W][3 C] in attention's channel layout, out [B H W][C], bias [nhead][(2 k - 1)^2] fp32.
    Per sample, head and pixel O = softmax(q K^T / sqrt(d) + bias) V over the k k keys of the pixel's
    clamped neighbourhood; st.lse receives every row's log-sum-exp.  out must not alias qkv.
    bf16_products: as attn_forward."""
    H, W, k = st.geom
    rows, C3 = qkv.shape
    C = C3 // 3
    n = B * nhead * H * W
    if rows != B * H * W or n > st.lse.shape[0]:
        raise ValueError("nattn_forward: %d rows at batch %d, state sized for %d" % (rows, B, st.lse.shape[0]))
    if qkv.data_ptr() == out.data_ptr():
        raise ValueError("nattn_forward: out must not alias qkv (backward reads qkv again)")
    if not _native_t(qkv):
        _, _, v, s, _, _ = _nattn_logits(qkv, bias, B, nhead, st)
        lse = torch.logsumexp(s, -1, keepdim=True)
        st.lse[:n].copy_(lse.reshape(-1))
        p = torch.exp(s - lse)
        out.copy_(torch.einsum("bhpj,bpjhd->bphd", _bf16_round(p) if bf16_products else p, v).reshape(rows, C))
        return
    _flat_bf16(qkv, out, who="nattn_forward")
    native.check(_k().cxn_nattn_fwd(qkv.data_ptr(), out.data_ptr(), bias.data_ptr(), st.lse.data_ptr(),
                                    st.lse2.data_ptr(), B, H, W, C, nhead, k, _stream()), "nattn_fwd")


def nattn_backward(g, qkv, dqkv, bias, gbias, B, nhead, st: NAttnState, prop_grad: bool, bf16_products=False):
    """g [B H W][C] = dO.  With P of the last forward, dP = dO V^T, D_i = sum_j P_ij dP_ij (into
    st.dsum) and dS = P (dP - D) over each pixel's neighbourhood: gbias[h][r] += sum of dS over the
    batch and the (query, key) pairs at relative index r (always), and with prop_grad dQ = dS K /
    sqrt(d), dK = dS^T Q / sqrt(d), dV = P^T dO -- a key collects from every query that attends it --
    into dqkv [B H W][3 C], which may be qkv (dQ then passes through st.dq).  bf16_products: as
    attn_backward (gbias takes the unrounded dS either way, as in the kernels)."""
    H, W, k = st.geom
    rows, C3 = qkv.shape
    C = C3 // 3
    n = B * nhead * H * W
    if not _native_t(g):
        q, kk, v, s, nbr, rel = _nattn_logits(qkv, bias, B, nhead, st)
        d = C // nhead
        sc = 1.0 / d ** 0.5
        do = (g if g.dtype == torch.float64 else g.float()).view(B, H * W, nhead, d)
        p = torch.exp(s - st.lse[:n].view(B, nhead, H * W, 1).to(s.dtype))
        dp = torch.einsum("bphd,bpjhd->bhpj", do, v)
        dsum = (p * dp).sum(-1, keepdim=True)
        st.dsum[:n].copy_(dsum.reshape(-1))
        ds = p * (dp - dsum)
        gbias.index_add_(1, rel.reshape(-1), ds.sum(0).reshape(nhead, -1).to(gbias.dtype))
        if not prop_grad:
            return
        if bf16_products:
            p, ds = _bf16_round(p), _bf16_round(ds)
        dq = torch.einsum("bhpj,bpjhd->bphd", ds, kk) * sc
        zero = torch.zeros_like(dq)
        dk = zero.index_add(1, nbr.reshape(-1), (torch.einsum("bhpj,bphd->bpjhd", ds, q) * sc).reshape(B, -1, nhead, d))
        dv = zero.index_add(1, nbr.reshape(-1), torch.einsum("bhpj,bphd->bpjhd", p, do).reshape(B, -1, nhead, d))
        dqkv.copy_(torch.stack([dq, dk, dv], 2).reshape(rows, C3))
        return
    _flat_bf16(g, qkv, who="nattn_backward")
    if prop_grad:
        _flat_bf16(dqkv, who="nattn_backward")
    stage = st.stage(qkv.device).data_ptr() if prop_grad and dqkv.data_ptr() == qkv.data_ptr() else None
    native.check(_k().cxn_nattn_bwd(qkv.data_ptr(), g.data_ptr(), bias.data_ptr(), st.lse2.data_ptr(),
                                    st.dsum.data_ptr(), dqkv.data_ptr() if prop_grad else None, stage,
                                    gbias.data_ptr(), st.ws.data_ptr(), st.ws.numel(), B, H, W, C, nhead, k,
                                    _stream()), "nattn_bwd")


# ----------------------------------------------------------------------------- kv attention
class KVAttnState:
    """Per-layer device buffers of kv_attention, sized once for the largest batch: the fp32
    log-sum-exp of every query row, [B nhead Tq] (the torch path's backward reads it; the kernels'
    backward normalises its own softmax again, see csrc/kernels/kvattn_kernels.hip), and the slab
    workspace of dK / dV when the queries are split (csrc/kernels/kvattn_kernels.hip).  A
    smaller batch uses their leading part."""

    def __init__(self, max_batch, Tq, Tk, C, nhead, device, dtype=torch.float32):
        self.lse = torch.zeros(max_batch * nhead * Tq, dtype=dtype, device=device)  # (fp64: the torch path's tests)
        self.ws = None
        if torch.device(device).type == "cuda":
            n = int(_k().cxn_kvattn_ws_floats(int(max_batch), int(Tq), int(Tk), int(C), int(nhead)))
            if n < 0:
                raise ValueError("KVAttnState: Tq %d, Tk %d, C %d, nhead %d is not served" % (Tq, Tk, C, nhead))
            self.ws = torch.zeros(max(n, 4), dtype=torch.float32, device=device)


def kvattn_tile(d: int, Tq: int):
    """(queries per tile, splits of the backward over Tq queries) of the kv_attention kernels."""
    import ctypes
    r, s = ctypes.c_int(0), ctypes.c_int(0)
    native.check(_k().cxn_kvattn_tile(int(d), int(Tq), ctypes.byref(r), ctypes.byref(s)), "kvattn_tile")
    return r.value, s.value


def _kvattn_heads(q, kv, B, nhead):
    """q [B, nhead, Tq, d] and k, v [B, nhead, Tk, d] of q [B Tq][C] and kv [B Tk][2 C], in their
    precision (fp32 at least)"""
    C = q.shape[1]
    up = (lambda t: t) if q.dtype == torch.float64 else (lambda t: t.float())
    x = up(kv).view(B, -1, 2, nhead, C // nhead).permute(2, 0, 3, 1, 4)
    return up(q).view(B, -1, nhead, C // nhead).permute(0, 2, 1, 3), x[0], x[1]


def kvattn_forward(q, kv, out, B, nhead, st: KVAttnState, bf16_products=False):
    """q [B Tq][C] (channel h d + j: component j of head h), kv [B Tk][2 C] (channel s C + h d + j,
    s = 0 for k and 1 for v), out [B Tq][C].  Per sample and head O = softmax(Q K^T / sqrt(d)) V with
    the softmax in fp32; st.lse receives every row's log-sum-exp.  out must alias neither input.
    bf16_products: as attn_forward."""
    (rows, C), Tk = q.shape, kv.shape[0] // B
    Tq = rows // B
    if B * nhead * Tq > st.lse.shape[0]:
        raise ValueError("kvattn_forward: batch %d, state sized for %d rows" % (B, st.lse.shape[0]))
    if out.data_ptr() in (q.data_ptr(), kv.data_ptr()):
        raise ValueError("kvattn_forward: out must not alias q or kv (backward reads them again)")
    if not _native_t(q):
        qh, k, v = _kvattn_heads(q, kv, B, nhead)
        s = qh @ k.transpose(-1, -2) / (C // nhead) ** 0.5
        lse = torch.logsumexp(s, -1, keepdim=True)
        st.lse[:B * nhead * Tq].copy_(lse.reshape(-1))
        p = torch.exp(s - lse)
        o = (_bf16_round(p) if bf16_products else p) @ v
        out.copy_(o.permute(0, 2, 1, 3).reshape(rows, C))
        return
    _flat_bf16(q, kv, out, who="kvattn_forward")
    native.check(_k().cxn_kvattn_fwd(q.data_ptr(), kv.data_ptr(), out.data_ptr(), st.lse.data_ptr(), B, Tq, Tk,
                                     C, nhead, _stream()), "kvattn_fwd")


def kvattn_backward(g, q, kv, dq, dkv, B, nhead, st: KVAttnState, prop_grad: bool, bf16_products=False):
    """g [B Tq][C] = dO.  With P = exp(S - lse) of the last forward, dP = dO V^T and
    D_i = sum_j P_ij dP_ij: dV = P^T dO, dS = P (dP - D), dQ = dS K / sqrt(d) into dq [B Tq][C], which
    may be q, and dK = dS^T Q / sqrt(d) with dV into dkv [B Tk][2 C], which may be kv.  Without
    prop_grad nothing is computed or written.  bf16_products: as attn_backward."""
    if not prop_grad:
        return
    (rows, C), Tk = q.shape, kv.shape[0] // B
    Tq = rows // B
    if not _native_t(g):
        qh, k, v = _kvattn_heads(q, kv, B, nhead)
        sc = 1.0 / (C // nhead) ** 0.5
        do = (g if g.dtype == torch.float64 else g.float()).view(B, Tq, nhead, C // nhead).permute(0, 2, 1, 3)
        p = torch.exp(qh @ k.transpose(-1, -2) * sc - st.lse[:B * nhead * Tq].view(B, nhead, Tq, 1).to(qh.dtype))
        dp = do @ v.transpose(-1, -2)
        ds = p * (dp - (p * dp).sum(-1, keepdim=True))
        if bf16_products:
            p, ds = _bf16_round(p), _bf16_round(ds)
        gq = ds @ k * sc
        gkv = torch.stack([ds.transpose(-1, -2) @ qh * sc, p.transpose(-1, -2) @ do])
        dq.copy_(gq.permute(0, 2, 1, 3).reshape(rows, C))
        dkv.copy_(gkv.permute(1, 3, 0, 2, 4).reshape(B * Tk, 2 * C))
        return
    _flat_bf16(g, q, kv, dq, dkv, who="kvattn_backward")
    native.check(_k().cxn_kvattn_bwd(q.data_ptr(), kv.data_ptr(), g.data_ptr(), dq.data_ptr(),
                                     dkv.data_ptr(), st.ws.data_ptr(), st.ws.numel(), B, Tq, Tk, C, nhead, _stream()),
                 "kvattn_bwd")


# ----------------------------------------------------------------------------- add (element-wise sum, fused relu)
class AddState:
    """The relu mask of an `add` layer with add_relu = 1, sized once for the layer's largest
    batch.  HIP path: ceil(n / 8) bytes, bit j of byte r = "element 8 r + j of the stored y is
    > 0" (csrc/kernels/add_kernels.hip).  Torch path (CPU, precision = fp32): n bools."""

    def __init__(self, max_numel, device, packed):
        self.packed = bool(packed)
        if self.packed:
            self.mask = torch.zeros((int(max_numel) + 7) // 8, dtype=torch.uint8, device=device)
        else:
            self.mask = torch.zeros(int(max_numel), dtype=torch.bool, device=device)


def _flat_bf16(*ts, who="add"):
    for t in ts:
        if not (t.is_contiguous() and t.dtype == torch.bfloat16):
            raise ValueError(who + ": contiguous bf16 tensors expected")


def add_forward(xs, y, relu: bool, st: AddState = None):
    """y = x0 + x1 (+ x2 + x3), fp32 accumulation in input order, then relu when `relu`, one
    rounding to y's dtype.  st (training forward with relu): receives the mask "stored y > 0".
    y must not alias an input."""
    n = y.numel()
    if not 2 <= len(xs) <= 4 or any(x.numel() != n for x in xs):
        raise ValueError("add: 2 to 4 inputs of the output's size expected")
    if not _native_t(y):
        acc = xs[0].float()
        for x in xs[1:]:
            acc = acc + x.float()
        if relu:
            acc = torch.where(acc > 0, acc, torch.zeros_like(acc))
        y.copy_(acc)
        if st is not None:
            torch.gt(y.reshape(-1), 0, out=st.mask[:n])
        return
    _flat_bf16(y, *xs)
    ptr = [x.data_ptr() for x in xs] + [None] * (4 - len(xs))
    native.check(_k().cxn_add_fwd(*ptr, len(xs), y.data_ptr(), st.mask.data_ptr() if st is not None else None, n,
                                  int(bool(relu)), _stream()), "add_fwd")


def add_backward(g, dsts, st: AddState = None):
    """Every dst = g where the forward's stored y was > 0 and exactly 0 elsewhere (st: the
    forward's mask); st None: every dst = g.  No dst may alias g."""
    n = g.numel()
    if not 1 <= len(dsts) <= 4 or any(d.numel() != n for d in dsts):
        raise ValueError("add: 1 to 4 destinations of the gradient's size expected")
    if not _native_t(g):
        v = g if st is None else torch.where(st.mask[:n].view(g.shape), g, torch.zeros_like(g))
        for d in dsts:
            d.copy_(v)
        return
    _flat_bf16(g, *dsts)
    ptr = [d.data_ptr() for d in dsts] + [None] * (4 - len(dsts))
    native.check(_k().cxn_add_bwd(g.data_ptr(), st.mask.data_ptr() if st is not None else None, *ptr, len(dsts), n,
                                  _stream()), "add_bwd")


# ----------------------------------------------------------------------------- ch_scale (per-sample channel gate)
def se_parts(B: int, HW: int, C: int) -> int:
    """Parts the ch_scale backward and the global pooling cut a map of HW pixels into
    (csrc/kernels/se_kernels.hip): a function of the shape alone.  1: no workspace, one launch."""
    n = int(_k().cxn_se_parts(int(B), int(HW), int(C)))
    if n < 1:
        raise ValueError("se_parts: bad shape (%d, %d, %d)" % (B, HW, C))
    return n


class ChScaleState:
    """The fp32 partial workspace [part][B C] of a `ch_scale` layer's backward, sized once for
    every batch up to max_batch (csrc/kernels/se_kernels.hip).  None on the torch path and where
    one block owns a whole (image, channel group)."""

    def __init__(self, max_batch, HW, C, device, native_path):
        self.ws = None
        if native_path:
            n = int(_k().cxn_se_ws_floats(int(max_batch), int(HW), int(C)))
            if n > 0:
                self.ws = torch.zeros(n, dtype=torch.float32, device=device)


def _ch_scale_dims(x, s):
    if x.dim() != 4 or s.numel() != x.shape[0] * x.shape[3]:
        raise ValueError("ch_scale: x [B][H][W][C] and a gate of B C elements expected")
    return x.shape[0], x.shape[1] * x.shape[2], x.shape[3]


def ch_scale_forward(x, s, y):
    """y[b,h,w,c] = x[b,h,w,c] s[b,c] in fp32, one rounding to y's dtype.  x, y NHWC; s any
    contiguous tensor of B C elements in [b][c] order.  y must not alias x or s."""
    B, HW, C = _ch_scale_dims(x, s)
    if not _native_t(x):
        y.copy_(x.float() * s.reshape(B, 1, 1, C).float())
        return
    _flat_bf16(x, s, y, who="ch_scale")
    native.check(_k().cxn_ch_scale_fwd(x.data_ptr(), s.data_ptr(), y.data_ptr(), B, HW, C, _stream()), "ch_scale_fwd")


def ch_scale_backward(g, x, s, dx, ds, st: ChScaleState = None):
    """dx = g s (one rounding) and ds[b,c] = sum over the map of g x, accumulated in fp32 in a
    fixed order and rounded once.  dx may alias x, ds may alias s; neither may alias g.
    st: the layer's workspace (HIP path, needed where se_parts(...) > 1)."""
    B, HW, C = _ch_scale_dims(x, s)
    if not _native_t(g):
        g32, s32 = g.float(), s.reshape(B, 1, 1, C).float()
        dsum = (g32 * x.float()).sum((1, 2))
        dx.copy_(g32 * s32)
        ds.copy_(dsum.reshape(ds.shape))
        return
    _flat_bf16(g, x, s, dx, ds, who="ch_scale")
    ws = st.ws if st is not None else None
    native.check(_k().cxn_ch_scale_bwd(g.data_ptr(), x.data_ptr(), s.data_ptr(), dx.data_ptr(), ds.data_ptr(),
                                       ws.data_ptr() if ws is not None else None,
                                       ws.numel() if ws is not None else 0, B, HW, C, _stream()), "ch_scale_bwd")


# ----------------------------------------------------------------------------- relu6 / hsigmoid / hswish
HACT_KINDS = ("relu6", "hsigmoid", "hswish")  # index = the kernels' kind (csrc/kernels/hact_kernels.hip)


def hact_pass_elems() -> int:
    """Elements one pass of the kernels' capped grid covers; a larger tensor makes a thread take a
    second grid-stride trip."""
    return int(_k().cxn_hact_pass_elems())


def _hact_kind(kind) -> int:
    if kind not in HACT_KINDS:
        raise ValueError("hact: kind must be one of %s, not %r" % (", ".join(HACT_KINDS), kind))
    return HACT_KINDS.index(kind)


def hact_forward(kind: str, x, y):
    """y = f(x) in fp32, one rounding to y's dtype; the breakpoints belong to the outer pieces:
    relu6     +0 for x <= 0, 6 for x >= 6, x (the same bits) between;
    hsigmoid  +0 for x <= -3, 1 for x >= 3, (x + 3) / 6 between;
    hswish    0 for x <= -3, x (the same bits) for x >= 3, x (x + 3) / 6 between.
    y must not alias x."""
    k = _hact_kind(kind)
    if x.numel() != y.numel():
        raise ValueError("hact: x and y of one size expected")
    if x.data_ptr() == y.data_ptr():
        raise ValueError("hact: y must not alias x (backward reads x again)")
    if not _native_t(x):
        v = x.float()
        zero = torch.zeros_like(v)
        if k == 0:
            out = torch.where(v <= 0, zero, torch.where(v >= 6, torch.full_like(v, 6.0), v))
        elif k == 1:
            out = torch.where(v <= -3, zero, torch.where(v >= 3, torch.ones_like(v), (v + 3.0) / 6.0))
        else:
            out = torch.where(v <= -3, zero, torch.where(v >= 3, v, v * (v + 3.0) / 6.0))
        y.copy_(out.view(y.shape))
        return
    _flat_bf16(x, y, who="hact")
    native.check(_k().cxn_hact_fwd(x.data_ptr(), y.data_ptr(), x.numel(), k, _stream()), "hact_fwd")


def hact_backward(kind: str, x, g, dx):
    """dx = g f'(x), the derivative taken from the layer's INPUT x, in fp32, one rounding:
    relu6     g (the same bits) for 0 < x < 6, 0 elsewhere;
    hsigmoid  g / 6 for -3 < x < 3, 0 elsewhere;
    hswish    0 for x <= -3, g (the same bits) for x >= 3, g (2 x + 3) / 6 between.
    dx may alias x; it must not alias g."""
    k = _hact_kind(kind)
    if not x.numel() == g.numel() == dx.numel():
        raise ValueError("hact: x, g and dx of one size expected")
    if dx.data_ptr() == g.data_ptr():
        raise ValueError("hact: dx must not alias g (it may alias x)")
    if not _native_t(g):
        v, gv = x.float(), g.float().view(x.shape)
        zero = torch.zeros_like(gv)
        if k == 0:
            out = torch.where((v > 0) & (v < 6), gv, zero)
        elif k == 1:
            out = torch.where((v > -3) & (v < 3), gv / 6.0, zero)
        else:
            out = torch.where(v <= -3, zero, torch.where(v >= 3, gv, gv * (2.0 * v + 3.0) / 6.0))
        dx.copy_(out.view(dx.shape))
        return
    _flat_bf16(x, g, dx, who="hact")
    native.check(_k().cxn_hact_bwd(x.data_ptr(), g.data_ptr(), dx.data_ptr(), x.numel(), k, _stream()), "hact_bwd")


# ----------------------------------------------------------------------------- silu
def silu_pass_elems() -> int:
    """Elements one pass of the silu kernels' capped grid covers; a larger tensor makes a thread take
    a second grid-stride trip."""
    return int(_k().cxn_silu_pass_elems())


def _sigma32(v):
    """1 / (1 + e^-x) in fp32, in the kernels' formulation: finite at both ends (e^-x = inf gives +0,
    e^-x = 0 gives 1 exactly)"""
    return 1.0 / (1.0 + torch.exp(-v))


def silu_forward(x, y):
    """y = x sigma(x), sigma(x) = 1 / (1 + e^-x), in fp32, one rounding to y's dtype.  Where sigma
    rounds to 1 (x >= 17 or so) y is x, the same bits; where e^-x overflows y is -0.
    y must not alias x."""
    if x.numel() != y.numel():
        raise ValueError("silu: x and y of one size expected")
    if x.data_ptr() == y.data_ptr():
        raise ValueError("silu: y must not alias x (backward reads x again)")
    if not _native_t(x):
        v = x.float()
        y.copy_((v * _sigma32(v)).view(y.shape))
        return
    _flat_bf16(x, y, who="silu")
    native.check(_k().cxn_silu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "silu_fwd")


def silu_backward(x, g, dx):
    """dx = g sigma(x) (1 + x (1 - sigma(x))), the derivative taken from the layer's INPUT x, in
    fp32, one rounding.  Where sigma rounds to 1 dx is g, the same bits; where e^-x overflows dx is
    a zero.  dx may alias x; it must not alias g."""
    if not x.numel() == g.numel() == dx.numel():
        raise ValueError("silu: x, g and dx of one size expected")
    if dx.data_ptr() == g.data_ptr():
        raise ValueError("silu: dx must not alias g (it may alias x)")
    if not _native_t(g):
        v, gv = x.float(), g.float().view(x.shape)
        s = _sigma32(v)
        dx.copy_((gv * s * (1.0 + v * (1.0 - s))).view(dx.shape))
        return
    _flat_bf16(x, g, dx, who="silu")
    native.check(_k().cxn_silu_bwd(x.data_ptr(), g.data_ptr(), dx.data_ptr(), x.numel(), _stream()), "silu_bwd")


# ----------------------------------------------------------------------------- gelu
def _cdf32(v):
    """Phi(x) = erfc(-x / sqrt 2) / 2 in fp32, the kernels' formulation: no cancellation on the
    left, +0 and 1 exactly at the ends"""
    return 0.5 * torch.erfc(v * -0.7071067811865476)


def gelu_forward(x, y):
    """y = x Phi(x) (the exact, erf form) in fp32, one rounding to y's dtype.  y must not alias x."""
    if x.numel() != y.numel():
        raise ValueError("gelu: x and y of one size expected")
    if x.data_ptr() == y.data_ptr():
        raise ValueError("gelu: y must not alias x (backward reads x again)")
    if not _native_t(x):
        v = x.float()
        y.copy_((v * _cdf32(v)).view(y.shape))
        return
    _flat_bf16(x, y, who="gelu")
    native.check(_k().cxn_gelu_fwd(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "gelu_fwd")


def gelu_backward(x, g, dx):
    """dx = g (Phi(x) + x phi(x)), phi(x) = e^(-x x / 2) / sqrt(2 pi), the derivative taken from the
    layer's INPUT x, in fp32, one rounding.  dx may alias x; it must not alias g."""
    if not x.numel() == g.numel() == dx.numel():
        raise ValueError("gelu: x, g and dx of one size expected")
    if dx.data_ptr() == g.data_ptr():
        raise ValueError("gelu: dx must not alias g (it may alias x)")
    if not _native_t(g):
        v, gv = x.float(), g.float().view(x.shape)
        pdf = 0.3989422804014327 * torch.exp(-0.5 * (v * v))
        dx.copy_((gv * (_cdf32(v) + v * pdf)).view(dx.shape))
        return
    _flat_bf16(x, g, dx, who="gelu")
    native.check(_k().cxn_gelu_bwd(x.data_ptr(), g.data_ptr(), dx.data_ptr(), x.numel(), _stream()), "gelu_bwd")


# ----------------------------------------------------------------------------- drop_path (per-sample dropout)
def drop_path_pass_elems() -> int:
    """Elements of one sample that a pass of the drop_path kernel's capped grid covers."""
    return int(_k().cxn_drop_path_pass_elems())


def drop_path_keep_ref(B: int, seed: int, pkeep: float, device="cpu") -> torch.Tensor:
    """The kernel's keep decisions as a bool tensor of B: hash_u32(b, seed) < dropout_thresh(pkeep)
    (csrc/kernels/nn_shared.h), seed the EFFECTIVE seed (ops.nn.effective_seed).  This is dropout's
    mask at element b, with the threshold taken from pkeep as the fp32 number the kernel receives."""
    p32 = float(torch.tensor(pkeep, dtype=torch.float32))
    t = min(int(p32 * 4294967296.0), 0xFFFFFFFF)
    return _hash_u32(torch.arange(B, dtype=torch.int64, device=device), seed & 0xFFFFFFFF) < t


def drop_path_apply(x, seed: int, pkeep: float, counter=None):
    """x[B][...] in place: sample b is kept or dropped as a whole (drop_path_keep_ref with the seed
    hash(counter, seed), read on the device, so a captured HIP graph draws a new mask on every
    replay).  A kept sample becomes x * (1.0f / pkeep), one fp32 product and one rounding to x's
    dtype; a dropped one becomes +0 whatever it held -- a selection, not x * 0.  Forward and backward
    use the same call."""
    if x.dim() < 1 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError("drop_path: a contiguous tensor [B][...] expected")
    if not 0.0 < pkeep <= 1.0:
        raise ValueError("drop_path: pkeep must be in (0, 1]")
    B = x.shape[0]
    n = x.numel() // B
    if not _native_t(x):
        keep = drop_path_keep_ref(B, effective_seed(seed, counter), pkeep, x.device)
        scale = torch.ones((), dtype=torch.float32, device=x.device) / torch.tensor(pkeep, dtype=torch.float32,
                                                                                  device=x.device)
        v = (x.reshape(B, n).float() * scale).to(x.dtype)
        x.copy_(torch.where(keep.view(B, 1), v, torch.zeros_like(v)).view(x.shape))
        return
    _flat_bf16(x, who="drop_path")
    native.check(_k().cxn_drop_path(x.data_ptr(), B, n, seed & 0xFFFFFFFF, _ctr(counter), float(pkeep), _stream()),
                 "drop_path")


# ----------------------------------------------------------------------------- prelu
def _prelu_mask_ref(x2d, slope, seed, counter, rnd):
    rows, C = x2d.shape
    m = slope.float().expand(rows, C)
    if rnd > 0:
        u = uniform_ref(rows * C, effective_seed(seed, counter), x2d.device).view(rows, C)
        m = m * (1 + u * rnd * 2.0 - rnd)
    return m.clamp(0, 1)


def prelu_forward(x2d, y2d, slope, seed, counter, rnd):
    """y = x > 0 ? x : x * clamp(slope * noise, 0, 1)   (reference prelu_layer-inl.hpp:111-135)."""
    rows, C = x2d.shape
    if not _native_t(x2d):
        x = x2d.float()
        y2d.copy_(torch.where(x > 0, x, x * _prelu_mask_ref(x2d, slope, seed, counter, rnd)))
        return
    native.check(_k().cxn_prelu(x2d.data_ptr(), None, y2d.data_ptr(), slope.data_ptr(), rows, C, seed & 0xFFFFFFFF,
                                _ctr(counter), float(rnd), 0, _stream()), "prelu_fwd")


def prelu_backward(x2d, g2d, dx2d, slope, gslope, seed, counter, rnd, prop_grad, ws=None):
    """gslope += sum min(x, 0) * g; dx = x > 0 ? g : g * mask  (reference :137-152).  dx may alias x."""
    rows, C = x2d.shape
    if not _native_t(x2d):
        x, g = x2d.float(), g2d.float()
        gslope.add_((torch.clamp(x, max=0) * g).sum(0))
        if prop_grad:
            dx2d.copy_(torch.where(x > 0, g, g * _prelu_mask_ref(x2d, slope, seed, counter, rnd)))
        return
    k = _k()
    if ws is None:
        ws = torch.empty(3 * C, dtype=torch.float32, device=x2d.device)
    native.check(k.cxn_chan_reduce(x2d.data_ptr(), g2d.data_ptr(), None, ws.data_ptr(), rows, C, 3, _stream()),
                 "prelu_slope_grad")
    gslope.add_(ws[:C])
    if prop_grad:
        native.check(k.cxn_prelu(x2d.data_ptr(), g2d.data_ptr(), dx2d.data_ptr(), slope.data_ptr(), rows, C,
                                 seed & 0xFFFFFFFF, _ctr(counter), float(rnd), 1, _stream()), "prelu_bwd")


# ----------------------------------------------------------------------------- insanity
def _insanity_div_ref(n, lb, ub, train, seed, counter, device):
    if not train:
        return torch.full((n,), 0.5 * (lb + ub), dtype=torch.float32, device=device)
    u = uniform_ref(n, effective_seed(seed, counter), device)
    return lb + u * (ub - lb)


def insanity_forward(x, y, y2, lb, ub, train, seed, counter):
    """y (and y2) = x > 0 ? x : x / U[lb, ub)  (test: / ((lb + ub) / 2))."""
    if not _native_t(x):
        d = _insanity_div_ref(x.numel(), lb, ub, train, seed, counter, x.device).view_as(x)
        xf = x.float()
        out = torch.where(xf > 0, xf, xf / d)
        y.copy_(out)
        if y2 is not None:
            y2.copy_(out)
        return
    native.check(_k().cxn_insanity(x.data_ptr(), None, y.data_ptr(), y2.data_ptr() if y2 is not None else None,
                                   x.numel(), float(lb), float(ub), int(train), seed & 0xFFFFFFFF, _ctr(counter), 0,
                                   _stream()), "insanity_fwd")


def insanity_backward(y, g, dx, lb, ub, train, seed, counter):
    """dx = y > 0 ? g : g / d with forward's draws (dx may alias y)."""
    if not _native_t(y):
        d = _insanity_div_ref(y.numel(), lb, ub, train, seed, counter, y.device).view_as(y)
        yf, gf = y.float(), g.float()
        dx.copy_(torch.where(yf > 0, gf, gf / d))
        return
    native.check(_k().cxn_insanity(y.data_ptr(), g.data_ptr(), dx.data_ptr(), None, y.numel(), float(lb), float(ub),
                                   int(train), seed & 0xFFFFFFFF, _ctr(counter), 1, _stream()), "insanity_bwd")


# ----------------------------------------------------------------------------- insanity pooling
def _shift_ref(N, H, W, C, keep, seed, counter, device):
    """Flat NHWC source index each input element is read from."""
    u = uniform_ref(N * H * W * C, effective_seed(seed, counter), device).view(N, H, W, C)
    d = (1.0 - keep) / 4.0
    yy = torch.arange(H, device=device).view(1, H, 1, 1).expand(N, H, W, C)
    xx = torch.arange(W, device=device).view(1, 1, W, 1).expand(N, H, W, C)
    ly = torch.where((u >= keep) & (u < keep + d), (yy - 1).clamp_min(0), yy)
    ly = torch.where((u >= keep + d) & (u < keep + 2 * d), (yy + 1).clamp_max(H - 1), ly)
    lx = torch.where((u >= keep + 2 * d) & (u < keep + 3 * d), (xx - 1).clamp_min(0), xx)
    lx = torch.where(u >= keep + 3 * d, (xx + 1).clamp_max(W - 1), lx)
    n = torch.arange(N, device=device).view(N, 1, 1, 1)
    c = torch.arange(C, device=device).view(1, 1, 1, C)
    return ((n * H + ly) * W + lx) * C + c


def ins_pool_forward(x, y, ysave, K, S, keep, seed, counter):
    N, H, W, C = x.shape
    Ho, Wo = y.shape[1], y.shape[2]
    if not _native_t(x):
        src = x.reshape(-1)[_shift_ref(N, H, W, C, keep, seed, counter, x.device)].float()  # shifted image
        out = torch.full((N, Ho, Wo, C), float("-inf"), device=x.device)
        for py in range(Ho):
            for px in range(Wo):
                win = src[:, py * S:min(py * S + K, H), px * S:min(px * S + K, W), :]
                out[:, py, px, :] = win.amax(dim=(1, 2))
        y.copy_(out)
        if ysave is not None:
            ysave.copy_(out)
        return
    native.check(_k().cxn_ins_pool_fwd(x.data_ptr(), y.data_ptr(), ysave.data_ptr() if ysave is not None else None,
                                       N, H, W, C, Ho, Wo, K, S, float(keep), seed & 0xFFFFFFFF, _ctr(counter),
                                       _stream()), "ins_pool_fwd")


def ins_pool_backward(x, ypool, gy, dx, K, S, keep, seed, counter):
    """dx must not alias x."""
    N, H, W, C = x.shape
    Ho, Wo = gy.shape[1], gy.shape[2]
    if not _native_t(x):
        vsrc = x.reshape(-1)[_shift_ref(N, H, W, C, keep, seed, counter, x.device)].float()
        out = torch.zeros(N, H, W, C, device=x.device)
        yp, g = ypool.float(), gy.float()
        for py in range(Ho):
            for px in range(Wo):
                y0, y1, x0, x1 = py * S, min(py * S + K, H), px * S, min(px * S + K, W)
                hit = (vsrc[:, y0:y1, x0:x1, :] == yp[:, py:py + 1, px:px + 1, :]).float()
                out[:, y0:y1, x0:x1, :] += hit * g[:, py:py + 1, px:px + 1, :]
        dx.copy_(out)
        return
    native.check(_k().cxn_ins_pool_bwd(x.data_ptr(), ypool.data_ptr(), gy.data_ptr(), dx.data_ptr(), N, H, W, C, Ho,
                                       Wo, K, S, float(keep), seed & 0xFFFFFFFF, _ctr(counter), _stream()),
                 "ins_pool_bwd")
