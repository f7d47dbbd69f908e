"""Ops of the less common layers: batch_norm, prelu, insanity, insanity_max_pooling, and of the
extensions batch_norm_ma, group_norm, add, ch_scale, relu6 / hsigmoid / hswish, silu, drop_path.

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
