"""Float64 references and derived per-element error bounds for the convolution and GEMM kernels.

A whole-tensor norm ratio cannot see a localized defect (one border pixel, the last image of an
odd batch, one channel fragment): bf16 output rounding alone puts it at ~1.7e-3, and a dropped
tap at one pixel of one image moves it by less than that.  The bounds here are per element and
derived from the arithmetic, not tuned to what a kernel gives:

  u   = 2^-8   bf16 unit roundoff of the stored output: 8 significand bits, so round to nearest
               moves a value by at most half an ulp = 2^-8 |v| (2^-9 is violated by a correct
               fp32 computation)
  g   = (K + 2) 2^-23   K fp32 additions in any order have the worst-case relative error
               (K - 1) 2^-24 against sum |terms|; doubled because the MFMA's internal rounding is
               unspecified (truncation: unit roundoff 2^-23); + 2 for the bias add
  forward / data gradient (bf16 out):  bound = u (|ref| + g A) + g A,  A = conv(|x|, |w|) + |b|
  bias-gradient sum (fp32):            bound = (R + 2) 2^-23 (sum |dx| + |init|),  R = N H W
  weight gradient (fp32, onto dw0):    bound = (K + 2) 2^-23 A,  A = |dw0| + conv_weight(|x|, |dy|),
                                       K = N Ho Wo
The fully-connected GEMMs take the same forms with K = nin (forward), nout (data gradient; its
alpha multiply is one more rounding: K + 3) and the batch (weight gradient); the fused SGD step's
bounds are derived in sgd_step_ref.

The operands are the exact bf16 values (bf16 x bf16 products are exact in float64, and float64
summation error is ~1e-13 relative: nothing next to 2^-23).  Everything runs on the CPU.
Tensors are NHWC activations and [Cout][KH][KW][Cg] weights, as the kernels take them.
"""
import torch
import torch.nn.functional as F

U_BF16 = 2.0 ** -8
EPS_F32 = 2.0 ** -23


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def _nchw(t):
    return _f64(t).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def gamma(K):
    return (K + 2) * EPS_F32


def _bf16_bound(ref, A, K):
    gA = gamma(K) * A
    return U_BF16 * (ref.abs() + gA) + gA


def forward_ref(x, w, b=None, *, stride=1, pad=0, groups=1, relu=False):
    """(ref, bound), NHWC float64, of y = [relu](conv(x, w) + b) stored as bf16.  pad: one number
    or (pad_y, pad_x); the kernel [Cout][KH][KW][Cg] need not be square."""
    xn, wn = _nchw(x), _nchw(w)
    bb = _f64(b) if b is not None else None
    pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
    ref = F.conv2d(xn, wn, bb, stride=stride, padding=pad, groups=groups)
    A = F.conv2d(xn.abs(), wn.abs(), bb.abs() if bb is not None else None, stride=stride, padding=pad, groups=groups)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    bound = _bf16_bound(ref, A, K)  # (of the value before the relu, which is 1-Lipschitz)
    if relu:
        ref = ref.clamp_min(0)
    return _nhwc(ref), _nhwc(bound)


def data_grad_ref(dy, w, *, stride=1, pad=0, groups=1, mask=None, in_hw=None, add=None):
    """(ref, bound), NHWC float64, of the data gradient dx = conv_transpose(dy, w) stored as bf16
    (stride: the forward stride; pad one number or (pad_y, pad_x)); with mask (bool NHWC, relu'(z)
    of the node written) ref and bound are zero where the mask is: a masked element must be
    exactly 0.  add (NHWC, dx's shape): a second gradient summed in before the store and the
    mask, dx = mask(conv_transpose(dy, w) + add).  in_hw = (H, W) of dx: with a stride several input sizes give dy's size, and the
    output_padding of the transposed convolution is what the geometry implies,
    H - ((Ho - 1) stride - 2 pad_y + KH) (0 without it, which is always right at stride 1)."""
    dn, wn = _nchw(dy), _nchw(w)
    py, px = (pad, pad) if isinstance(pad, int) else pad
    op = (0, 0)
    if in_hw is not None:
        op = tuple(full - ((o - 1) * stride - 2 * p + k) for full, o, p, k in
                   zip(in_hw, dy.shape[1:3], (py, px), w.shape[1:3]))
        assert all(0 <= v < max(stride, 2) for v in op), (in_hw, op)
    kw = dict(stride=stride, padding=(py, px), output_padding=op, groups=groups)
    ref = _nhwc(F.conv_transpose2d(dn, wn, **kw))
    A = _nhwc(F.conv_transpose2d(dn.abs(), wn.abs(), **kw))
    K = w.shape[1] * w.shape[2] * (w.shape[0] // groups)
    if add is not None:  # a second gradient summed in fp32 before the store: one more term
        ref, A, K = ref + _f64(add), A + _f64(add).abs(), K + 1
    bound = _bf16_bound(ref, A, K)
    if mask is not None:
        m = mask.detach().to("cpu", torch.float64)
        ref, bound = ref * m, bound * m
    return ref, bound


def dbias_ref(dx_stored, init):
    """(ref, bound) of dbias = init + the column sums of the stored dx (fp32 sums of R = N H W
    terms per column, in any order, plus the add onto init)."""
    d = _f64(dx_stored).reshape(-1, dx_stored.shape[-1])
    i = _f64(torch.as_tensor(init)).expand(d.shape[1])
    return i + d.sum(0), (d.shape[0] + 2) * EPS_F32 * (d.abs().sum(0) + i.abs())


def weight_grad_ref(x, dy, dw0, *, stride=1, pad=0, groups=1):
    """(ref, bound), [Cout][KH][KW][Cg] float64, of dw = dw0 + sum over pixels of dy (x) x in
    fp32.  The bound grows with K = N Ho Wo: meaningful (one missing pixel term still exceeds
    it) up to K ~ 1500."""
    xn, dn = _nchw(x), _nchw(dy)
    shape = (dw0.shape[0], dw0.shape[3], dw0.shape[1], dw0.shape[2])
    d0 = _f64(dw0)
    pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
    ref = d0 + _nhwc(torch.nn.grad.conv2d_weight(xn, shape, dn, stride=stride, padding=pad, groups=groups))
    A = d0.abs() + _nhwc(torch.nn.grad.conv2d_weight(xn.abs(), shape, dn.abs(), stride=stride, padding=pad, groups=groups))
    K = dy.shape[0] * dy.shape[1] * dy.shape[2]
    return ref, gamma(K) * A


def fc_forward_ref(x, w, b=None, relu=False):
    """(ref, bound), [B][nout] float64, of y = [relu](x . w^T + b) stored as bf16; x [B][nin],
    w [nout][nin]: the forward bound with K = nin."""
    x64, w64 = _f64(x), _f64(w)
    bb = _f64(b) if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    ref = x64 @ w64.t() + bb
    A = x64.abs() @ w64.abs().t() + bb.abs()
    bound = _bf16_bound(ref, A, x.shape[1])  # (of the value before the relu, which is 1-Lipschitz)
    return (ref.clamp_min(0) if relu else ref), bound


def fc_data_grad_ref(dy, w, alpha=1.0, mask=None):
    """(ref, bound), [B][nin] float64, of dx = alpha dy . w stored as bf16 (dy [B][nout],
    w [nout][nin]): K = nout, and the multiply by alpha (an fp32 number) is one more rounding,
    so g = (K + 3) 2^-23.  mask as in data_grad_ref."""
    d64, w64 = _f64(dy), _f64(w)
    a = float(torch.tensor(alpha, dtype=torch.float32))
    ref = a * (d64 @ w64)
    A = abs(a) * (d64.abs() @ w64.abs())
    bound = _bf16_bound(ref, A, dy.shape[1] + 1)
    if mask is not None:
        m = mask.detach().to("cpu", torch.float64)
        ref, bound = ref * m, bound * m
    return ref, bound


def fc_weight_grad_ref(x, dy, dw0=None):
    """(ref, bound), [nout][nin] float64, of dw = [dw0 +] dy^T . x in fp32 (the store and the +=
    epilogues): K = the batch, bound = (K + 2) 2^-23 (|dw0| + |dy|^T . |x|)."""
    x64, d64 = _f64(x), _f64(dy)
    ref, A = d64.t() @ x64, d64.abs().t() @ x64.abs()
    if dw0 is not None:
        ref, A = ref + _f64(dw0), A + _f64(dw0).abs()
    return ref, gamma(x.shape[0]) * A


def _as_f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def sgd_step_ref(x, dy, w, m, lr, wd, mom):
    """The fc weight gradient fused with the SGD step (EPI_F32_SGD): g = dy^T . x,
    m' = mom m - lr (g + wd w), w' = w + m', wb = bf16(w').  Returns
    ((m', bound), (w', bound), (wb, bound)), [nout][nin] float64; w, m are the fp32 state before
    the step, lr / wd / mom are taken as the fp32 numbers the kernel is handed.

    The computed gradient is g^ with |g^ - g| <= eg = (K + 2) 2^-23 Ag, Ag = |dy|^T . |x|, K the
    batch (the weight-gradient bound).  m' takes at most five fp32 roundings (wd w, + g, lr ..,
    mom m, the subtraction; fewer where they are fused), each of at most 2^-24 of an intermediate
    no larger than S = mom |m| + lr (|g| + eg + wd |w|), and the gradient's error enters scaled by
    lr:
        em  = lr eg + 3 2^-23 S              (3 2^-23 = 6 2^-24 >= 5 2^-24 (1 + 2^-24)^4)
    w' = w + m' is one more rounding of a value within em of the reference:
        ew  = em + 2^-23 (|w'| + em)
    and the shadow is its bf16 rounding, u = 2^-8:
        ewb = ew + u (|w'| + ew)"""
    x64, d64, w64, m64 = _f64(x), _f64(dy), _f64(w), _f64(m)
    lr, wd, mom = _as_f32(lr), _as_f32(wd), _as_f32(mom)
    g, Ag = d64.t() @ x64, d64.abs().t() @ x64.abs()
    eg = gamma(x.shape[0]) * Ag
    m1 = mom * m64 - lr * (g + wd * w64)
    S = abs(mom) * m64.abs() + abs(lr) * (g.abs() + eg + abs(wd) * w64.abs())
    em = abs(lr) * eg + 3 * EPS_F32 * S
    w1 = w64 + m1
    ew = em + EPS_F32 * (w1.abs() + em)
    ewb = ew + U_BF16 * (w1.abs() + ew)
    return (m1, em), (w1, ew), (w1, ewb)


def violations(got, ref, bound):
    """(count, worst d / bound, flat indices of the violations by decreasing excess).  An element
    violates when not |got - ref| <= bound (so a NaN does); where bound is 0 (a masked element)
    any difference is an infinite excess."""
    d = (_f64(got) - ref).abs()
    ratio = d / bound
    ratio = torch.where(bound > 0, ratio, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    ratio = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), ratio)
    bad = torch.nonzero(~(d <= bound).reshape(-1)).reshape(-1)
    worst = ratio.max().item() if ratio.numel() else 0.0
    if bad.numel():
        bad = bad[torch.argsort(ratio.reshape(-1)[bad], descending=True)]
    return int(bad.numel()), worst, bad


def assert_within(got, ref, bound, what="", axes="nhwc", show=8):
    """Assert |got - ref| <= bound for every element; returns the worst d / bound.  A failure
    names the number of violations, the worst excess and the coordinates of the worst few, so
    that the place of the damage (edge, last image, channel block) can be read off it."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(bound.shape), (got.shape, ref.shape, bound.shape)
    n, worst, bad = violations(got, ref, bound)
    if n:
        g64 = _f64(got)
        lines = []
        for flat in bad[:show].tolist():
            idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
            lines.append("  (%s)=%s got %.6g ref %.6g bound %.3g" % (", ".join(axes[:len(idx)]), idx, g64[idx].item(),
                                                                     ref[idx].item(), bound[idx].item()))
        spans = []
        allidx = torch.unravel_index(bad, ref.shape)
        for name, ix in zip(axes, allidx):
            spans.append("%s %d..%d" % (name, ix.min().item(), ix.max().item()))
        raise AssertionError("%s: %d of %d elements outside the bound, worst d/bound %.3g, within %s (shape %s)\n%s" % (
            what or "output", n, ref.numel(), worst, ", ".join(spans), tuple(ref.shape), "\n".join(lines)))
    return worst
