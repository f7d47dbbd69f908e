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
bounds are derived in sgd_step_ref.  The cross-channel LRN (alone and fused behind the 3 x 3 / 2
max pooling), the row softmax and the loss gradient have theirs derived in _lrn_parts,
lrn_backward_ref, pool_lrn_backward_ref, _softmax_parts and loss_grad_ref.

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


# ------------------------------------------------------------------ LRN, fused pool -> LRN, softmax
# Assumed accuracy of the hardware transcendentals v_log_f32 / v_exp_f32, in ulps (of 2^-23
# relative): no ISA document is at hand that states it, so 2 ulp each is taken (the vendor's
# published figure for both is 1 ulp; the factor 2 costs nothing, see LRN_E_MAX).
ULP_LOG2 = 2
ULP_EXP2 = 2
# Condition of the LRN bounds, asserted wherever they are computed: the relative fp32 error e of
# norm^-beta stays below 2^-14, at least 64 times under u = 2^-8, so the generous constants in e
# cost the bound no power (it is u |ref| to within 2 %).
LRN_E_MAX = 2.0 ** -14
LN2 = 0.6931471805599453


def _lrn_window(v, h):
    """sum over channels c-h .. c+h, clipped to [0, C), of v[..., c]"""
    C = v.shape[-1]
    p = F.pad(v, (h, h))
    out = torch.zeros_like(v)
    for i in range(2 * h + 1):
        out = out + p[..., i:i + C]
    return out


def _lrn_parts(x, n, alpha, beta, k):
    """(x64, h, salpha, beta, norm, p = norm^-beta, e) of the cross-channel LRN
        norm[c] = k + salpha sum_{c' in [c-h, c+h] clipped to [0, C)} x[c']^2,  h = n // 2,
    with salpha = float32(alpha) / n as the launchers compute it (an fp32 quotient) and beta, k the
    fp32 numbers the kernel is handed.  The window is the kernels' (2 h + 1 channels: for an even
    local size one more than n, divided by n all the same).

    e bounds the relative fp32 error of norm^-beta computed as exp2(-beta log2(norm)):
      (n + 2) 2^-23 beta   x^2 is exact (bf16 squared has 16 significand bits); the window sum is
               2 h <= n additions, the scale by salpha and the add of k two more roundings, all of
               positive terms, so norm is off by at most (n + 2) roundings relative to itself
               (2^-23 each, twice round-to-nearest's 2^-24, as gamma() above), and norm^-beta by
               beta times that;
      ln2 M beta (ULP_LOG2 + 1) 2^-23,  M = max(1, |log2 norm|)   the exponent t = -beta L,
               L = log2(norm): L is off by ULP_LOG2 ulps -- of M, not of |L|: next to norm = 1
               the log's error is bounded absolutely -- and the multiply by beta rounds once; an
               absolute error dt of the exponent is a relative error ln2 dt of 2^t;
      (ULP_EXP2 + 1) 2^-23   the exp2 itself, and the multiply by x (forward) or dy (backward)
               that follows it."""
    x64 = _f64(x)
    h = int(n) // 2
    sa = float(torch.tensor(alpha, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))
    beta, k = _as_f32(beta), _as_f32(k)
    norm = k + sa * _lrn_window(x64 * x64, h)
    assert float(norm.min()) > 0
    M = norm.log2().abs().clamp_min(1.0)
    e = EPS_F32 * (beta * (n + 2) + LN2 * M * beta * (ULP_LOG2 + 1) + ULP_EXP2 + 1)
    assert float(e.max()) <= LRN_E_MAX, "LRN bound condition e <= 2^-14 broken: %g" % float(e.max())
    return x64, h, sa, beta, norm, norm.pow(-beta), e


def lrn_rel_err(x, n, alpha, beta, k):
    """The largest e (see _lrn_parts) over the input: the tests assert it <= LRN_E_MAX."""
    return float(_lrn_parts(x, n, alpha, beta, k)[6].max())


def lrn_forward_ref(x, n, alpha, beta, k):
    """(ref, bound), float64 of x's shape (channels last), of y = x norm^-beta stored as bf16:
        bound = u |ref| (1 + e) + e |ref|
    the fp32 value is within e |ref| of ref (e of _lrn_parts) and the store rounds it by u."""
    x64, _, _, _, _, p, e = _lrn_parts(x, n, alpha, beta, k)
    ref = x64 * p
    return ref, U_BF16 * ref.abs() * (1 + e) + e * ref.abs()


def lrn_backward_ref(x, dy, n, alpha, beta, k, mask_relu=False):
    """(ref, bound) of the LRN data gradient stored as bf16,
        ref = dy p - 2 beta salpha x sum_{c' in win(c)} dy x p / norm,   p = norm^-beta,
        A   = |dy| p + 2 beta salpha |x| sum_win |dy x| p / norm   (both terms in absolute value)
        bound = u (|ref| + g A) + g A,   g = e + (n + 3) 2^-23.
    e covers p in both terms.  In the second, dy x is exact (two bf16 factors), the factor 1 / norm
    is exp2(-L) of the same L (or the exponent (-beta - 1) L in one piece), and the remaining
    roundings are two multiplies per window term, 2 h <= n additions of the second window sum,
    three multiplies by 2 beta salpha x and the subtraction: n + 6 roundings of 2^-24, which
    (n + 3) 2^-23 holds.  1 / norm's own error (norm's roundings unscaled by beta, the shared log)
    is paid from the doubled units: e charges 2^-23 where round-to-nearest gives 2^-24 and 2 ulp
    where the transcendentals are published at 1, which covers it for beta >= 1/2; the emulation
    in test_norm_bounds_cpu.py (fp32, the kernels' order of operations) peaks below the bound.
    mask_relu: x is a relu output and the gradient is also multiplied by (x > 0): ref and bound
    are 0 where x <= 0 -- such an element must be exactly 0."""
    x64, h, sa, beta, norm, p, e = _lrn_parts(x, n, alpha, beta, k)
    d64 = _f64(dy)
    c2 = 2.0 * beta * sa
    ref = d64 * p - c2 * x64 * _lrn_window(d64 * x64 * p / norm, h)
    A = d64.abs() * p + c2 * x64.abs() * _lrn_window((d64 * x64).abs() * p / norm, h)
    gA = (e + (n + 3) * EPS_F32) * A
    bound = U_BF16 * (ref.abs() + gA) + gA
    if mask_relu:
        live = (x64 > 0).to(torch.float64)
        ref, bound = ref * live, bound * live
    return ref, bound


def pool3s2_out(H):
    """output size of the 3 x 3 / stride 2 ceil-mode max pooling (windows clipped at the far edge)"""
    return min(H - 2, H - 1) // 2 + 1


def pool3s2_first_max(x, relu_flags):
    """(P, state) of the 3 x 3 / 2 ceil-mode max pooling of x [N][H][W][C], taken explicitly: the
    nine taps in kh * 3 + kw order, a later tap replacing the maximum only when strictly greater
    (the first maximum wins a tie; -0.0 == 0.0 is a tie), taps past the far edge left out, relu
    on the way in when relu_flags & 1.  P float64 [N][Ho][Wo][C]; state uint8, the tap chosen, with
    bit 7 set where relu_flags & 2 and the pooled maximum is not > 0."""
    x64 = _f64(x)
    if relu_flags & 1:
        x64 = x64.clamp_min(0)
    N, H, W, C = x64.shape
    Ho, Wo = pool3s2_out(H), pool3s2_out(W)
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    arg = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    for kh in range(3):
        for kw in range(3):
            t = x64[:, kh::2, kw::2][:, :Ho, :Wo]  # rows 2 ho + kh < H, columns 2 wo + kw < W
            nh, nw = t.shape[1], t.shape[2]
            take = t > best[:, :nh, :nw]
            best[:, :nh, :nw] = torch.where(take, t, best[:, :nh, :nw])
            arg[:, :nh, :nw] = torch.where(take, torch.full_like(arg[:, :nh, :nw], kh * 3 + kw), arg[:, :nh, :nw])
    if relu_flags & 2:
        arg = arg | (~(best > 0)).to(torch.uint8) * 128
    return best + 0.0, arg  # (+ 0.0: a maximum of -0.0 compares equal either way)


def _route(v, tap, hw):
    """sum of the window values v [N][Ho][Wo][C] at the input pixel each window's tap names"""
    N, Ho, Wo, C = v.shape
    out = torch.zeros((N, hw[0], hw[1], C), dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            o = out[:, kh::2, kw::2][:, :Ho, :Wo]
            nh, nw = o.shape[1], o.shape[2]
            o += torch.where(tap[:, :nh, :nw] == kh * 3 + kw, v[:, :nh, :nw], torch.zeros_like(v[:, :nh, :nw]))
    return out


def pool_lrn_backward_ref(x, dY, n, alpha, beta, k, relu_flags, relu_bit=True, dbias_init=None):
    """Backward of max-pool (3 x 3 / 2, ceil mode) -> LRN: a dict with
      P, state    pool3s2_first_max(x, relu_flags): what the forward must store, exactly;
      gp, b_gp    lrn_backward_ref(P, dY): the pooled gradient and its bound (it is rounded to
                  bf16 before it is routed, as the separate layers store it), zeroed where the
                  window's bit 7 is set (relu_flags & 2, pooled max <= 0) and relu_bit applies;
      dx, dx_bound  dx = the sum of the gp routed to each input pixel by the first-max tap (at
                  most four windows cover a pixel: an fp32 sum of <= 4 terms, then the bf16 store)
                    bound = sum of the routed b_gp + u (|dx| + that) + 4 2^-23 sum |gp routed|
                  -- 0 at a pixel no window chose, which must then be exactly 0;
      dbias, dbias_bound  (with dbias_init) init + the column sums of gp over R = N Ho Wo windows
                    bound = sum of b_gp over the column + (R + 2) 2^-23 (sum |gp| + |init|);
                  it grows like R u: R <= 100 is asserted, so that one missing window term (of
                  typical size sum |gp| / R, against R u / 2 of it from the rounding of gp) still
                  exceeds it."""
    P, state = pool3s2_first_max(x, relu_flags)
    gp, b_gp = lrn_backward_ref(P, dY, n, alpha, beta, k)
    if relu_bit and relu_flags & 2:
        live = (state < 128).to(torch.float64)
        gp, b_gp = gp * live, b_gp * live
    tap = state & 127
    hw = x.shape[1:3]
    dx, routed_b, routed_a = _route(gp, tap, hw), _route(b_gp, tap, hw), _route(gp.abs(), tap, hw)
    out = dict(P=P, state=state, gp=gp, b_gp=b_gp, dx=dx,
               dx_bound=routed_b + U_BF16 * (dx.abs() + routed_b) + 4 * EPS_F32 * routed_a)
    if dbias_init is not None:
        C = gp.shape[-1]
        R = gp.numel() // C
        assert R <= 100, "dbias bound is only meaningful up to R = 100 windows: %d" % R
        i = _f64(torch.as_tensor(dbias_init)).expand(C)
        g2 = gp.reshape(-1, C)
        out["dbias"] = i + g2.sum(0)
        out["dbias_bound"] = b_gp.reshape(-1, C).sum(0) + (R + 2) * EPS_F32 * (g2.abs().sum(0) + i.abs())
    return out


def _softmax_parts(x):
    """(p, bound32, bound16, sum_bound) of the row softmax of x [rows][K]: p float64; bound32 for
    the fp32 copy, bound16 for the bf16 one; sum_bound [rows] for |sum_k p32 - 1|.
    The kernels compute e_k = __expf(x_k - m) = exp2((x_k - m) log2 e), s = sum e_k, p = e_k / s:
      delta_k = (2 + 2 |x_k - m|) 2^-23   relative error of e_k: the subtraction is exact or one
               rounding, the product with log2 e (itself rounded) another: two roundings of an
               exponent of size |x_k - m| log2 e, each an absolute ln2 |x_k - m| log2 e 2^-23 =
               |x_k - m| 2^-23 in the result's relative error; plus one ulp for exp2 and one spare;
      D = sum_k p_k delta_k   relative error of s from its terms' errors;
      (K + 4) 2^-23   K additions in any order (lanes, then a shuffle tree), the reciprocal and
               the final multiply;
      bound32 = p_k (delta_k + D + (K + 4) 2^-23) + 2^-126   (the floor: a result below the
               smallest normal may be flushed to 0)
      bound16 = u (p + bound32) + bound32
      sum_bound = (K + 4) 2^-23 + D   (the p32 sum to 1 as well as s was summed; the test's own
               float64 sum adds nothing)."""
    x64 = _f64(x)
    K = x64.shape[1]
    m = x64.max(1, keepdim=True).values
    p = torch.softmax(x64, dim=1)
    delta = (2 + 2 * (x64 - m).abs()) * EPS_F32
    D = (p * delta).sum(1, keepdim=True)
    b32 = p * (delta + D + (K + 4) * EPS_F32) + 2.0 ** -126
    b16 = U_BF16 * (p + b32) + b32
    return p, b32, b16, ((K + 4) * EPS_F32 + D).reshape(-1)


def softmax_ref(x):
    """(p, bound32, bound16) of _softmax_parts"""
    return _softmax_parts(x)[:3]


def softmax_sum_bound(x):
    """[rows] bound of |sum_k p32[r][k] - 1| (sum_bound of _softmax_parts)"""
    return _softmax_parts(x)[3]


def loss_grad_ref(p32, label, scale, kind="softmax"):
    """(ref, bound) of the loss gradient written as bf16 over the node: (p - target) float32(scale),
    target = onehot(label[:, 0]) for "softmax", label [rows][K] otherwise; p32 the predictions the
    kernel read (its own fp32 softmax, or the bf16 node).  The subtraction, the multiply (and
    float32(scale) being taken exactly) are fp32 roundings, then the bf16 store:
        bound = u |ref| + 3 2^-23 |ref| + 2^-133   (2^-133: the smallest bf16 denormal)."""
    p = _f64(p32)
    lab = _f64(label)
    if kind == "softmax":
        tgt = torch.zeros_like(p)
        tgt.scatter_(1, lab[:, :1].long(), 1.0)
    else:
        tgt = lab
    ref = (p - tgt) * _as_f32(scale)
    return ref, U_BF16 * ref.abs() + 3 * EPS_F32 * ref.abs() + 2.0 ** -133


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
