"""Float64 references and derived per-element error bounds for the kernels of the layer
`batch_norm` (and `bias`), prelu, insanity, insanity_max_pooling (csrc/kernels/layer_kernels.hip),
the activations and dropout (csrc/kernels/act_kernels.hip) and the fused optimizer step
(csrc/kernels/optim_kernels.hip), in the style of tests/bounds.py and tests/bn_bounds.py: the
operands are the exact bf16 / fp32 values the kernel reads, the reference is float64 on the CPU and
written out here (it never calls the package's host path of the same op; only the package's counter
hash is used, which defines the generator, not the operation), and every bound comes from the
arithmetic -- none is tuned to what a kernel gives.

  u = 2^-23   charged per fp32 operation (round to nearest errs by u / 2; u leaves room for fused
              and unfused forms and for a reciprocal-based division)
  U = 2^-8    bf16 unit roundoff of a stored output
  g(K) = (K + 2) u   K fp32 additions in any order, against the sum of the absolute terms
  FLOOR = 2^-126     a result below the smallest normal fp32 number may be flushed to 0

A bf16 output whose fp32 value is within `fp` of the reference has the bound
      store(ref, fp) = fp + U (|ref| + fp).
Hyper-parameters (eps, rnd, lb, ub, keep, b, pkeep, lr, wd, mom, clip, d1, d2) are taken as the
fp32 numbers the kernel is handed.

batch_norm (two-pass: mean = (sum x) (1 / R); var = (sum (x - mean)^2) (1 / R) against the stored
fp32 mean; inv = 1 / sqrt(var + eps)).  bn_bounds.stats_ref's bounds hold for this scheme: the sum
of x is R additions and two more roundings (1 / R and the product), inside g(R) sum|x| / R; the
centred squares against the stored mean m' give exactly var + (m' - mean)^2 <= var + e_mean^2,
and their roundings (the subtraction, the square, R additions, the scale: R + 4 half-units) are
inside g(R) var.  Forward y = ((x - m') inv') slope + bias is bn_bounds.forward_ref's.
  x-hat = bf16((x - m') inv'), written over the input node in training:
      fp = |x - mean| e_inv + inv e_mean + 2 u |(x - mean) inv|       (the subtraction, the product)
  backward dx = g A + (x - m') B + Cc is bn_bounds.backward_ref's, plus what bn_bwd_coeffs takes
  and bn_bounds does not count:
      B is formed as ve = 1 / (iv iv); gvar = sl s2 (-0.5) iv / ve; B = gvar (1 / R) 2: seven
        rounded operations (iv iv, the reciprocal, sl s2, . iv, / ve, 1 / R, . (1 / R)) where the
        4 u |B| term charges four: + 3 u |B| |x - mean|
      the first part of Cc, -sl s1 iv (1 / R), is five (sl s1, . iv, the sum with the second part,
        1 / R, . (1 / R)) against the four of 4 u |Cc|: + u |Cc|
      the second part of Cc is gvar (1 / R) (-2 s0) (1 / R) = -B s0 / R with s0 = sum (x - m'),
        zero in exact arithmetic and as computed bounded by
            e_s0 = R e_mean + g(R) (sum|x - mean| + R e_mean)
        (sum (x - m') = R (mean - m') exactly; each difference is rounded and the R of them are
        added in fp32): + |B| e_s0 / R (1 + 8 u)
  affine_forward with given fp32 mean / inv / slope / bias, y = ((x - mean) inv) slope + bias:
      fp = 3 u |(x - mean) inv slope| + u |ref|     (subtract, two products; the add)

prelu.  m = clamp(slope (1 + u01 rnd 2 - rnd), 0, 1) with the draw u01 at flat index r C + c;
y = x > 0 ? x : x m (backward: g in place of x, decided by x).  rnd = 0: m = clamp(slope), exact.
Otherwise four rounded operations (u01 rnd, 1 + ., . - rnd, slope .) on intermediates no larger
than 1 + 2 rnd, and the clamp is 1-Lipschitz:  e_m = 4 u |slope| (1 + 2 rnd).
      x > 0: exact (bound 0);  else fp = |v| (e_m + u m),  v = x or g
  gslope = gslope0 + sum_r min(x, 0) g: the products are exact (two bf16 factors), R additions in
  any order, and the op adds the kernel's sum onto gslope in a second step -- one more rounding
  than bounds.dbias_ref:  (R + 3) u (sum|min(x, 0) g| + |gslope0|).

insanity.  d = lb + u01 (ub - lb) in training (three rounded operations on values no larger than
D = max(|lb|, |ub|, |ub - lb|): e_d = 3 u D), d = 0.5 (lb + ub) at test time (e_d = u |d|);
y = x > 0 ? x : x / d:  fp = |x / d| (e_d / |d| + u) + FLOOR.  Backward: g in place of x, decided
by the sign of the stored y.

insanity_max_pooling.  Element (n, y, x, c) is read from a neighbour chosen by its own draw
u01 (flat NHWC index): u01 < keep stays, [keep, keep + d) y - 1, [.., keep + 2 d) y + 1,
[.., keep + 3 d) x - 1, else x + 1, clamped at the border, d = (1 - keep) / 4 -- the thresholds
are the fp32 values keep + d, keep + 2 d, keep + 3 d, and INS_POOL_GAP is asserted: no draw lies
within 4 u of a threshold, so that a fused or unfused threshold decides alike.  Windows are
[py S, min(py S + K, H)) x [px S, min(px S + K, W)), py < Ho = ins_pool_out(H, K, S).  Forward:
the max of the shifted values, exact.  Backward: dx of an element = the sum of gy over the covering
windows whose stored max equals the element's shifted value (every tie takes the gradient): an
fp32 sum of T <= ceil(K / S)^2 exact bf16 terms, fp = g(T) sum|terms|; 0 terms: exactly 0.

activations (kind relu / sigmoid / tanh / xelu(b)).
  relu     max(x, 0): exact
  xelu     x > 0 ? x : x / b:    fp = u |ref| + FLOOR
  sigmoid  1 / (1 + __expf(-x)), __expf(t) = exp2(t log2 e).  As in bounds._softmax_parts the
           exponential e = exp(-x) has the relative error delta = (2 + 2 |x|) u (two roundings of
           an exponent of size |x| log2 e, each |x| u in the result; one unit for exp2, one
           spare); s = 1 / (1 + e) has ds / s = (1 - s) de / e, and the add and the divide are
           two more operations:   fp = s ((1 - s) delta + 2 u) + FLOOR
           (where e overflows, s is 0 and the reference is below 2^-128: inside FLOOR)
  tanh     tanhf, assumed accurate to ULP_TANH = 4 units of 2^-23 (no document is at hand that
           states the device library's figure; next to U = 2^-8 a generous one costs nothing):
           fp = ULP_TANH u |ref| + FLOOR
  backward from the stored bf16 y:  dx = dy f'(y);  relu dy (y > 0), exact; sigmoid dy (y (1 - y)),
  three operations; tanh dy (1 - y y), y y exact, two; xelu y > 0 ? dy : dy (1 / b), two:
           fp = n_ops u |ref| + FLOOR

dropout.  Element i is kept iff hash(i, seed) < min(int(pkeep 2^32), 2^32 - 1) (pkeep the fp32
number); a kept element is bf16(x float32(1 / pkeep)): fp = u |ref|; a dropped one is exactly 0.

fused_update: see update_ref.
"""
import math

import numpy as np
import torch

import bn_bounds as BN
from bounds import U_BF16, EPS_F32, assert_within, violations, _as_f32  # noqa: F401  (re-exported)
from cxxnet_amd.ops.layer_ops import uniform_ref
from cxxnet_amd.ops.nn import _hash_u32, effective_seed

U32 = EPS_F32
FLOOR = 2.0 ** -126
ULP_TANH = 4
# condition of the insanity-pooling reference, asserted where the shifts are computed
INS_POOL_GAP = 4 * U32
# condition of the Adam bound, asserted in update_ref: the second moment after the step stays above
# this floor and its own error below half of it, so that |sqrt(m2 + e) - sqrt(m2)| <= e / sqrt(m2)
ADAM_M2_MIN = 1e-6


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def g(K):
    return (K + 2) * U32


def store(ref, fp):
    """bound of a bf16 output whose fp32 value is within fp of ref"""
    return fp + U_BF16 * (ref.abs() + fp)


def draws(n, seed, counter=None):
    """float64 [n] of the exact fp32 draws u01(i, hash(counter, seed)) of the kernels"""
    return uniform_ref(n, effective_seed(seed, counter)).double()


# ------------------------------------------------------------------------------------ batch_norm
def bn_forward_ref(x, slope, bias, eps):
    """dict of the training forward of layer batch_norm: mean / inv (ref, bound), y, xhat."""
    eps = _as_f32(eps)
    y, y_b, s = BN.forward_ref(x, slope, bias, eps)
    d, inv, e_inv, e_mean = s["d"], s["inv"], s["e_inv"], s["e_mean"]
    xh = d * inv
    xh_b = store(xh, d.abs() * e_inv + inv * e_mean + 2 * U32 * xh.abs())
    return {"mean": (s["mean"], e_mean), "inv": (inv, e_inv), "y": (y, y_b), "xhat": (xh, xh_b), "stats": s}


def bn_backward_ref(gy, x, slope, gslope0, gbias0, eps):
    """bn_bounds.backward_ref plus the roundings of bn_bwd_coeffs it does not count (see above)."""
    eps = _as_f32(eps)
    out = BN.backward_ref(gy, x, slope, gslope0, gbias0, eps)
    s = BN.stats_ref(x)
    R, d, e_mean = s["R"], s["d"], s["e_mean"]
    inv, _ = BN.inv_ref(s["var"], s["e_var"], eps)
    g64, sl = _f64(gy), _f64(slope)
    A = sl * inv
    B = -A * inv * inv * (g64 * d).sum(0) / R
    Cc = -A * g64.sum(0) / R
    e_s0 = R * e_mean + g(R) * (d.abs().sum(0) + R * e_mean)
    extra = 3 * U32 * B.abs() * d.abs() + U32 * Cc.abs() + B.abs() * e_s0 / R * (1 + 8 * U32)
    dx, dx_b = out["dx"]
    out["dx"] = (dx, dx_b + extra)
    return out


def affine_ref(x, mean, inv, slope, bias):
    """(ref, bound) of y = ((x - mean) inv) slope + bias from the given fp32 vectors."""
    x, mean, inv, slope, bias = _f64(x), _f64(mean), _f64(inv), _f64(slope), _f64(bias)
    t = (x - mean) * inv * slope
    ref = t + bias
    return ref, store(ref, 3 * U32 * t.abs() + U32 * ref.abs())


# ------------------------------------------------------------------------------------ prelu
def prelu_mask_ref(rows, C, slope, rnd, seed, counter=None, u=None):
    """(m, e_m) float64 [rows][C]; u: the draws to use instead of the generator's (tests)."""
    sl = _f64(slope).expand(rows, C)
    rnd = _as_f32(rnd)
    if not rnd > 0:
        return sl.clamp(0, 1), torch.zeros(rows, C, dtype=torch.float64)
    if u is None:
        u = draws(rows * C, seed, counter).view(rows, C)
    m = (sl * (1 + u * rnd * 2 - rnd)).clamp(0, 1)
    return m, 4 * U32 * sl.abs() * (1 + 2 * rnd)


def prelu_ref(x, v, slope, rnd, seed, counter=None, u=None):
    """(ref, bound) of out = x > 0 ? v : v m (forward: v = x; backward: v = g)."""
    x64, v64 = _f64(x), _f64(v)
    m, e_m = prelu_mask_ref(x.shape[0], x.shape[1], slope, rnd, seed, counter, u)
    pos = x64 > 0
    ref = torch.where(pos, v64, v64 * m)
    fp = torch.where(pos, torch.zeros_like(ref), v64.abs() * (e_m + U32 * m))
    return ref, torch.where(pos, torch.zeros_like(ref), store(ref, fp))


def prelu_gslope_ref(x, gy, gslope0):
    t = _f64(x).clamp_max(0) * _f64(gy)
    i = _f64(gslope0)
    return i + t.sum(0), (x.shape[0] + 3) * U32 * (t.abs().sum(0) + i.abs())


# ------------------------------------------------------------------------------------ insanity
def insanity_div_ref(n, lb, ub, train, seed, counter=None, u=None):
    lb, ub = _as_f32(lb), _as_f32(ub)
    if not train:
        d = torch.full((n,), 0.5 * (lb + ub), dtype=torch.float64)
        return d, U32 * d.abs()
    if u is None:
        u = draws(n, seed, counter)
    d = lb + u * (ub - lb)
    return d, torch.full_like(d, 3 * U32 * max(abs(lb), abs(ub), abs(ub - lb)))


def insanity_ref(sel, v, lb, ub, train, seed, counter=None, u=None):
    """(ref, bound) of out = sel > 0 ? v : v / d, flat.  Forward: sel = v = x; backward: sel = the
    stored y, v = g."""
    s64, v64 = _f64(sel).reshape(-1), _f64(v).reshape(-1)
    d, e_d = insanity_div_ref(v64.numel(), lb, ub, train, seed, counter, u)
    assert float((d.abs() - e_d).min()) > 0
    pos = s64 > 0
    q = v64 / d
    ref = torch.where(pos, v64, q)
    fp = q.abs() * (e_d / d.abs() + U32) + FLOOR
    return ref, torch.where(pos, torch.zeros_like(ref), store(ref, fp))


# ------------------------------------------------------------------------------------ insanity pooling
def ins_pool_out(H, K, S):
    """Windows along an axis: the ceil rule min(H - K + S - 1, H - 1) // S + 1, and one clipped
    window where the map is smaller than the kernel (the rule alone gives none there)."""
    return max(min(H - K + S - 1, H - 1) // S + 1, 1)


def ins_pool_shifted(x, keep, seed, counter=None, clamp=True):
    """float64 [N][H][W][C]: the value each element is read from, written out per element.
    clamp=False: the defect of an unclamped shift (wraps to the neighbouring row / image)."""
    N, H, W, C = x.shape
    x64 = _f64(x).reshape(-1)
    u = draws(N * H * W * C, seed, counter).numpy()
    k = np.float32(_as_f32(keep))
    d = np.float32((np.float32(1) - k) * np.float32(0.25))
    t1 = np.float32(k + d)
    t2 = np.float32(k + np.float32(np.float32(2) * d))
    t3 = np.float32(k + np.float32(np.float32(3) * d))
    if float(d) > 0:  # (d = 0: the intervals are empty whichever way they are rounded)
        for t in (k, t1, t2, t3):
            assert np.abs(u - float(t)).min() > INS_POOL_GAP, "a draw lies within 4 u of the threshold %r" % t
    out = torch.empty(N * H * W * C, dtype=torch.float64)
    i = 0
    for n in range(N):
        for y in range(H):
            for xx in range(W):
                for c in range(C):
                    ly, lx, v = y, xx, u[i]
                    if v < k:
                        pass
                    elif v < t1:
                        ly = y - 1 if (y > 0 or not clamp) else y
                    elif v < t2:
                        ly = y + 1 if (y + 1 < H or not clamp) else H - 1
                    elif v < t3:
                        lx = xx - 1 if (xx > 0 or not clamp) else xx
                    else:
                        lx = xx + 1 if (xx + 1 < W or not clamp) else W - 1
                    out[i] = x64[(((n * H + ly) * W + lx) * C + c) % x64.numel()]
                    i += 1
    return out.view(N, H, W, C)


def ins_pool_forward_ref(shifted, K, S):
    """float64 [N][Ho][Wo][C]: the max of the shifted values over each clipped window. Exact."""
    N, H, W, C = shifted.shape
    Ho, Wo = ins_pool_out(H, K, S), ins_pool_out(W, K, S)
    out = torch.empty(N, Ho, Wo, C, dtype=torch.float64)
    for py in range(Ho):
        for px in range(Wo):
            win = shifted[:, py * S:min(py * S + K, H), px * S:min(px * S + K, W), :]
            assert win.shape[1] > 0 and win.shape[2] > 0
            out[:, py, px, :] = win.amax(dim=(1, 2))
    return out + 0.0


def ins_pool_backward_ref(shifted, ymax, gy, K, S):
    """(ref, bound) of dx [N][H][W][C] from the stored max ymax and gy."""
    N, H, W, C = shifted.shape
    y64, g64 = _f64(ymax), _f64(gy)
    Ho, Wo = y64.shape[1], y64.shape[2]
    ref = torch.zeros(N, H, W, C, dtype=torch.float64)
    A = torch.zeros_like(ref)
    T = torch.zeros_like(ref)
    for py in range(Ho):
        for px in range(Wo):
            y0, y1, x0, x1 = py * S, min(py * S + K, H), px * S, min(px * S + K, W)
            hit = (shifted[:, y0:y1, x0:x1, :] == y64[:, py:py + 1, px:px + 1, :]).double()
            gg = g64[:, py:py + 1, px:px + 1, :]
            ref[:, y0:y1, x0:x1, :] += hit * gg
            A[:, y0:y1, x0:x1, :] += hit * gg.abs()
            T[:, y0:y1, x0:x1, :] += hit
    assert float(T.max()) <= math.ceil(K / S) ** 2
    return ref, torch.where(T > 0, store(ref, (T + 2) * U32 * A), torch.zeros_like(ref))


# ------------------------------------------------------------------------------------ activations
ACT_KINDS = ["relu", "sigmoid", "tanh", "xelu"]


def act_forward_ref(kind, x, b=5.0):
    x64 = _f64(x)
    b = _as_f32(b)
    zero = torch.zeros_like(x64)
    if kind == "relu":
        return x64.clamp_min(0), zero
    if kind == "xelu":
        ref = torch.where(x64 > 0, x64, x64 / b)
        return ref, torch.where(x64 > 0, zero, store(ref, U32 * ref.abs() + FLOOR))
    if kind == "sigmoid":
        ref = torch.sigmoid(x64)
        delta = (2 + 2 * x64.abs()) * U32
        return ref, store(ref, ref * ((1 - ref) * delta + 2 * U32) + FLOOR)
    ref = torch.tanh(x64)
    return ref, store(ref, ULP_TANH * U32 * ref.abs() + FLOOR)


def act_backward_ref(kind, y, dy, b=5.0):
    """from the stored bf16 y"""
    y64, d64 = _f64(y), _f64(dy)
    b = _as_f32(b)
    if kind == "relu":
        ref = torch.where(y64 > 0, d64, torch.zeros_like(d64))
        return ref, torch.zeros_like(ref)
    if kind == "sigmoid":
        ref, nops = d64 * (y64 * (1 - y64)), 3
    elif kind == "tanh":
        ref, nops = d64 * (1 - y64 * y64), 2
    else:
        ref, nops = torch.where(y64 > 0, d64, d64 / b), 2
    return ref, store(ref, nops * U32 * ref.abs() + FLOOR)


# ------------------------------------------------------------------------------------ dropout
def dropout_keep_ref(n, pkeep, seed, counter=None, shift=0):
    """bool [n], the exact keep set.  shift: the defect of a mask shifted by that many elements."""
    t = min(int(_as_f32(pkeep) * 4294967296.0), 0xFFFFFFFF)
    idx = torch.arange(n, dtype=torch.int64) + shift
    return _hash_u32(idx, effective_seed(seed, counter)) < t


def dropout_ref(x, pkeep, seed, counter=None):
    """(ref, bound, keep), flat"""
    x64 = _f64(x).reshape(-1)
    keep = dropout_keep_ref(x64.numel(), pkeep, seed, counter)
    scale = float(np.float32(1) / np.float32(pkeep))
    ref = torch.where(keep, x64 * scale, torch.zeros_like(x64))
    return ref, torch.where(keep, store(ref, U32 * ref.abs()), torch.zeros_like(ref)), keep


# ------------------------------------------------------------------------------------ fused_update
def update_ref(algo, w, gr, m1, m2, segs, d1=0.1, d2=0.001):
    """One optimizer step over the segments (offset, n, lr, wd, mom, clip) of the flat fp32 state
    before the step.  Returns a dict of float64 arrays of the whole arena: w, m1, m2 (the values
    after the step; outside every segment the values before it) with the bounds e_w, e_m1, e_m2,
    e_wb (bf16 shadow, reference w) -- all 0 outside the segments -- and `inside` (bool).

    sgd   gc = clip(g) (only here; clip = 0: none; NaN -> 0 under a non-zero clip, +-inf -> +-clip;
          exact).  m' = mom m - lr (gc + wd w), w' = w + m': bounds.sgd_step_ref's bound with the
          gradient given exactly (eg = 0):
              S = mom |m| + lr (|gc| + wd |w|)      e_m1 = 3 u S  (five roundings of u / 2)
              e_w = e_m1 + u (|w'| + e_m1)           e_wb = e_w + U (|w'| + e_w)
    nag   m' as sgd without the clip: e_m1 = 3 u S.  w' = w + (1 + mom) m' - mom m: five more
          roundings of u / 2 (1 + mom, its product, the sum, mom m, the difference) of
          intermediates no larger than T = |w| + (1 + mom) (|m'| + e_m1) + mom |m|:
              e_w = (1 + mom) e_m1 + 3 u T
    adam  g' = g - wd w only when wd > 0 (two operations: e_g = u (|g| + wd |w|), else 0)
          m1' = m1 + d1 (g' - m1)    three operations of intermediates <= M1 = |m1| + d1 (|g'| + e_g + |m1|):
              e_m1 = d1 e_g + 2 u M1
          m2' = m2 + d2 (g'^2 - m2)  four, with q2 = g'^2 + 2 |g'| e_g + e_g^2, M2 = |m2| + d2 (q2 + |m2|):
              e_m2 = d2 (2 |g'| e_g + e_g^2) + 3 u M2
          s = sqrt(m2') + 1e-8 (the fp32 number).  Condition (asserted): m2' >= ADAM_M2_MIN and
          e_m2 <= m2' / 2, under which |sqrt(m2' + e) - sqrt(m2')| <= e / sqrt(m2'):
              e_s = e_m2 / sqrt(m2') + u s           (the square root, the add)
          q = m1' / s:  e_q = (e_m1 + |q| e_s) / (s - e_s) + u |q|
          w' = w - lr q:  e_w = lr e_q + u lr (|q| + e_q) + u (|w'| + lr e_q)
    e_wb = e_w + U (|w'| + e_w) for all three."""
    w0, g0, a0 = _f64(w).clone(), _f64(gr), _f64(m1).clone()
    b0 = _f64(m2).clone() if m2 is not None else None
    out = {"w": w0.clone(), "m1": a0.clone(), "m2": b0.clone() if b0 is not None else None}
    for k in ("e_w", "e_m1", "e_m2", "e_wb"):
        out[k] = torch.zeros_like(w0)
    inside = torch.zeros(w0.numel(), dtype=torch.bool)
    d1, d2 = _as_f32(d1), _as_f32(d2)
    for off, n, lr, wd, mom, clip in segs:
        lr, wd, mom, clip = _as_f32(lr), _as_f32(wd), _as_f32(mom), _as_f32(clip)
        sl = slice(off, off + n)
        assert not inside[sl].any(), "overlapping segments"
        inside[sl] = True
        wv, gv, mv = w0[sl], g0[sl], a0[sl]
        if algo == "sgd" and clip != 0.0:
            gv = torch.where(torch.isnan(gv), torch.zeros_like(gv), gv).clamp(-clip, clip)
        if algo in ("sgd", "nag"):
            mn = mom * mv - lr * (gv + wd * wv)
            S = abs(mom) * mv.abs() + abs(lr) * (gv.abs() + abs(wd) * wv.abs())
            em = 3 * U32 * S
            if algo == "sgd":
                wn = wv + mn
                ew = em + U32 * (wn.abs() + em)
            else:
                wn = wv + (1 + mom) * mn - mom * mv
                T = wv.abs() + (1 + mom) * (mn.abs() + em) + abs(mom) * mv.abs()
                ew = (1 + mom) * em + 3 * U32 * T
        else:
            m2v = b0[sl]
            if wd > 0:
                gp, eg = gv - wd * wv, U32 * (gv.abs() + wd * wv.abs())
            else:
                gp, eg = gv, torch.zeros_like(gv)
            mn = mv + d1 * (gp - mv)
            em = d1 * eg + 2 * U32 * (mv.abs() + d1 * (gp.abs() + eg + mv.abs()))
            q2 = gp * gp + 2 * gp.abs() * eg + eg * eg
            m2n = m2v + d2 * (gp * gp - m2v)
            em2 = d2 * (2 * gp.abs() * eg + eg * eg) + 3 * U32 * (m2v.abs() + d2 * (q2 + m2v.abs()))
            if n:
                assert float(m2n.min()) >= ADAM_M2_MIN and bool((em2 <= m2n / 2).all()), "Adam bound condition broken"
            eps8 = _as_f32(1e-8)
            s = m2n.sqrt() + eps8
            es = em2 / m2n.sqrt() + U32 * s
            q = mn / s
            eq = (em + q.abs() * es) / (s - es) + U32 * q.abs()
            wn = wv - lr * q
            ew = abs(lr) * eq + U32 * abs(lr) * (q.abs() + eq) + U32 * (wn.abs() + abs(lr) * eq)
            out["m2"][sl], out["e_m2"][sl] = m2n, em2
        out["w"][sl], out["m1"][sl] = wn, mn
        out["e_w"][sl], out["e_m1"][sl] = ew, em
        out["e_wb"][sl] = ew + U_BF16 * (wn.abs() + ew)
    out["inside"] = inside
    return out
