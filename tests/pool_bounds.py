"""Float64 references, derived per-element bounds and the shared case table of the pooling kernels
(csrc/kernels/pool_kernels.hip behind cxn_pool_fwd, cxn_pool_bwd and cxn_pool_bwd_tie_all).

The references are written out as loops over the KH * KW taps with slicing, the way
bounds.pool3s2_first_max and bounds._route are for 3 x 3 / 2; they share no code with the
project's CPU executor path (ops._pool_ref, the unpool loops of ops.pool_backward), so the two can
be checked against each other (test_pool_bounds_cpu.py).  Operands are the exact bf16 values,
everything is float64 on the CPU, tensors are NHWC.

Geometry.  Window ho of an axis covers the input rows ho S - P .. ho S - P + K - 1, clipped to
[0, H); the number of windows is the reference's ceil rule min(Hp - K + S - 1, Hp - 1) // S + 1,
Hp = H + 2 P (out_size).  With a pad that rule can give a last window that lies wholly in the
padding (H = 5, K = 2, S = 2, P = 1: window 3 starts at row 5): has_empty_window.  No case of the
table has one (asserted when the table is built) and the pooling layer refuses such a geometry.

Max forward (max_forward_ref) has no bound: y is one of the bf16 inputs (or 0 behind a relu) and
the state is an integer; both must be exact.

The bounds take the form of tests/bounds.py,
    bound = u (|ref| + g A) + g A,   u = 2^-8 (the bf16 store),   g = r 2^-23,
A the same operation on the absolute values, r a count of fp32 roundings, each charged 2^-23:
twice round-to-nearest's 2^-24, the doubled unit of bounds.gamma, which also holds every
second-order term ((1 + 2^-24)^r - 1 <= r 2^-23 for r < 2^22).  The store rounds an fp32 value v
with |v - ref| <= g A: |bf16(v) - ref| <= u |v| + |v - ref| <= u (|ref| + g A) + g A.

  forward sum    K terms (the taps inside the map) are added in K - 1 roundings at most (the first
                 add, onto 0, is exact), in any order: r = K - 1, that is g = (K + c) 2^-23 with
                 c = C_SUM = -1.  A window of one tap must be reproduced to the bf16 rounding.
  forward avg    the sum, then one multiply by the fp32 constant fl(1 / (KH KW)): the constant is
                 off by one rounding from the quotient the reference divides by, the product
                 rounds once more: r = K + 1, c = C_AVG = +1.  The divisor is KH KW even where the
                 window is clipped: the reference's rule (pooling_layer-inl.hpp divides the
                 clipped sum by ksize_y ksize_x), so an edge average is smaller than the mean of
                 the taps it holds.
  backward max   (first): dx = the sum of the dy routed to the pixel by state & 127.  At most
                 T = ceil(KH / S) ceil(KW / S) windows cover one pixel, so at most T - 1 roundings;
                 g = (T + 2) 2^-23 = bounds.gamma(T), the form of the conv data gradient (whose
                 + 2, there the bias add, is room here).  A = the routed |dy|.  Where no window
                 chose the pixel A = 0 and dx = 0, so the bound is 0: exactly 0 is required; so it
                 is where the relu masks (relu = 1: x <= 0).  relu = 2: a window whose bit 7 is
                 set routes nothing.
  backward sum   the same with every covering window routed: g = (T + 2) 2^-23.
  backward avg   each term is dy fl(1 / (KH KW)): two more roundings per term (the constant's and
                 the product's), relative to the term, so 2 2^-23 A in all: g = (T + 4) 2^-23.
  tie_all        every input equal to its window's saved maximum y receives that window's dy; the
                 max-backward form, g = (T + 2) 2^-23.  With relu the maximum was taken over
                 relu(x) and the result is masked by x > 0.
  folded dbias   pool_bwd<8> sums what it stored, so the reference is
                 bounds.dbias_ref(dx stored by the kernel, init), R = N H W terms per column.  Like
                 weight_grad_ref's, that bound keeps its power up to about 1500 terms:
                 R <= DBIAS_R_MAX is asserted for the dbias cases.

None of the constants comes from a kernel's observed error.  Everything runs on the CPU.
"""
import functools
from collections import namedtuple

import torch

from bounds import EPS_F32, U_BF16, assert_within, dbias_ref, violations  # noqa: F401

C_SUM = -1
C_AVG = 1
DBIAS_R_MAX = 1500
MODES = ("max", "sum", "avg")


def _f64(t):
    return t.detach().to("cpu", torch.float64)


# ------------------------------------------------------------------------------------- geometry
def out_size(H, K, S, P=0):
    """number of windows along an axis: the reference's ceil rule"""
    Hp = H + 2 * P
    return min(Hp - K + S - 1, Hp - 1) // S + 1


def has_empty_window(H, K, S, P):
    """whether a window of the axis lies wholly in the padding: the first one (P >= K), or the last
    one the ceil rule gives (it starts at or past row H)"""
    return P >= K or (out_size(H, K, S, P) - 1) * S - P >= H


def windows_over_a_pixel(KH, KW, S):
    """T: the largest number of windows that cover one input pixel"""
    return -(-KH // S) * -(-KW // S)


def _axis(H, Ho, k, S, P):
    """(slice of the outputs, slice of the inputs) that tap k of an axis pairs up: output o reads
    input o S - P + k where that is inside [0, H); None when no output does"""
    lo = max(0, -(-(P - k) // S))
    hi = min(Ho - 1, (H - 1 + P - k) // S) if H - 1 + P - k >= 0 else -1
    if hi < lo:
        return None
    i0 = lo * S - P + k
    return slice(lo, hi + 1), slice(i0, i0 + (hi - lo) * S + 1, S)


def _taps(x_shape, KH, KW, S, P):
    """((kh, kw, output slices, input slices), ...) in kh * KW + kw order, taps that no window has
    inside the map left out; and (Ho, Wo)"""
    _, H, W, _ = x_shape
    Ho, Wo = out_size(H, KH, S, P), out_size(W, KW, S, P)
    out = []
    for kh in range(KH):
        ah = _axis(H, Ho, kh, S, P)
        for kw in range(KW):
            aw = _axis(W, Wo, kw, S, P)
            if ah is not None and aw is not None:
                out.append((kh, kw, (slice(None), ah[0], aw[0]), (slice(None), ah[1], aw[1])))
    return out, (Ho, Wo)


def tap_count(x_shape, KH, KW, S, P):
    """K [1][Ho][Wo][1]: the number of taps of each window that lie inside the map"""
    taps, (Ho, Wo) = _taps(x_shape, KH, KW, S, P)
    K = torch.zeros((1, Ho, Wo, 1), dtype=torch.float64)
    for _, _, so, _ in taps:
        K[so] += 1
    return K


# ------------------------------------------------------------------------------------- forward
def max_forward_ref(x, KH, KW, S, P, relu_flags=0):
    """(y, state) of the max pooling of x [N][H][W][C], taken explicitly: the taps in kh * KW + kw
    order, a later tap replacing the maximum only when strictly greater (the first maximum wins a
    tie; -0.0 == 0.0 is a tie), taps outside [0, H) x [0, W) left out, relu on the way in when
    relu_flags & 1.  y float64 [N][Ho][Wo][C] (compare with ==, so that signed zeros agree); state
    uint8, the tap chosen, with bit 7 set where relu_flags & 2 and the maximum is not > 0.  (A
    window with no tap inside the map would give -inf and tap 0: has_empty_window.)"""
    x64 = _f64(x)
    if relu_flags & 1:
        x64 = x64.clamp_min(0)
    taps, (Ho, Wo) = _taps(x64.shape, KH, KW, S, P)
    N, _, _, C = x64.shape
    best = torch.full((N, Ho, Wo, C), float("-inf"), dtype=torch.float64)
    arg = torch.zeros((N, Ho, Wo, C), dtype=torch.uint8)
    for kh, kw, so, si in taps:
        t = x64[si]
        take = t > best[so]
        best[so] = torch.where(take, t, best[so])
        arg[so] = torch.where(take, torch.full_like(arg[so], kh * KW + kw), arg[so])
    if relu_flags & 2:
        arg = arg | (~(best > 0)).to(torch.uint8) * 128
    return best + 0.0, arg


def _gamma_fwd(K, mode):
    return (K + (C_AVG if mode == "avg" else C_SUM)) * EPS_F32


def sum_forward_ref(x, KH, KW, S, P, mode, relu_flags=0):
    """(ref, bound), float64 [N][Ho][Wo][C], of the sum or avg pooling stored as bf16: the module
    docstring's forward sum / forward avg.  avg divides by KH KW, clipped window or not."""
    assert mode in ("sum", "avg")
    x64 = _f64(x)
    if relu_flags & 1:
        x64 = x64.clamp_min(0)
    taps, (Ho, Wo) = _taps(x64.shape, KH, KW, S, P)
    N, _, _, C = x64.shape
    ref = torch.zeros((N, Ho, Wo, C), dtype=torch.float64)
    A = torch.zeros_like(ref)
    for _, _, so, si in taps:
        ref[so] += x64[si]
        A[so] += x64[si].abs()
    if mode == "avg":
        ref, A = ref / (KH * KW), A / (KH * KW)
    gA = _gamma_fwd(tap_count(x64.shape, KH, KW, S, P), mode) * A
    return ref, U_BF16 * (ref.abs() + gA) + gA


# ------------------------------------------------------------------------------------- backward
def _bwd_bound(dx, A, r):
    gA = r * EPS_F32 * A
    return U_BF16 * (dx.abs() + gA) + gA


def max_backward_ref(x, state, dy, KH, KW, S, P, relu=0):
    """(dx, bound), float64 of x's shape, of the max-unpool to the recorded first maximum: the
    module docstring's backward max.  relu 1: times (x > 0); relu 2: a window whose bit 7 is set
    routes nothing (bit 7 only has a meaning there: a state that carries it is refused otherwise)."""
    st = state.detach().cpu()
    assert relu == 2 or not bool((st & 128).any()), "bit 7 in the state with relu != 2"
    d64 = _f64(dy)
    if relu == 2:
        d64 = d64 * (st < 128).to(torch.float64)
    tap = st & 127
    taps, _ = _taps(x.shape, KH, KW, S, P)
    dx = torch.zeros(tuple(x.shape), dtype=torch.float64)
    A = torch.zeros_like(dx)
    for kh, kw, so, si in taps:
        v = torch.where(tap[so] == kh * KW + kw, d64[so], torch.zeros_like(d64[so]))
        dx[si] += v
        A[si] += v.abs()
    bound = _bwd_bound(dx, A, windows_over_a_pixel(KH, KW, S) + 2)
    if relu == 1:
        live = (_f64(x) > 0).to(torch.float64)
        dx, bound = dx * live, bound * live
    return dx, bound


def sum_backward_ref(x, dy, KH, KW, S, P, mode, relu=0):
    """(dx, bound) of the sum or avg unpool: every window that covers a pixel hands it its dy
    (avg: dy / (KH KW)): the module docstring's backward sum / backward avg.  relu 1: times
    (x > 0)."""
    assert mode in ("sum", "avg")
    d64 = _f64(dy)
    if mode == "avg":
        d64 = d64 / (KH * KW)
    taps, _ = _taps(x.shape, KH, KW, S, P)
    dx = torch.zeros(tuple(x.shape), dtype=torch.float64)
    A = torch.zeros_like(dx)
    for _, _, so, si in taps:
        dx[si] += d64[so]
        A[si] += d64[so].abs()
    bound = _bwd_bound(dx, A, windows_over_a_pixel(KH, KW, S) + (4 if mode == "avg" else 2))
    if relu == 1:
        live = (_f64(x) > 0).to(torch.float64)
        dx, bound = dx * live, bound * live
    return dx, bound


def tie_all_backward_ref(x, y, dy, KH, KW, S, P, relu=False):
    """(dx, bound) of the max-unpool with the reference's tie rule: every input equal to its
    window's saved maximum y receives that window's dy; relu: the comparison is of relu(x) and the
    result is masked by x > 0.  The max-backward bound."""
    x64, y64, d64 = _f64(x), _f64(y), _f64(dy)
    xv = x64.clamp_min(0) if relu else x64
    taps, _ = _taps(x.shape, KH, KW, S, P)
    dx = torch.zeros(tuple(x.shape), dtype=torch.float64)
    A = torch.zeros_like(dx)
    for _, _, so, si in taps:
        v = torch.where(xv[si] == y64[so], d64[so], torch.zeros_like(d64[so]))
        dx[si] += v
        A[si] += v.abs()
    bound = _bwd_bound(dx, A, windows_over_a_pixel(KH, KW, S) + 2)
    if relu:
        live = (x64 > 0).to(torch.float64)
        dx, bound = dx * live, bound * live
    return dx, bound


# ------------------------------------------------------------------------------------- emulation
def _f32_inv(KH, KW):
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(KH * KW), dtype=torch.float32)


def emulate_forward(x, KH, KW, S, P, mode, relu_flags=0):
    """What the kernels compute in sum / avg mode: an fp32 sum over the taps in h-major order, the
    multiply by the fp32 1 / (KH KW), one rounding to bf16."""
    xf = x.detach().cpu().float()
    if relu_flags & 1:
        xf = xf.clamp_min(0)
    taps, (Ho, Wo) = _taps(xf.shape, KH, KW, S, P)
    acc = torch.zeros((xf.shape[0], Ho, Wo, xf.shape[3]), dtype=torch.float32)
    for _, _, so, si in taps:
        acc[so] = acc[so] + xf[si]
    if mode == "avg":
        acc = acc * _f32_inv(KH, KW)
    return acc.to(torch.bfloat16)


def emulate_backward(x, state, dy, KH, KW, S, P, mode, relu=0):
    """What the gather kernels compute: per pixel an fp32 sum over the covering windows in (ho, wo)
    order (the taps in descending order), max: of the windows whose recorded byte is the tap;
    avg: of dy times the fp32 1 / (KH KW); the relu mask; one rounding to bf16."""
    df = dy.detach().cpu().float()
    taps, _ = _taps(x.shape, KH, KW, S, P)
    g = torch.zeros(tuple(x.shape), dtype=torch.float32)
    st = state.detach().cpu() if mode == "max" else None
    inv = _f32_inv(KH, KW)
    for kh, kw, so, si in reversed(taps):
        if mode == "max":
            g[si] = g[si] + torch.where(st[so] == kh * KW + kw, df[so], torch.zeros_like(df[so]))
        else:
            g[si] = g[si] + (df[so] * inv if mode == "avg" else df[so])
    if relu == 1:
        g = torch.where(x.detach().cpu().float() > 0, g, torch.zeros_like(g))
    return g.to(torch.bfloat16)


# ------------------------------------------------------------------------------------- dispatch
S1K3_R = 4                     # output (forward) / input (backward) rows per strip of the s1k3 kernels
GLOBAL_POOL_MIN_WINDOW = 64    # windows above it (whole-map sum / avg) leave for se_kernels.hip


def fwd_kernel(c, flags):
    """The kernel cxn_pool_fwd launches for case c with the relu flags: its dispatch conditions
    restated (C % 8, stride, square kernel size, mode, pad, and flag 4 without flag 1 for the
    integer-key NN forms).  pool_fwd_rows<1,3,NN> is the one instantiation no ordinary geometry
    reaches: 3 x 3 / 1 max goes to the strips up to pad 2, and from pad 3 on the first window lies
    wholly in the padding (only CXXNET_POOL_STRIPS=0, read when the library loads, sends max there)."""
    if c.C % 8:
        return "pool_fwd<1>"
    nn = c.mode == "max" and flags & 4 and not flags & 1
    sq = c.KH if c.KH == c.KW else 0
    tag = ",NN>" if nn else ">"
    if c.S == 1 and sq == 3 and c.mode == "max" and c.P <= 2:
        return "pool_fwd_s1k3<4" + tag
    for s, k in ((2, 3), (1, 3), (2, 2)):
        if c.S == s and sq == k:
            return "pool_fwd_rows<%d,%d%s" % (s, k, tag)
    return "pool_fwd_rows<0,0>"


def bwd_kernel(c, dbias=False, cells=True):
    """The kernel ops.pool_backward reaches for case c (cells: the A/B variant of the 3 x 3 / 2
    max-unpool, on by default)."""
    if c.C % 8:
        return "pool_bwd<1>+bias_grad" if dbias else "pool_bwd<1>"
    if dbias:
        return "pool_bwd<8>"
    sq = c.KH if c.KH == c.KW else 0
    if c.S == 1 and sq == 3 and c.mode == "max" and c.P <= 2:
        return "pool_bwd_s1k3<4>"
    if c.S == 2 and sq == 3 and c.mode == "max" and cells:
        return "pool_bwd_s2k3"
    for s, k in ((2, 3), (1, 3), (2, 2)):
        if c.S == s and sq == k:
            return "pool_bwd_rows<%d,%d>" % (s, k)
    return "pool_bwd_rows<0,0>"


# ------------------------------------------------------------------------------------- the cases
# fwd / bwd: the kernel the case is meant to reach with flags 0 / without dbias (fwd_kernel and
# bwd_kernel must agree: asserted below); dbias: also run the backward with a bias gradient
# (C % 8 == 0: pool_bwd<8>, else pool_bwd<1> and a bias_grad pass); alias: also run the backward
# with dx aliasing x and relu = 1; tie: also run pool_bwd_tie_all
Case = namedtuple("Case", "N H W C KH KW S P mode fwd bwd dbias alias tie", defaults=(False, False, False))

CASES = {
    # C % 8 != 0: the grid-stride scalar kernels (378 outputs / 1638 inputs: more than one block)
    "c3_max_k3s2": Case(3, 13, 14, 3, 3, 3, 2, 0, "max", "pool_fwd<1>", "pool_bwd<1>", alias=True, tie=True),
    "c12_avg_k3s1p1": Case(1, 6, 7, 12, 3, 3, 1, 1, "avg", "pool_fwd<1>", "pool_bwd<1>"),
    "c12_max_k2s2": Case(3, 7, 5, 12, 2, 2, 2, 0, "max", "pool_fwd<1>", "pool_bwd<1>", dbias=True),
    "c3_sum_k2x3s1": Case(1, 5, 4, 3, 2, 3, 1, 0, "sum", "pool_fwd<1>", "pool_bwd<1>", dbias=True),
    # 3 x 3 / 2: odd x even, even x odd, a 2 x 3 map; pads 0 and 1 (max backward: 2 x 2 cells)
    "k3s2_max_9x8": Case(3, 9, 8, 40, 3, 3, 2, 0, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3", alias=True),
    "k3s2_max_8x13p1": Case(1, 8, 13, 16, 3, 3, 2, 1, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3"),
    "k3s2_max_2x3p1": Case(3, 2, 3, 8, 3, 3, 2, 1, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3"),
    "k3s2_max_7x6p1": Case(1, 7, 6, 8, 3, 3, 2, 1, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3"),
    "k3s2_max_6x7": Case(3, 6, 7, 16, 3, 3, 2, 0, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3", tie=True),
    "k3s2_avg_9x8": Case(3, 9, 8, 8, 3, 3, 2, 0, "avg", "pool_fwd_rows<2,3>", "pool_bwd_rows<2,3>", alias=True),
    "k3s2_sum_8x7p1": Case(1, 8, 7, 16, 3, 3, 2, 1, "sum", "pool_fwd_rows<2,3>", "pool_bwd_rows<2,3>"),
    # 3 x 3 / 1 in sum and avg mode
    "k3s1_avg_5x6p1": Case(3, 5, 6, 8, 3, 3, 1, 1, "avg", "pool_fwd_rows<1,3>", "pool_bwd_rows<1,3>"),
    "k3s1_sum_6x5": Case(1, 6, 5, 24, 3, 3, 1, 0, "sum", "pool_fwd_rows<1,3>", "pool_bwd_rows<1,3>"),
    # 2 x 2 / 2
    "k2s2_max_7x6": Case(3, 7, 6, 16, 2, 2, 2, 0, "max", "pool_fwd_rows<2,2>", "pool_bwd_rows<2,2>"),
    "k2s2_max_6x8p1": Case(1, 6, 8, 8, 2, 2, 2, 1, "max", "pool_fwd_rows<2,2>", "pool_bwd_rows<2,2>"),
    "k2s2_avg_6x8p1": Case(3, 6, 8, 8, 2, 2, 2, 1, "avg", "pool_fwd_rows<2,2>", "pool_bwd_rows<2,2>"),
    # everything else: the generic <0,0> kernels
    "k2s1_max_5x6": Case(3, 5, 6, 8, 2, 2, 1, 0, "max", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>", tie=True),
    "k3s3_max_8x10": Case(1, 8, 10, 16, 3, 3, 3, 0, "max", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    "k5s2_max_9x12p2": Case(1, 9, 12, 8, 5, 5, 2, 2, "max", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    "k5s2_avg_9x12p2": Case(3, 9, 12, 8, 5, 5, 2, 2, "avg", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    "k2x3s2_max_7x8": Case(3, 7, 8, 8, 2, 3, 2, 0, "max", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    "k2x3s2_sum_7x8": Case(1, 7, 8, 16, 2, 3, 2, 0, "sum", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    # the whole 7 x 7 map: 49 taps <= GLOBAL_POOL_MIN_WINDOW, so it stays on pool_fwd_rows
    "k7s1_avg_7x7": Case(3, 7, 7, 16, 7, 7, 1, 0, "avg", "pool_fwd_rows<0,0>", "pool_bwd_rows<0,0>"),
    # the folded bias gradient: C / 8 in {1, 3, 5}; the grid is rounded down to a multiple of
    # m = (C / 8) / gcd(C / 8, 256), at least m: c24_avg 4 blocks -> 3, c40 8 blocks -> 5, c24_sum 1 block -> 3
    "db_c8_max_k3s2": Case(3, 9, 8, 8, 3, 3, 2, 0, "max", "pool_fwd_rows<2,3>", "pool_bwd_s2k3", dbias=True),
    "db_c24_avg_k2s2": Case(3, 10, 9, 24, 2, 2, 2, 0, "avg", "pool_fwd_rows<2,2>", "pool_bwd_rows<2,2>", dbias=True,
                            alias=True),
    "db_c40_max_k3s1p1": Case(3, 11, 12, 40, 3, 3, 1, 1, "max", "pool_fwd_s1k3<4>", "pool_bwd_s1k3<4>", dbias=True),
    "db_c24_sum_k3s2": Case(1, 6, 7, 24, 3, 3, 2, 0, "sum", "pool_fwd_rows<2,3>", "pool_bwd_rows<2,3>", dbias=True),
}


def _add_s1k3():
    """3 x 3 / 1 max on strips of four rows: for each pad, the heights that give the forward Ho in
    {3, 4, 5, 9} output rows (fewer than one strip, one full strip, a partial last strip) and the
    backward H in {3, 4, 5, 9} input rows; W = H + 1 or H + 2."""
    for P in (0, 1, 2):
        hs = sorted({3, 4, 5, 9} | {ho + 2 - 2 * P for ho in (3, 4, 5, 9)})
        for i, H in enumerate(hs):
            CASES["k3s1_max_h%dp%d" % (H, P)] = Case((3, 1)[i % 2], H, H + 1 + i % 2, (24, 8)[i % 2], 3, 3, 1, P, "max",
                                                     "pool_fwd_s1k3<4>", "pool_bwd_s1k3<4>", alias=(H == 9 and P == 1),
                                                     tie=(H == 5 and P == 1))


_add_s1k3()


def assert_no_empty_window(name, c):
    assert not has_empty_window(c.H, c.KH, c.S, c.P) and not has_empty_window(c.W, c.KW, c.S, c.P), \
        "%s: a window lies wholly in the padding" % name


def _check_table():
    for name, c in CASES.items():
        assert_no_empty_window(name, c)
        assert c.mode in MODES and c.KH <= c.H + 2 * c.P and c.KW <= c.W + 2 * c.P, name
        assert c.N * c.H * c.W * c.C <= 100000, name
        assert fwd_kernel(c, 0) == c.fwd and bwd_kernel(c) == c.bwd, (name, fwd_kernel(c, 0), bwd_kernel(c))
        assert not (c.mode == "avg" and c.KH * c.KW > GLOBAL_POOL_MIN_WINDOW), name
        assert not c.tie or c.mode == "max", name
        if c.dbias:
            assert c.N * c.H * c.W <= DBIAS_R_MAX, name


_check_table()


def out_shape(c):
    return (c.N, out_size(c.H, c.KH, c.S, c.P), out_size(c.W, c.KW, c.S, c.P), c.C)


# forward flags run per kind of input (bit 0: relu in the pool; bit 1: mark relu' in the state's
# bit 7; bit 2: the input is >= 0, which sends the fixed-window max kernels to their integer keys)
FWD_FLAGS = {"signed": (0, 1, 2, 3), "nonneg": (0, 2, 4, 6)}
SUM_FLAGS = (0, 1)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of the case's CPU tensors, made once: x (bf16; "signed"), xn (bf16 >= 0; "nonneg", max
    cases), dy (bf16).  Max cases draw from seven values a quarter apart, so exact ties are
    frequent; channel 1 is all <= 0 (signed: negative; nonneg: 0) so that every window of it is
    marked when flag 2 is on, channel 2 is 0 over the upper left quarter, and a few -0.0 are
    planted.  Sum and avg cases draw from a normal distribution."""
    c = CASES[name]
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    shape = (c.N, c.H, c.W, c.C)
    out = {"dy": torch.randn(out_shape(c), generator=gen).to(torch.bfloat16)}
    if c.mode != "max":
        out["x"] = torch.randn(shape, generator=gen).to(torch.bfloat16)
        return out
    x = torch.randint(-3, 4, shape, generator=gen).float() * 0.25
    x[..., 1] = -x[..., 1].abs() - 0.25 * (x[..., 1] == 0)
    xn = x.clamp_min(0)
    xn[:, :c.H // 2 + 1, :c.W // 2 + 1, 2] = 0
    for t in (x, xn):
        flat = t.reshape(-1)
        zeros = torch.nonzero(flat == 0).reshape(-1)
        flat[zeros[::3]] = -0.0
    out["x"], out["xn"] = x.to(torch.bfloat16), xn.to(torch.bfloat16)
    return out


def data(name, kind):
    return inputs(name)["xn" if kind == "nonneg" else "x"]


@functools.lru_cache(maxsize=None)
def forward_ref(name, kind, flags):
    """max: (y, state) of max_forward_ref; sum / avg: (ref, bound) of sum_forward_ref; on the
    case's data of that kind with the flags' bits 0 and 1 (bit 2 changes the kernel, not the
    result).  Computed once and shared; the tensors must be left unchanged."""
    c = CASES[name]
    x = data(name, kind)
    if c.mode == "max":
        return max_forward_ref(x, c.KH, c.KW, c.S, c.P, flags & 3)
    return sum_forward_ref(x, c.KH, c.KW, c.S, c.P, c.mode, flags & 1)


# (kind of input, forward flags that made the state, backward relu) of the backward runs
BWD_RUNS = {"max": (("signed", 0, 0), ("signed", 1, 1), ("nonneg", 2, 2), ("signed", 3, 2)),
            "sum": (("signed", 0, 0), ("signed", 0, 1)),
            "avg": (("signed", 0, 0), ("signed", 0, 1))}


@functools.lru_cache(maxsize=None)
def backward_ref(name, kind, flags, relu):
    """(dx, bound) of the case's backward with the reference state of forward_ref(name, kind,
    flags); shared and to be left unchanged."""
    c = CASES[name]
    x, dy = data(name, kind), inputs(name)["dy"]
    if c.mode == "max":
        return max_backward_ref(x, forward_ref(name, kind, flags)[1], dy, c.KH, c.KW, c.S, c.P, relu)
    return sum_backward_ref(x, dy, c.KH, c.KW, c.S, c.P, c.mode, relu)


@functools.lru_cache(maxsize=None)
def tie_all_ref(name, relu):
    """(y as bf16, dx, bound) of the tie_all backward on the case's signed data"""
    c = CASES[name]
    x, dy = data(name, "signed"), inputs(name)["dy"]
    y = max_forward_ref(x, c.KH, c.KW, c.S, c.P, int(relu))[0]
    return (y.to(torch.bfloat16),) + tie_all_backward_ref(x, y, dy, c.KH, c.KW, c.S, c.P, relu)


def assert_exact(got, ref, what, axes="nhwc"):
    """got == ref for every element (a numeric compare: -0.0 == 0.0; a NaN fails), reported like
    assert_within: a bound of 0 everywhere."""
    return assert_within(got, _f64(ref), torch.zeros(tuple(ref.shape), dtype=torch.float64), what, axes=axes)
