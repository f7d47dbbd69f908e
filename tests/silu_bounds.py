"""Float64 references, derived per-element bounds, shared test inputs and fp32 emulations of silu
(csrc/kernels/silu_kernels.hip, layers/extra.py SiluLayer).  x, g are flat bf16;

    forward    y  = x s,                  s = sigma(x) = 1 / (1 + e),  e = e^-x
    backward   dx = g s (1 + x (1 - s))   (the derivative taken from the input x)

The bounds have the form of tests/bounds.py and tests/hact_bounds.py: u = 2^-8 the bf16 unit
roundoff of the store, eps32 = 2^-23 charged per fp32 rounding (twice round-to-nearest's 2^-24, and
what a transcendental published at one ulp costs).

    forward   u |ref| + K eps32 (1 + |x|) |ref|                         K = K_SILU_FWD = 4
        s's relative sensitivity to e is e / (1 + e) = 1 - s <= 1.  x * (1 / (1 + e)) with
        e = exp2(x * -log2(e)), the kernels' order: the exp2, the sum 1 + e, the reciprocal and the
        product by x are 4 roundings of the result's own size; the exponent's scaling (the rounded
        constant and the product with it) is 2 roundings of an exponent of size |x| log2(e), each
        ln(2) |x| log2(e) eps32 = |x| eps32 in e's relative error: (4 + 2 |x|) eps32 at most, which
        4 (1 + |x|) holds.  x / (1 + e): the exp, the sum, the quotient: 3, and an exp that takes x
        itself has no scaling term.
        + 2^-134, half the bf16 subnormal spacing, where 0 < |ref| < 2^-126: the store rounds to a
        multiple of 2^-133 there (x = +-2^-133 gives ref = x / 2), so u |ref| is not its error.
        + |ref| where x <= -87: s is below fp32's normal range there (e^87 > 2^125), and whether the
        device keeps such an s or makes it +0 (the reciprocal and the exp keep no subnormals; from
        x = -88.8 on e is +inf) is not prescribed: both ref and a zero are inside.
    backward  u |ref| + K' eps32 |g| (1 + |x|)                          K' = K_SILU_BWD = 10
        an ABSOLUTE term: what is left of the bound where ref cancels, at the zero of silu'
        (x = -1.2785; at its bf16 neighbours, where |silu'| is 1e-3, more than half of u |ref|).  With u_ = 1 - s, q = 1 + x u_ and ds the error of s, ds <= (3 + 2 |x| u_) eps32 s
        (the forward's count without the product; |x| s u_ <= 0.224 makes that <= 3.46 eps32):
            |dx - ref| / |g| <= s |x| ds + 2 eps32 s |x| u_ + |q| ds + 3 eps32 s |q|
        (ds carried through 1 - s and the product by x; the roundings of 1 - s and x u_; ds times q;
        the roundings of 1 + p and of the two products).  |q| ds <= (1 + |x| u_) (3 + 2 |x| u_) s
        eps32 <= 3.8 eps32 (its maximum, at x = 1.97) and s |q| = |silu'| <= 1.1, so the sum is at
        most (3.46 |x| + 0.45 + 3.8 + 3.3) eps32 <= 8 (1 + |x|) eps32.  The expanded order
        g (s + x (s u_)) has one product more; K' = 10 holds both.  Where x <= -87 the term is
        2^-20 |g| (1 + |x|) against a ref below 2^-120 |g|: ref and a zero are both inside.
    where sigma rounds to 1 in fp32 (x >= 17.33, e < 2^-25) an fp32 evaluation gives y = x and
    dx = g, the same bits; the bounds do not demand it (the tests check it at 88, 100 and 2^8).

Next to u |ref| the forward's eps32 term is 68 2^-15 = 2^-8.9 of it at most for |x| <= 16; the
backward's is that small wherever silu' is of order 1.  Derived, not tuned.
Everything runs on the CPU."""
import functools

import torch

from bounds import EPS_F32, U_BF16, assert_within, violations  # noqa: F401

K_SILU_FWD, K_SILU_BWD = 4, 10
BF16_MIN_NORMAL, BF16_HALF_SUBNORMAL = 2.0 ** -126, 2.0 ** -134
SIGMA_SUBNORMAL_X = -87.0        # from here down sigma(x) < 2^-125: fp32 may hold it as a subnormal, or as +0
SILU_GRAD_ZERO = -1.2784645      # the zero of silu'
# -0.0 first; the subnormal neighbours of 0; the values nearest 0 whose result (x / 2) is a normal bf16
# number; the bf16 neighbours on both sides of the zero of silu' (-164/128, -163/128); and the two ends
PLANTED_X = [-0.0, 0.0, -2.0 ** -133, 2.0 ** -133, -2.0 ** -125, 2.0 ** -125, -1.28125, -1.2734375,
             -8.0, 8.0, -16.0, 16.0, -2.0 ** 8, 2.0 ** 8, -88.0, 88.0, -100.0, 100.0]
PLANTED_G = [-0.0, 1.0]


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def planted_x():
    return list(PLANTED_X)


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(x, g): flat bf16 of n elements on the CPU.  x is uniform over [-16, 16], g is N(0, 1).  The
    planted values (PLANTED_X, and PLANTED_G in g) are written cyclically from element 0, as many as
    fit, and once more at the very end of the buffer (the last run, the tail of n % 8) where n
    allows: element i of the first len(PLANTED_X) holds PLANTED_X[i], and g[i] = PLANTED_G[i % 2]
    there (every positive planted x meets g = 1); at the end each x meets the other g."""
    gen = torch.Generator().manual_seed(4700 + n % 9973)
    x = (32.0 * torch.rand(n, generator=gen) - 16.0).to(torch.bfloat16)
    g = torch.randn(n, generator=gen).to(torch.bfloat16)
    px = torch.tensor(PLANTED_X, dtype=torch.float32).to(torch.bfloat16)
    m = min(n, px.numel())
    x[:m] = px[:m]
    g[:m] = torch.tensor([PLANTED_G[i % 2] for i in range(m)], dtype=torch.float32).to(torch.bfloat16)
    if n >= 2 * px.numel():
        x[n - px.numel():] = px
        g[n - px.numel():] = torch.tensor([PLANTED_G[(i + 1) % 2] for i in range(px.numel())]).to(torch.bfloat16)
    return x, g


def _sigma64(v):
    return 1.0 / (1.0 + torch.exp(-v))


def forward_ref(x):
    """(ref, bound), float64 of x's shape, of y = x sigma(x) stored as bf16."""
    v = _f64(x)
    ref = v * _sigma64(v)
    zero = torch.zeros_like(v)
    b = U_BF16 * ref.abs() + K_SILU_FWD * EPS_F32 * (1.0 + v.abs()) * ref.abs()
    b = b + torch.where((ref != 0) & (ref.abs() < BF16_MIN_NORMAL), torch.full_like(b, BF16_HALF_SUBNORMAL), zero)
    b = b + torch.where(v <= SIGMA_SUBNORMAL_X, ref.abs(), zero)
    return ref, b


def backward_ref(x, g):
    """(ref, bound), float64, of dx = g sigma(x) (1 + x (1 - sigma(x))) stored as bf16."""
    v, gv = _f64(x), _f64(g)
    s = _sigma64(v)
    ref = gv * s * (1.0 + v * (1.0 - s))
    b = U_BF16 * ref.abs() + K_SILU_BWD * EPS_F32 * gv.abs() * (1.0 + v.abs())
    return ref, b


@functools.lru_cache(maxsize=8)
def case_ref(n):
    """{"y": (ref, bound), "dx": (ref, bound)} of inputs(n), computed once and shared (the last few:
    the largest case's float64 tensors are not kept for the whole session)."""
    x, g = inputs(n)
    return {"y": forward_ref(x), "dx": backward_ref(x, g)}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------ fp32 emulation
ORDERS = ("recip", "quot")  # x * (1 / (1 + e)) and g s (1 + x (1 - s));  x / (1 + e) and g (s + x (s (1 - s)))


def emulate_forward(x, order):
    v = x.float()
    e = torch.exp(-v)
    out = v * (1.0 / (1.0 + e)) if order == "recip" else v / (1.0 + e)
    return out.to(torch.bfloat16)


def emulate_backward(x, g, order):
    v, gv = x.float(), g.float()
    s = 1.0 / (1.0 + torch.exp(-v))
    out = gv * s * (1.0 + v * (1.0 - s)) if order == "recip" else gv * (s + v * (s * (1.0 - s)))
    return out.to(torch.bfloat16)


def bump_ulps(t, flat_index, ulps=2):
    """A copy of bf16 tensor t with one element moved away from zero by `ulps` bf16 ulps."""
    out = t.clone()
    out.view(-1).view(torch.int16)[flat_index] += ulps
    return out
