"""Float64 references, derived per-element bounds, shared test inputs and fp32 emulations of the
bounded activations relu6 / hsigmoid / hswish (csrc/kernels/hact_kernels.hip, layers/extra.py
HardActLayer).  x, g are flat bf16; "strictly inside" decides every breakpoint:

    kind       x <= lo    lo < x < hi            x >= hi     (lo, hi)
    relu6      y = +0     y = x                  y = 6       (0, 6)
               dx = 0     dx = g                 dx = 0
    hsigmoid   y = +0     y = (x + 3) / 6        y = 1       (-3, 3)
               dx = 0     dx = g / 6             dx = 0
    hswish     y = 0      y = x (x + 3) / 6      y = x       (-3, 3)
               dx = 0     dx = g (2 x + 3) / 6   dx = g

The bounds have the form of tests/bounds.py: u = 2^-8 the bf16 unit roundoff of the store,
eps32 = 2^-23 charged per fp32 rounding (twice round-to-nearest's 2^-24, as gamma() there), k the
number of roundings of the longest reasonable evaluation order, against the magnitude M the
roundings act on (every intermediate is at most M in absolute value):

    hsigmoid forward   u |ref| + k eps32 (|x| + 3) / 6            k = K_HSIGMOID_FWD = 3
        (x + 3) * (1/6 as an fp32 number): the sum, the constant's own rounding, the product: 3.
        (x + 3) / 6 divided: 2.  fma(x, 1/6f, 0.5f): the constant and the fma: 2.
    hswish forward     u |ref| + k eps32 |x| (|x| + 3) / 6        k = K_HSWISH_FWD = 4
        x * ((x + 3) * 1/6f): the three above and the product by x: 4.  x * (x + 3) / 6: the sum,
        the product, the quotient: 3.  x * fma(x, 1/6f, 0.5f): 3.
    hsigmoid backward  u |ref| + k eps32 |ref|                    k = K_HSIGMOID_BWD = 2
        g * 1/6f: the constant and the product: 2.  g / 6: 1.
    hswish backward    u |ref| + k eps32 |g| (2 |x| + 3) / 6      k = K_HSWISH_BWD = 4
        g * ((2 x + 3) * 1/6f): 2 x is exact; the sum, the constant, two products: 4.
        g * fma(x, 1/3f, 0.5f): 3.  g * (2 x + 3) / 6: 3.
    relu6, and every row of the table that says 0, 1, 6 or a copy of x or g: bound 0 -- the stored
    value is the reference exactly (a bf16 value widened to fp32 and rounded back keeps its bits;
    the tests compare relu6 bit for bit, -0.0 included).

    hswish forward below bf16's normal range, |ref| < 2^-126 (x = +-2^-133 gives ref = x / 2): the
    store rounds to a multiple of the subnormal spacing 2^-133, so u |ref| is not its error there;
    half that spacing, 2^-134, is added to the bound of those elements.  No other kind or
    direction can produce a subnormal that is not a copy of its input from these inputs (hsigmoid
    gives 1/2 next to 0, the backwards a multiple of a normal g), so no other bound has the term.

Next to u = 2^-8 the eps32 terms are 2^-13 of it at most, except where ref cancels (hswish' at
x = -1.5, hsigmoid at x next to -3): there they are the whole bound.  Derived, not tuned.
Everything runs on the CPU."""
import functools

import torch

from bounds import EPS_F32, U_BF16, assert_within, violations  # noqa: F401

KINDS = ("relu6", "hsigmoid", "hswish")
K_HSIGMOID_FWD, K_HSWISH_FWD, K_HSIGMOID_BWD, K_HSWISH_BWD = 3, 4, 2, 4
BF16_MIN_NORMAL, BF16_HALF_SUBNORMAL = 2.0 ** -126, 2.0 ** -134
LO_HI = {"relu6": (0.0, 6.0), "hsigmoid": (-3.0, 3.0), "hswish": (-3.0, 3.0)}


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def _bf16_neighbours(v):
    """the bf16 values just below and just above v (v a bf16 number); for 0 the smallest subnormals,
    -+2^-133"""
    if v == 0.0:
        return [-2.0 ** -133, 2.0 ** -133]
    t = torch.tensor([v], dtype=torch.bfloat16)
    bits = t.view(torch.int16)
    return [float((bits + d).view(torch.bfloat16)[0]) for d in (-1, 1)]


def planted_x():
    """-0.0, 0, +-3, 6; the bf16 neighbours on both sides of -3, 3, 0 (the subnormals +-2^-133) and
    6; -1.5 (the zero of hswish'); 2^8 and 2^-8; and +-2^-125, the values nearest 0 at which every
    kind's result is still a normal bf16 number (hswish gives x / 2 = 2^-126 there).  -0.0 comes
    first.  The subnormals are what sees a flush to zero in a compare, a select or the store."""
    vals = [-0.0, 0.0, 3.0, -3.0, 6.0]
    for v in (-3.0, 3.0, 0.0, 6.0):
        vals += _bf16_neighbours(v)
    return vals + [-1.5, 2.0 ** 8, 2.0 ** -8, -2.0 ** -125, 2.0 ** -125]


PLANTED_G = [-0.0, 1.0]


@functools.lru_cache(maxsize=None)
def inputs(n):
    """(x, g): flat bf16 of n elements on the CPU.  x is spread over [-8, 8] (3 N(0, 1) clipped)
    so that every piece of every kind is hit, g is N(0, 1).  The planted values (planted_x, and
    PLANTED_G in g) are written cyclically from element 0, as many as fit, and once more at the
    very end of the buffer (the last run, the tail of n % 8) where n allows: element i of the
    first len(planted_x()) holds planted_x()[i], and g[i] = PLANTED_G[i % 2] there."""
    gen = torch.Generator().manual_seed(4300 + n % 9973)
    x = (3.0 * torch.randn(n, generator=gen)).clamp_(-8.0, 8.0).to(torch.bfloat16)
    g = torch.randn(n, generator=gen).to(torch.bfloat16)
    px = torch.tensor(planted_x(), dtype=torch.float32).to(torch.bfloat16)
    m = min(n, px.numel())
    x[:m] = px[:m]
    g[:m] = torch.tensor([PLANTED_G[i % 2] for i in range(m)], dtype=torch.float32).to(torch.bfloat16)
    if n >= 2 * px.numel():
        x[n - px.numel():] = px
        g[n - px.numel():] = torch.tensor([PLANTED_G[(i + 1) % 2] for i in range(px.numel())]).to(torch.bfloat16)
    return x, g


def forward_ref(kind, x):
    """(ref, bound), float64 of x's shape, of y = f(x) stored as bf16."""
    v = _f64(x)
    lo, hi = LO_HI[kind]
    inside = (v > lo) & (v < hi)
    zero = torch.zeros_like(v)
    if kind == "relu6":
        return torch.where(inside, v, torch.where(v >= hi, torch.full_like(v, 6.0), zero)), zero
    if kind == "hsigmoid":
        ref = torch.where(inside, (v + 3.0) / 6.0, torch.where(v >= hi, torch.ones_like(v), zero))
        b = U_BF16 * ref.abs() + K_HSIGMOID_FWD * EPS_F32 * (v.abs() + 3.0) / 6.0
    else:
        ref = torch.where(inside, v * (v + 3.0) / 6.0, torch.where(v >= hi, v, zero))
        b = U_BF16 * ref.abs() + K_HSWISH_FWD * EPS_F32 * v.abs() * (v.abs() + 3.0) / 6.0
        b = b + torch.where((ref != 0) & (ref.abs() < BF16_MIN_NORMAL), torch.full_like(b, BF16_HALF_SUBNORMAL), zero)
    return ref, torch.where(inside, b, zero)


def backward_ref(kind, x, g):
    """(ref, bound), float64, of dx = g f'(x) stored as bf16."""
    v, gv = _f64(x), _f64(g)
    lo, hi = LO_HI[kind]
    inside = (v > lo) & (v < hi)
    zero = torch.zeros_like(v)
    if kind == "relu6":
        return torch.where(inside, gv, zero), zero
    if kind == "hsigmoid":
        ref = torch.where(inside, gv / 6.0, zero)
        b = U_BF16 * ref.abs() + K_HSIGMOID_BWD * EPS_F32 * ref.abs()
    else:
        ref = torch.where(inside, gv * (2.0 * v + 3.0) / 6.0, torch.where(v >= hi, gv, zero))
        b = U_BF16 * ref.abs() + K_HSWISH_BWD * EPS_F32 * gv.abs() * (2.0 * v.abs() + 3.0) / 6.0
    return ref, torch.where(inside, b, zero)


@functools.lru_cache(maxsize=8)
def case_ref(kind, n):
    """{"y": (ref, bound), "dx": (ref, bound)} of inputs(n), computed once and shared (the last few:
    the largest case's float64 tensors are not kept for the whole session)."""
    x, g = inputs(n)
    return {"y": forward_ref(kind, x), "dx": backward_ref(kind, x, g)}


def ref_bits(ref):
    """the bf16 bit patterns (int16) of a float64 reference whose values are bf16 numbers (relu6)"""
    return ref.to(torch.bfloat16).view(torch.int16)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------ fp32 emulation
ORDERS = ("sum_div", "sum_mul", "fma")
_SIXTH = torch.tensor(1.0 / 6.0, dtype=torch.float32)
_THIRD = torch.tensor(1.0 / 3.0, dtype=torch.float32)


def _fma32(a, b, c):
    """fp32 fma: the product and the sum are exact in float64 for fp32 operands of this range
    (24 + 24 significand bits), then one rounding"""
    return (a.double() * b.double() + c.double()).float()


def _ramp(v, order):
    """(x + 3) / 6 in fp32 in the given order"""
    if order == "sum_div":
        return (v + 3.0) / 6.0
    if order == "sum_mul":
        return (v + 3.0) * _SIXTH
    return _fma32(v, _SIXTH, torch.tensor(0.5))


def emulate_forward(kind, x, order):
    v = x.float()
    lo, hi = LO_HI[kind]
    inside = (v > lo) & (v < hi)
    zero = torch.zeros_like(v)
    if kind == "relu6":
        out = torch.where(inside, v, torch.where(v >= hi, torch.full_like(v, 6.0), zero))
    elif kind == "hsigmoid":
        out = torch.where(inside, _ramp(v, order), torch.where(v >= hi, torch.ones_like(v), zero))
    else:
        out = torch.where(inside, v * _ramp(v, order), torch.where(v >= hi, v, zero))
    return out.to(torch.bfloat16)


def emulate_backward(kind, x, g, order):
    v, gv = x.float(), g.float()
    lo, hi = LO_HI[kind]
    inside = (v > lo) & (v < hi)
    zero = torch.zeros_like(v)
    if kind == "relu6":
        out = torch.where(inside, gv, zero)
    elif kind == "hsigmoid":
        out = torch.where(inside, gv / 6.0 if order == "sum_div" else gv * _SIXTH, zero)
    else:
        if order == "sum_div":
            s = (2.0 * v + 3.0) / 6.0
        elif order == "sum_mul":
            s = (2.0 * v + 3.0) * _SIXTH
        else:
            s = _fma32(v, _THIRD, torch.tensor(0.5))
        out = torch.where(inside, gv * s, torch.where(v >= hi, gv, zero))
    return out.to(torch.bfloat16)


def bump_ulps(t, flat_index, ulps=2):
    """A copy of bf16 tensor t with one element moved away from zero by `ulps` bf16 ulps."""
    out = t.clone()
    out.view(-1).view(torch.int16)[flat_index] += ulps
    return out
