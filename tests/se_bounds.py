"""Float64 references, derived per-element bounds, shared test inputs and an fp32 emulation of the
squeeze-and-excitation kernels (csrc/kernels/se_kernels.hip): `ch_scale` forward and backward and
the global sum / avg pooling.  x, g are [B][H][W][C] bf16, the gate s is [B][C] bf16.

The bounds have the form of tests/bounds.py, u = 2^-8 the bf16 unit roundoff:
    y = x s, dx = g s    the product of two bf16 values has 16 significand bits: exact in fp32, so
                         the store is the only rounding:  bound = u |ref|  (0 where ref is 0: such
                         an element must be +-0 exactly)
    ds[b,c] = sum_hw g x     N = H W exact products summed in fp32 in any order, one rounding:
    pooled  = sum_hw x       bound = u (|ref| + g A) + g A,  A = the sum of the terms' magnitudes,
                             g = gamma(N) = (N + 2) 2^-23 as in bounds.py (N - 1 additions err by at
                             most (N - 1) 2^-24 A in any order; the slack of (N + 5) 2^-24 holds the
                             avg's two extra roundings, 1 / N as an fp32 number and the multiply)
At N = 3136 (56 x 56) g A is several times u |ref| for random terms, so there the bound of a sum
sees a missing part or pixel run, not a misrounded store; up to N = 196 it sees two bf16 ulps
(test_se_bounds_cpu.py shows both).  Derived, not tuned.  Everything runs on the CPU."""
import functools

import torch

from bounds import EPS_F32, U_BF16, assert_within, gamma, violations  # noqa: F401

# name -> ((B, H, W, C), element offset of every view into its 16-byte aligned buffer)
CASES = {
    "b2c8": ((2, 1, 1, 8), 0),        # one pixel, one channel group
    "h3w5": ((1, 3, 5, 8), 0),        # fewer pixels than pixel lanes
    "c64": ((2, 7, 7, 64), 0),        # 8 group lanes x 32 pixel lanes, one part
    "c24": ((3, 14, 14, 24), 0),      # 3 group lanes: 85 pixel lanes, one idle thread
    "c3": ((2, 5, 5, 3), 0),          # C % 8 != 0: the scalar path
    "off1": ((1, 3, 5, 8), 1),        # C % 8 == 0 but every buffer starts 2 bytes past alignment: scalar path
    "multi": ((2, 56, 56, 16), 0),    # the map is cut into parts: fp32 partials and the merge launch
    "c3multi": ((2, 40, 40, 3), 0),   # parts on the scalar path
}
MULTI = ("multi", "c3multi")          # the cases whose part count must be > 1
POOL_CASES = {                        # global pooling: C % 8 == 0 and more than 64 pixels (the routed shapes)
    "p9": (2, 9, 9, 8),
    "p14": (1, 14, 14, 24),
    "p56": (2, 56, 56, 16),
}


def _f64(t):
    return t.detach().to("cpu", torch.float64)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x, s, g) of the case: bf16, on the CPU, x and g [B][H][W][C], s [B][C] in (0, 1).  Planted:
    s = 0 exactly on channel 0 and 1 exactly on channel 1; -0.0 in x at (0, 0, 0, 1), so that
    y there is -0.0 * 1; and where the map has at least two pixels: the column (B - 1, C - 1)
    whose g x terms cancel exactly in pairs (x equal, g opposite; an odd last pixel has x = 0),
    and 2^8 next to 2^-8 in the column (0, 2) of x, with g = 1 on both."""
    B, H, W, C = CASES[name][0] if name in CASES else POOL_CASES[name]
    gen = torch.Generator().manual_seed(4200 + B * H * W * C + len(name))
    x = torch.randn(B, H * W, C, generator=gen).to(torch.bfloat16)
    g = torch.randn(B, H * W, C, generator=gen).to(torch.bfloat16)
    s = torch.rand(B, C, generator=gen).to(torch.bfloat16)
    s[:, 0], s[:, 1] = 0.0, 1.0
    x[0, 0, 1] = -0.0
    HW = H * W
    if HW >= 2:
        n2 = HW // 2
        x[B - 1, 1:2 * n2:2, C - 1] = x[B - 1, 0:2 * n2:2, C - 1]
        g[B - 1, 1:2 * n2:2, C - 1] = -g[B - 1, 0:2 * n2:2, C - 1]
        if HW % 2:
            x[B - 1, HW - 1, C - 1] = 0.0
        x[0, 0, 2], x[0, 1, 2] = 2.0 ** 8, 2.0 ** -8
        g[0, 0, 2] = g[0, 1, 2] = 1.0
    return x.view(B, H, W, C), s, g.view(B, H, W, C)


def scale_ref(x, s):
    """(ref, bound), float64 [B][H][W][C], of x s[b, c] stored as bf16 (y of x, s; dx of g, s)."""
    B, C = x.shape[0], x.shape[3]
    ref = _f64(x) * _f64(s).reshape(B, 1, 1, C)
    return ref, U_BF16 * ref.abs()


def _sum_bound(ref, A, N):
    gA = gamma(N) * A
    return U_BF16 * (ref.abs() + gA) + gA


def ds_ref(g, x):
    """(ref, bound), float64 [B][C], of ds = sum over the map of g x stored as bf16."""
    t = _f64(g) * _f64(x)
    N = x.shape[1] * x.shape[2]
    ref, A = t.sum((1, 2)), t.abs().sum((1, 2))
    return ref, _sum_bound(ref, A, N)


def pool_ref(x, mode):
    """(ref, bound), float64 [B][C], of the global "sum" / "avg" pooling of x stored as bf16."""
    t = _f64(x)
    N = x.shape[1] * x.shape[2]
    k = 1.0 / N if mode == "avg" else 1.0
    ref, A = t.sum((1, 2)) * k, t.abs().sum((1, 2)) * k
    return ref, _sum_bound(ref, A, N)


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """dict of (ref, bound) pairs y, dx, ds of the case, computed once and shared."""
    x, s, g = inputs(name)
    return {"y": scale_ref(x, s), "dx": scale_ref(g, s), "ds": ds_ref(g, x)}


@functools.lru_cache(maxsize=None)
def pool_case_ref(name, mode):
    return pool_ref(inputs(name)[0], mode)


# ------------------------------------------------------------------ fp32 emulation
ORDERS = ("forward", "reversed", "pairwise")


def emulate_sum(terms, order):
    """fp32 sum over axis 1 of terms [B][N][C] (fp32) in the given order, kept in fp32."""
    t = terms.float()
    if order == "reversed":
        t = t.flip(1)
    if order in ("forward", "reversed"):
        acc = torch.zeros_like(t[:, 0])
        for i in range(t.shape[1]):
            acc = acc + t[:, i]
        return acc
    n = 1
    while n < t.shape[1]:
        n *= 2
    t = torch.cat([t, torch.zeros(t.shape[0], n - t.shape[1], t.shape[2])], 1)
    while t.shape[1] > 1:
        h = t.shape[1] // 2
        t = t[:, :h] + t[:, h:]
    return t[:, 0]


def emulate_scale(x, s):
    B, C = x.shape[0], x.shape[3]
    return (x.float() * s.float().reshape(B, 1, 1, C)).to(torch.bfloat16)


def emulate_ds(g, x, order):
    B, H, W, C = x.shape
    return emulate_sum((g.float() * x.float()).reshape(B, H * W, C), order).to(torch.bfloat16)


def emulate_pool(x, mode, order):
    B, H, W, C = x.shape
    acc = emulate_sum(x.float().reshape(B, H * W, C), order)
    if mode == "avg":
        acc = acc * torch.tensor(1.0 / (H * W), dtype=torch.float32)
    return acc.to(torch.bfloat16)


def bump_ulps(t, flat_index, ulps=2):
    """A copy of bf16 tensor t with one element moved away from zero by `ulps` bf16 ulps."""
    out = t.clone()
    out.view(-1).view(torch.int16)[flat_index] += ulps
    return out
