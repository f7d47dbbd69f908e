"""Float64 references and derived per-element error bounds for the group_norm kernels
(csrc/kernels/gn_kernels.hip), in the style of tests/bn_bounds.py: the operands are the exact
bf16 / fp32 values the kernel reads, the reference is float64 on the CPU, and every bound comes
from the arithmetic -- none is tuned to what a kernel gives.

Tensors are x, g, y, dx [B][HW][C]; group q of a sample owns channels [q Cg, (q + 1) Cg), Cg = C / G,
m = HW Cg elements.  u = 2^-23, U = 2^-8 and g(n) = (n + 2) u as in bn_bounds.

Statistics per (sample, group), fp32 results checked directly.  The m elements of a (sample, group)
are one column of bn_bounds.stats_ref (its derivation asks nothing of the order in which a
Welford / pairwise-merge scheme visits the elements, so the cut into lanes, chunks and channels is
free), which gives mean, var (biased) and

  e_mean = g(m) sum|x| / m
  e_var  = g(m) var + 8 u max|x| sum|x - mean| / m + e_mean^2
  rstd = (var + eps)^-1/2:   e_rstd = rstd^3 e_var / 2 + 3 u rstd      (bn_bounds.inv_ref)

Forward (bf16), a = slope rstd, y = (x - mean) a + bias:

  y    U |ref| + |x - mean| |slope| e_rstd + |a| e_mean + 4 u (|x a| + |mean a| + |bias|)

Backward, xhat = (x - mean) rstd as the kernel forms it from its own fp32 statistics:

  e_xh = |x - mean| e_rstd + rstd e_mean + 3 u |xhat|        (the subtraction, the product, spare)
  gbias[c]  = gbias0 + sum_{b,hw} g:          g(B HW) (sum|g| + |gbias0|)
  gslope[c] = gslope0 + sum_{b,hw} g xhat:    (g(B HW) + 2 u) (sum|g xhat| + |gslope0|) + sum |g| e_xh
                                              (+ 2 u: the products g xhat are rounded)
  s1[b,q] = sum_{hw, c in q} slope g          e_s1 = (g(m) + 2 u) sum|slope g|
  s2[b,q] = sum_{hw, c in q} slope g xhat     e_s2 = (g(m) + 4 u) sum|slope g xhat| + sum |slope g| e_xh
  k1 = s1 / m, k2 = s2 / m                    e_k = e_s / m + u |k|
  t  = slope g - k1 - xhat k2                 e_t = e_k1 + |xhat| e_k2 + |k2| e_xh
                                                    + 4 u (|slope g| + |k1| + |xhat k2|)
  dx = rstd t (bf16)                          U |ref| + |t| e_rstd + rstd e_t + 2 u |ref|
"""
import torch

import bn_bounds as BN
from bn_bounds import U32, g
from bounds import U_BF16, assert_within, violations  # noqa: F401  (re-exported for the tests)


def _f64(t):
    return t.detach().to("cpu", torch.float64)


def _cols(x, G):
    """[B][HW][C] -> [m][B G]: column b G + q holds the m = HW Cg elements of (sample b, group q)."""
    B, HW, C = x.shape
    return x.reshape(B, HW, G, C // G).permute(1, 3, 0, 2).reshape(HW * (C // G), B * G)


def _per_elem(v, B, HW, C, G):
    """[B G] (or [B][G]) -> [B][HW][C]: a (sample, group) value at every element of the group."""
    return v.reshape(B, 1, G, 1).expand(B, HW, G, C // G).reshape(B, HW, C)


def _group_sum(v, G):
    """[B][HW][C] -> [B][G]: the sum over the elements of each (sample, group)."""
    B, HW, C = v.shape
    return v.reshape(B, HW, G, C // G).sum((1, 3))


def stats_ref(x, G, eps):
    """x [B][HW][C] (exact bf16 values) -> dict of float64 [B][G] mean, var (biased), rstd and their
    bounds e_mean, e_var, e_rstd; m the element count of a group."""
    B, HW, C = x.shape
    s = BN.stats_ref(_cols(x, G))
    rstd, e_rstd = BN.inv_ref(s["var"], s["e_var"], eps)
    out = {k: s[k].reshape(B, G) for k in ("mean", "var", "e_mean", "e_var")}
    out.update(rstd=rstd.reshape(B, G), e_rstd=e_rstd.reshape(B, G), m=s["R"])
    return out


def _elem_stats(x, G, eps):
    B, HW, C = x.shape
    s = stats_ref(x, G, eps)
    e = {k: _per_elem(s[k], B, HW, C, G) for k in ("mean", "rstd", "e_mean", "e_rstd")}
    return s, e


def forward_ref(x, slope, bias, G, eps):
    """(y ref, y bound, stats) of the forward; slope, bias fp32 [C]."""
    s, e = _elem_stats(x, G, eps)
    x, slope, bias = _f64(x), _f64(slope), _f64(bias)
    d = x - e["mean"]
    a = slope * e["rstd"]
    ref = d * a + bias
    bound = (U_BF16 * ref.abs() + d.abs() * slope.abs() * e["e_rstd"] + a.abs() * e["e_mean"]
             + 4 * U32 * ((x * a).abs() + (e["mean"] * a).abs() + bias.abs()))
    return ref, bound, s


def backward_ref(gy, x, slope, gslope0, gbias0, G, eps):
    """dict of (ref, bound) pairs for dx [B][HW][C], gslope [C], gbias [C]; the statistics are those
    of x."""
    B, HW, C = x.shape
    s, e = _elem_stats(x, G, eps)
    m = s["m"]
    gy, x, slope, gslope0, gbias0 = _f64(gy), _f64(x), _f64(slope), _f64(gslope0), _f64(gbias0)
    rstd, e_rstd = e["rstd"], e["e_rstd"]
    d = x - e["mean"]
    xh = d * rstd
    e_xh = d.abs() * e_rstd + rstd * e["e_mean"] + 3 * U32 * xh.abs()
    R = B * HW
    a_g, a_gx = gy.abs().sum((0, 1)), (gy * xh).abs().sum((0, 1))
    gbias = gbias0 + gy.sum((0, 1))
    gbias_b = g(R) * (a_g + gbias0.abs())
    gslope = gslope0 + (gy * xh).sum((0, 1))
    gslope_b = (g(R) + 2 * U32) * (a_gx + gslope0.abs()) + (gy.abs() * e_xh).sum((0, 1))
    sg = slope * gy
    s1, s2 = _group_sum(sg, G), _group_sum(sg * xh, G)
    e_s1 = (g(m) + 2 * U32) * _group_sum(sg.abs(), G)
    e_s2 = (g(m) + 4 * U32) * _group_sum((sg * xh).abs(), G) + _group_sum(sg.abs() * e_xh, G)
    k1, k2 = s1 / m, s2 / m
    e_k1, e_k2 = e_s1 / m + U32 * k1.abs(), e_s2 / m + U32 * k2.abs()
    k1, k2, e_k1, e_k2 = (_per_elem(v, B, HW, C, G) for v in (k1, k2, e_k1, e_k2))
    t = sg - k1 - xh * k2
    e_t = e_k1 + xh.abs() * e_k2 + k2.abs() * e_xh + 4 * U32 * (sg.abs() + k1.abs() + (xh * k2).abs())
    dx = rstd * t
    dx_b = U_BF16 * dx.abs() + t.abs() * e_rstd + rstd * e_t + 2 * U32 * dx.abs()
    return {"dx": (dx, dx_b), "gslope": (gslope, gslope_b), "gbias": (gbias, gbias_b)}


# ------------------------------------------------------------------ the cases of the kernel tests
# name: (B, HW, C, gn_group); each shape is the smallest that reaches a distinct code path
CASES = {
    "one_elem": (1, 1, 8, 8),        # one element per group: var = 0 exactly, y = bias, dx = 0
    "ln_pixel": (1, 1, 8, 1),        # layer norm of a single pixel
    "scalar": (2, 7, 6, 3),          # scalar path, Cg = 2
    "lane4groups": (3, 49, 64, 32),  # vector path, Cg = 2: a lane spans 4 groups
    "group2lanes": (2, 196, 64, 4),  # Cg = 16: a group spans 2 lanes
    "straddle": (2, 25, 24, 2),      # Cg = 12: a lane straddles a group boundary
    "partials": (1, 4099, 72, 9),    # many partials per sample, prime HW, C % 64 != 0
    "matrix": (5, 1, 1000, 1),       # matrix node, wide layer norm
    "bigmean": (3, 130, 64, 8),      # mean / std about 50 (bn_bounds.case_c_inputs)
}
EPS = 1e-5
_cache = {}


def case(name):
    """Inputs (CPU, exact bf16 / fp32) and float64 references of one case, computed once and shared
    by the tests; nobody writes to them."""
    if name in _cache:
        return _cache[name]
    B, HW, C, G = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "bigmean":
        x = BN.case_c_inputs(B * HW, C, 3).reshape(B, HW, C)
    else:
        x = (torch.randn(B, HW, C, generator=gen) * 1.5 + 0.7).to(torch.bfloat16)
    gy = torch.randn(B, HW, C, generator=gen).to(torch.bfloat16)
    slope = torch.rand(C, generator=gen) + 0.5
    bias = torch.randn(C, generator=gen)
    gs0, gb0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    y, y_b, s = forward_ref(x, slope, bias, G, EPS)
    bwd = backward_ref(gy, x, slope, gs0, gb0, G, EPS)
    _cache[name] = dict(B=B, HW=HW, C=C, G=G, x=x, gy=gy, slope=slope, bias=bias, gs0=gs0, gb0=gb0, y=y, y_b=y_b,
                        s=s, bwd=bwd)
    return _cache[name]
