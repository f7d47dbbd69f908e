"""tests/gn_bounds.py on the CPU.  fp32 emulations of the group_norm computation in two evaluation
orders -- one Welford walk over the elements of a (sample, group), and pairwise Chan merges from
single elements up -- stay inside every bound on every case of the kernel tests, so a correct fp32
kernel can meet them; a raw E[x^2] - E[x]^2 emulation breaks the variance bound on the large-mean
case, so the bound separates the schemes it is meant to separate; and the closed-form references
equal float64 autograd of the definition."""
import pytest
import torch

import gn_bounds as GB


def _welford(cols):
    """cols fp32 [m][N]: one sequential Welford walk per column -> (mean, var)."""
    mean = torch.zeros(cols.shape[1])
    m2 = torch.zeros(cols.shape[1])
    for i, r in enumerate(cols):
        d = r - mean
        mean = mean + d * (torch.tensor(1.0) / torch.tensor(float(i + 1)))
        m2 = m2 + d * (r - mean)
    return mean, m2 / float(cols.shape[0])


def _pairwise(cols):
    """cols fp32 [m][N]: (count, mean, M2) of single elements merged pairwise, level by level."""
    m = cols.shape[0]
    size = 1
    while size < m:
        size <<= 1
    n = torch.zeros(size, cols.shape[1])
    n[:m] = 1.0
    mean = torch.zeros(size, cols.shape[1])
    mean[:m] = cols
    m2 = torch.zeros(size, cols.shape[1])
    while n.shape[0] > 1:
        na, nb, ma, mb, qa, qb = n[0::2], n[1::2], mean[0::2], mean[1::2], m2[0::2], m2[1::2]
        nn = na + nb
        f = torch.where(nn > 0, nb / nn.clamp_min(1.0), torch.zeros_like(nn))
        d = mb - ma
        n, mean, m2 = nn, ma + d * f, qa + qb + d * d * na * f
    return mean[0], m2[0] / float(m)


def _emulate(c, stats):
    """The layer in fp32 torch from the given statistics scheme: what an fp32 kernel can reach."""
    B, HW, C, G = c["B"], c["HW"], c["C"], c["G"]
    Cg = C // G
    x, gy = c["x"].float(), c["gy"].float()
    mean, var = stats(GB._cols(x, G))
    rstd = 1.0 / torch.sqrt(var + torch.tensor(GB.EPS))
    me, re = (GB._per_elem(v, B, HW, C, G) for v in (mean, rstd))
    y = ((x - me) * (re * c["slope"]) + c["bias"]).to(torch.bfloat16)
    xh = (x - me) * re
    gbias = c["gb0"] + gy.sum((0, 1))
    gslope = c["gs0"] + (gy * xh).sum((0, 1))
    sg = c["slope"] * gy
    m = torch.tensor(float(HW * Cg))
    k1 = GB._per_elem(GB._group_sum(sg, G) / m, B, HW, C, G)
    k2 = GB._per_elem(GB._group_sum(sg * xh, G) / m, B, HW, C, G)
    dx = (re * (sg - k1 - xh * k2)).to(torch.bfloat16)
    assert all(t.dtype == torch.float32 for t in (mean, var, rstd, gbias, gslope))
    return dict(mean=mean.reshape(B, G), var=var.reshape(B, G), rstd=rstd.reshape(B, G), y=y, dx=dx, gslope=gslope,
                gbias=gbias)


@pytest.mark.parametrize("scheme", [_welford, _pairwise], ids=["welford", "pairwise"])
@pytest.mark.parametrize("name", list(GB.CASES))
def test_fp32_emulations_stay_inside_the_bounds(name, scheme):
    c = GB.case(name)
    out = _emulate(c, scheme)
    s = c["s"]
    GB.assert_within(out["mean"], s["mean"], s["e_mean"], "mean", axes="bg")
    GB.assert_within(out["var"], s["var"], s["e_var"], "var", axes="bg")
    GB.assert_within(out["rstd"], s["rstd"], s["e_rstd"], "rstd", axes="bg")
    GB.assert_within(out["y"], c["y"], c["y_b"], "y", axes="brc")
    GB.assert_within(out["dx"], *c["bwd"]["dx"], "dx", axes="brc")
    GB.assert_within(out["gslope"], *c["bwd"]["gslope"], "gslope", axes="c")
    GB.assert_within(out["gbias"], *c["bwd"]["gbias"], "gbias", axes="c")


def test_raw_moments_violate_the_variance_bound():
    c = GB.case("bigmean")
    cols = GB._cols(c["x"].float(), c["G"])
    s1 = torch.zeros(cols.shape[1])
    s2 = torch.zeros(cols.shape[1])
    for r in cols:  # raw moments, accumulated element by element in fp32
        s1 = s1 + r
        s2 = s2 + r * r
    m = torch.tensor(float(cols.shape[0]))
    raw = (s2 / m - (s1 / m) * (s1 / m)).reshape(c["B"], c["G"])
    n_raw, worst, _ = GB.violations(raw, c["s"]["var"], c["s"]["e_var"])
    print("raw moments: %d of %d (sample, group) variances outside the bound, worst %.1f x" % (n_raw, raw.numel(), worst))
    assert n_raw > raw.numel() // 2 and worst > 4, (n_raw, worst)


def test_one_element_groups_have_zero_variance_and_zero_bound():
    s = GB.case("one_elem")["s"]
    assert torch.equal(s["var"], torch.zeros_like(s["var"]))
    assert float(s["e_var"].max()) < 1e-10


def test_references_match_autograd():
    """forward_ref / backward_ref equal float64 autograd of the definition (and torch's group_norm)."""
    gen = torch.Generator().manual_seed(0)
    B, HW, C, G = 2, 5, 6, 3
    x = torch.randn(B, HW, C, generator=gen).to(torch.bfloat16)
    gy = torch.randn(B, HW, C, generator=gen).to(torch.bfloat16)
    slope, bias = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xd = x.double().requires_grad_()
    sd, bd = slope.double().requires_grad_(), bias.double().requires_grad_()
    xg = xd.reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xg - mean) / torch.sqrt(var + GB.EPS)).reshape(B, HW, C) * sd + bd
    y.backward(gy.double())
    ref, _, _ = GB.forward_ref(x, slope, bias, G, GB.EPS)
    assert torch.allclose(ref, y.detach(), rtol=1e-12, atol=1e-12)
    lib = torch.nn.functional.group_norm(x.double().permute(0, 2, 1), G, slope.double(), bias.double(), GB.EPS)
    assert torch.allclose(ref, lib.permute(0, 2, 1), rtol=1e-10, atol=1e-10)
    out = GB.backward_ref(gy, x, slope, torch.zeros(C), torch.zeros(C), G, GB.EPS)
    assert torch.allclose(out["dx"][0], xd.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(out["gslope"][0], sd.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(out["gbias"][0], bd.grad, rtol=1e-9, atol=1e-12)
