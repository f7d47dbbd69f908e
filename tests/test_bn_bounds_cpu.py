"""tests/bn_bounds.py on the CPU: the variance bound separates the schemes it is meant to separate.
On case c of the kernel tests (64 + 0.5 k, mean / std ~ 50) an fp32 emulation of the raw-moment
formula E[x^2] - E[x]^2 violates it, while the partial (count, mean, M2) merge scheme the kernels
use stays inside it -- evaluated in float64 (the reference of the scheme) and in fp32 (what the
kernel's arithmetic can reach)."""
import numpy as np
import torch

import bn_bounds as B


def _merge(na, ma, qa, nb, mb, qb, dt):
    n = na + nb
    f = dt(nb) / dt(n)
    d = mb - ma
    return n, ma + d * f, qa + qb + d * d * dt(na) * f


def _merge_scheme(x, lanes, dt):
    """Welford per row lane (rows lane, lane + lanes, ...), then a pairwise tree over the lanes:
    the block scheme of bn_ma_stats, in precision dt."""
    parts = []
    for l in range(lanes):
        rows = x[l::lanes]
        n, mean, m2 = 0, np.zeros(x.shape[1], dt), np.zeros(x.shape[1], dt)
        for r in rows:
            n += 1
            d = r - mean
            mean = mean + d * (dt(1) / dt(n))
            m2 = m2 + d * (r - mean)
        parts.append((n, mean, m2))
    while len(parts) > 1:
        s = 1
        while s < len(parts):
            s <<= 1
        s >>= 1
        for i in range(len(parts) - s):
            parts[i] = _merge(*parts[i], *parts[i + s], dt)
        parts = parts[:s]
    n, mean, m2 = parts[0]
    return mean, m2 / dt(n)


def test_raw_moments_violate_the_variance_bound_and_the_merge_scheme_does_not():
    xb = B.case_c_inputs()
    s = B.stats_ref(xb)
    x32 = xb.float().numpy()
    # raw moments, accumulated row by row in fp32
    s1 = np.zeros(x32.shape[1], np.float32)
    s2 = np.zeros(x32.shape[1], np.float32)
    for r in x32:
        s1 = s1 + r
        s2 = s2 + r * r
    R = np.float32(x32.shape[0])
    raw = s2 / R - (s1 / R) * (s1 / R)
    n_raw, worst_raw, _ = B.violations(torch.from_numpy(raw.astype(np.float64)), s["var"], s["e_var"])
    # (41 of the 64 channels; the worst errs by 7.5e-4, 7.9 x the bound, of which the summation
    # term g(R) var is 3e-5 and the propagated mean error the rest)
    assert n_raw > x32.shape[1] // 2 and worst_raw > 4, (n_raw, worst_raw)

    for dt in (np.float64, np.float32):
        mean, var = _merge_scheme(x32.astype(dt), 32, dt)
        B.assert_within(torch.from_numpy(var.astype(np.float64)), s["var"], s["e_var"], "var %s" % dt.__name__, axes="c")
        B.assert_within(torch.from_numpy(mean.astype(np.float64)), s["mean"], s["e_mean"], "mean %s" % dt.__name__,
                        axes="c")


def test_reference_matches_autograd():
    """backward_ref's closed form equals float64 autograd of the forward formula."""
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(12, 5, generator=gen).to(torch.bfloat16)
    gy = torch.randn(12, 5, generator=gen).to(torch.bfloat16)
    slope, bias = torch.rand(5, generator=gen) + 0.5, torch.randn(5, generator=gen)
    eps = 1e-5
    xd = x.double().requires_grad_()
    sd, bd = slope.double().requires_grad_(), bias.double().requires_grad_()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    y = (xd - mean) / torch.sqrt(var + eps) * sd + bd
    y.backward(gy.double())
    ref, _, _ = B.forward_ref(x, slope, bias, eps)
    assert torch.allclose(ref, y.detach(), rtol=1e-12, atol=1e-12)
    out = B.backward_ref(gy, x, slope, torch.zeros(5), torch.zeros(5), eps)
    assert torch.allclose(out["dx"][0], xd.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(out["gslope"][0], sd.grad, rtol=1e-9, atol=1e-12)
    assert torch.allclose(out["gbias"][0], bd.grad, rtol=1e-9, atol=1e-12)
