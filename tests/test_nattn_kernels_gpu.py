"""neighborhood_attention (csrc/kernels/nattn_kernels.hip) through ops.layer_ops, element by element
against float64 computed from the same bf16 inputs in the dense masked formulation of
test_nattn_cpu (per-query key lists built from the clamped definition).

Bounds: those of test_attn_kernels_gpu.py as test_wattn_kernels_gpu.py uses them -- O, dQ, dK, dV:
2^-8 |ref| + 2^-8 sum |a||b| over the product whose operand the kernel rounds to bf16 + 4 times the
largest fp32-torch error of the element's row + 2^-126; lse: 2^-17 (1 + max_j sum_c |q_ic k_jc| /
sqrt(d)) over the attended keys + 2^-23 |bias|max; gbias, per entry: n 2^-24 sum |dS_ij| over its n
terms + 4 times the largest error of the same formula in torch fp32.  The fp32 torch evaluation
(the layer's own torch path on the CPU, on these inputs) stays inside them: O, dQ, dK, dV and gbias
by construction, its own error entering them four times, at most 0.03 and 0.16 of the bound; the
lse bound has no such term, and there the fp32 path measured 0.03 of it at worst.
Measured on an MI355X, worst d/bound over the five cases: O 0.71, lse 0.06, dQ 0.80, dK 0.82 (k = 5),
dV 0.79, gbias 0.16; the hot case: O 0.62, dQ 0.74, dK 0.85, dV 0.72."""
import pytest
import torch

from cxxnet_amd.ops import layer_ops as L
from test_nattn_cpu import B, C, CASES, D, NHEAD, nat_dense, neighbourhood

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -8


def _case(H, W, k, hot, B=B, exact=True):
    """qkv [B H W][3 C], dO [B H W][C], standard normal in bf16, and the bias table, normal x 2.  Per
    sample and head, as in test_wattn_kernels_gpu.py: the query of pixel (0, 0) scaled by 8 with its
    match q / 2 as the key of pixel (k - 1, k - 1), the last of its neighbourhood (the exact case: sum
    1, P = 1, dS = 0), and the query of pixel (0, 1) all zeros.  hot: v of the pixels in columns
    x >= 12 and dO of the pixels in columns x >= 12 are 1e4.  exact False: no such rows, all normal."""
    gen = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(B, H, W, 3, NHEAD, D, generator=gen)
    if exact:
        x[:, 0, 0, 0] *= 8.0
        x[:, 0, 1, 0] = 0.0
        x[:, k - 1, k - 1, 1] = x[:, 0, 0, 0] / 2
    g = torch.randn(B, H, W, C, generator=gen)
    if hot:
        x[:, :, 12:, 2] = 1e4
        g[:, :, 12:] = 1e4
    bias = torch.randn(NHEAD, (2 * k - 1) ** 2, generator=gen) * 2
    return x.reshape(-1, 3 * C).to(torch.bfloat16), g.reshape(-1, C).to(torch.bfloat16), bias


def _eval(qkv, g, bias, geom, dt):
    """the layer's formulas in dtype dt as map rows: O, dQ, dK, dV [B H W][C] and, per output, the
    sum |a||b| of the product whose operand the kernel rounds; lse and its magnitude term
    [B, nhead, H W]; gbias, the sum of |dS| and the number of terms of every entry"""
    H, W, k = geom
    B = qkv.shape[0] // (H * W)
    q, kk, v, s = nat_dense(qkv.to(dt).view(B, H * W, 3 * C), bias.to(dt), H, W, k, NHEAD)
    do = g.to(dt).view(B, H * W, NHEAD, D).permute(0, 2, 1, 3)
    sc = 1.0 / D ** 0.5
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    outs = dict(O=p @ v, dQ=ds @ kk * sc, dK=ds.transpose(-1, -2) @ q * sc, dV=p.transpose(-1, -2) @ do)
    mags = dict(O=p @ v.abs(), dQ=ds.abs() @ kk.abs() * sc, dK=ds.abs().transpose(-1, -2) @ q.abs() * sc,
                dV=p.transpose(-1, -2) @ do.abs())
    lmag = (q.abs() @ kk.abs().transpose(-1, -2)).masked_fill(torch.isinf(s), 0).amax(-1, keepdim=True) * sc
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(B * H * W, -1)
    keys, rel = neighbourhood(H, W, k)
    near = ds.gather(3, keys.expand(B, NHEAD, -1, -1)).sum(0).reshape(NHEAD, -1), \
        ds.abs().gather(3, keys.expand(B, NHEAD, -1, -1)).sum(0).reshape(NHEAD, -1), \
        torch.full((NHEAD, keys.numel()), float(B), dtype=dt)
    gb = [torch.zeros(NHEAD, bias.shape[1], dtype=dt).index_add_(1, rel.reshape(-1), t) for t in near]
    return {k_: rows(t) for k_, t in outs.items()}, {k_: rows(t) for k_, t in mags.items()}, lse[..., 0], lmag[..., 0], gb


def _check(got, name, ref, f32, keep=None):
    r, m, e = ref[0][name], ref[1][name], (f32[0][name].double() - ref[0][name]).abs()
    bound = U * r.abs() + U * m + 4 * e.amax(-1, keepdim=True) + 2.0 ** -126
    got = got.double().cpu()
    dist = (got - r).abs()
    if keep is not None:
        got, dist, bound = got[keep], dist[keep], bound[keep]
    assert bool(torch.isfinite(got).all()), name + ": non-finite output"
    print("%s: worst d/bound %.3f" % (name, float((dist / bound).max())))
    bad = ~(dist <= bound)
    assert not bool(bad.any()), "%s: %d outside the bound, first at %s" % (name, int(bad.sum()), torch.nonzero(bad)[0].tolist())


@pytest.mark.parametrize("geom,hot", [(c, False) for c in CASES] + [(CASES[2], True)],
                         ids=["7x7-k7-one-neighbourhood", "9x10-k7-no-interior", "22x17-k7", "12x11-k5", "8x8-k3",
                              "22x17-k7-hot-far-columns"])
def test_neighborhood_attention(geom, hot):
    H, W, k = geom
    qkv, g, bias = _case(*geom, hot)
    ref, f32 = _eval(qkv, g, bias, geom, torch.float64), _eval(qkv, g, bias, geom, torch.float32)
    st = L.NAttnState(B, H, W, C, NHEAD, k, DEV)
    xd, gd, bd = qkv.to(DEV), g.to(DEV), bias.to(DEV)
    keep = (torch.arange(W) <= 8).repeat(B * H) if hot else None  # hot: the pixels whose pairs are all cool
    out = torch.empty_like(gd)
    L.nattn_forward(xd, out, bd, B, NHEAD, st)
    _check(out, "O", ref, f32, keep)
    runs = []
    for prop in (True, True, False):
        dx, gb = torch.full_like(xd, -3.0), torch.zeros_like(bd)
        L.nattn_backward(gd, xd, dx, bd, gb, B, NHEAD, st, prop)
        runs.append((dx.cpu(), gb.cpu()))
    for s, name in enumerate(("dQ", "dK", "dV")):
        _check(runs[0][0][:, s * C:(s + 1) * C], name, ref, f32, keep)
    if hot:
        return
    lse = st.lse.view(B, NHEAD, H * W).double().cpu()
    dl = (lse - ref[2]).abs() / (2.0 ** -17 * (1 + ref[3]) + 2.0 ** -23 * float(bias.abs().max()))
    print("lse: worst d/bound %.3f" % float(dl.max()))
    assert bool(torch.isfinite(lse).all()) and float(dl.max()) <= 1.0
    gbias, gabs, terms = ref[4]
    bound = terms * 2.0 ** -24 * gabs + 4 * float((f32[4][0].double() - gbias).abs().max())
    dgb = (runs[0][1].double() - gbias).abs() / bound
    print("gbias: worst d/bound %.3f" % float(dgb.max()))
    assert float(dgb.max()) <= 1.0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    assert bool((runs[2][0] == -3.0).all()), "prop_grad false wrote the gradient"
    assert torch.equal(runs[2][1], runs[0][1]), "prop_grad false: another bias gradient"
    inplace, gb = xd.clone(), torch.zeros_like(bd)
    L.nattn_backward(gd, inplace, inplace, bd, gb, B, NHEAD, st, True)
    assert torch.equal(inplace.cpu(), runs[0][0]) and torch.equal(gb.cpu(), runs[0][1]), \
        "the in-place gradient differs from the out-of-place one"


def test_backward_at_a_smaller_batch_than_the_state():
    """A state serves every batch up to the one it was sized for, and a smaller batch can need MORE
    bias-gradient slabs: 8 x 8 at k = 3 is one patch per sample, and at 2 heads the query orientation
    cuts at most 384 runs, so batch 512 walks 256 runs of 2 patches and batch 384 walks 384 runs of 1.
    Both run on a state sized for 512, the smaller first, against the same bounds (this is also the
    one case here in which a block walks more than one patch).  The inputs are plain normal draws: the
    dominant-key row of _case is exact only while every other key's exp underflows to 0 in fp32, a
    margin above 104, and the logit of the match is 5.66 |q|^2 with |q|^2 chi-squared of 32 -- over
    the 768 (sample, head) draws here a fifth fall short of that (the least margin is 70), and a
    probability near 2^-126 is then flushed or not, for which the bound has the one 2^-126 and a sum
    over 9 keys needs more.  The parametrised cases keep that row; their margins are above 100.
    Measured on an MI355X, worst d/bound over both batches: O 0.84, dQ 0.90, dK 0.92, dV 0.93, gbias 0.001."""
    geom = H, W, k = 8, 8, 3
    st = L.NAttnState(512, H, W, C, NHEAD, k, DEV)
    for nb in (384, 512):
        qkv, g, bias = _case(*geom, False, nb, exact=False)
        ref, f32 = _eval(qkv, g, bias, geom, torch.float64), _eval(qkv, g, bias, geom, torch.float32)
        xd, gd, bd = qkv.to(DEV), g.to(DEV), bias.to(DEV)
        out, dx, gb = torch.empty_like(gd), torch.empty_like(xd), torch.zeros_like(bd)
        L.nattn_forward(xd, out, bd, nb, NHEAD, st)
        L.nattn_backward(gd, xd, dx, bd, gb, nb, NHEAD, st, True)
        _check(out, "O", ref, f32)
        for s, name in enumerate(("dQ", "dK", "dV")):
            _check(dx[:, s * C:(s + 1) * C], name, ref, f32)
        gbias, gabs, terms = ref[4]
        bound = terms * 2.0 ** -24 * gabs + 4 * float((f32[4][0].double() - gbias).abs().max())
        dgb = (gb.double().cpu() - gbias).abs() / bound
        print("batch %d gbias: worst d/bound %.3f" % (nb, float(dgb.max())))
        assert float(dgb.max()) <= 1.0
