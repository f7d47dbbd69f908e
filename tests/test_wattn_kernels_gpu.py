"""window_attention (csrc/kernels/wattn_kernels.hip) through ops.layer_ops, element by element
against float64 computed from the same bf16 inputs in Swin's formulation (test_wattn_cpu).

Bounds.  O, dQ, dK, dV and the log-sum-exp: those of test_attn_kernels_gpu.py, derived there --
2^-8 |ref| + 2^-8 sum |a||b| over the product whose operand the kernel rounds to bf16 + 4 times the
largest fp32-torch error of the element's row + 2^-126; lse 2^-17 (1 + max_j sum_c |q_ic k_jc| /
sqrt(d)) over the attended keys, plus 2^-23 |bias|max for the fp32 bias (one rounding of bias log2e,
one of the sum).  gbias, per entry: n 2^-24 sum |dS_ij| over its n terms (a fixed-order fp32 sum)
+ 4 times the largest error of the same formula in torch fp32.
Measured on an MI355X, worst d/bound over the four cases: O 0.74, lse 0.05, dQ 0.87 (ws = 4),
dK 0.83, dV 0.83, gbias 0.20; the hot case: O 0.63, dQ 0.81."""
import pytest
import torch

from cxxnet_amd.ops import layer_ops as L
from test_wattn_cpu import B, CASES, D, NHEAD, heads_to_map, swin_logits, unwindows, windows

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -8
C = NHEAD * D


def _case(H, W, ws, shift, hot):
    """qkv [B H W][3 C], dO [B H W][C], standard normal in bf16, and the bias table, normal x 2.  Per
    sample, window and head, as in test_attn_kernels_gpu.py: the query of token 0 scaled by 8 with
    its match q / 2 as the key of the window's LAST token, the query of token 1 all zeros.  Where the
    mask lets that query see its match the logit is in the hundreds, every other key's exp2
    underflows against it and the row is the exact case (sum 1, P = 1, dS = 0); a match that merely
    dominates (a first draft had q / 8, logit about 45) leaves dS as a cancellation at the rounding
    of the log-sum-exp, ulp(lse) |dP|, for which the bound has no term and which the fp32 torch
    evaluation suffers just the same -- that draft measured dQ at 12.7 bounds on one row at ws = 4.
    hot: the v and dO rows of every token that wraps round the map (y < shift or x < shift) are 1e4."""
    gen = torch.Generator().manual_seed(H * 100 + W)
    n = ws * ws
    xw = torch.randn(B, (H // ws) * (W // ws), n, 3, NHEAD, D, generator=gen)
    xw[:, :, 0, 0] *= 8.0
    xw[:, :, 1, 0] = 0.0
    xw[:, :, n - 1, 1] = xw[:, :, 0, 0] / 2
    x = unwindows(xw.reshape(B, -1, n, 3 * C), H, W, ws, shift)
    g = torch.randn(B, H, W, C, generator=gen)
    if hot:
        for t in (x[..., 2 * C:], g):
            t[:, :shift] = 1e4
            t[:, :, :shift] = 1e4
    bias = torch.randn(NHEAD, (2 * ws - 1) ** 2, generator=gen) * 2
    return x.reshape(-1, 3 * C).to(torch.bfloat16), g.reshape(-1, C).to(torch.bfloat16), bias


def _eval(qkv, g, bias, geom, dt):
    """the layer's formulas in dtype dt as map rows: O, dQ, dK, dV [B H W][C] and, per output, the
    sum |a||b| of the product whose operand the kernel rounds; lse and its magnitude term
    [B, nhead, H W]; gbias, the sum of |dS| and the number of terms of every entry"""
    H, W, ws, shift = geom
    q, k, v, s, table = swin_logits(qkv.to(dt).view(B, H, W, 3 * C), bias.to(dt), *geom, NHEAD)
    do = windows(g.to(dt).view(B, H, W, C), *geom).view(B, -1, ws * ws, NHEAD, D).permute(0, 1, 3, 2, 4)
    sc = 1.0 / D ** 0.5
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    outs = dict(O=p @ v, dQ=ds @ k * sc, dK=ds.transpose(-1, -2) @ q * sc, dV=p.transpose(-1, -2) @ do)
    mags = dict(O=p @ v.abs(), dQ=ds.abs() @ k.abs() * sc, dK=ds.abs().transpose(-1, -2) @ q.abs() * sc,
                dV=p.transpose(-1, -2) @ do.abs())
    lmag = (q.abs() @ k.abs().transpose(-1, -2)).masked_fill(torch.isinf(s), 0).amax(-1, keepdim=True) * sc
    rows = lambda t: heads_to_map(t, *geom).reshape(B * H * W, -1)
    stat = lambda t: heads_to_map(t, *geom).reshape(B, H * W, NHEAD).permute(0, 2, 1)
    gb = [torch.zeros(NHEAD, bias.shape[1], dtype=dt).index_add_(1, table.reshape(-1), t.sum((0, 1)).reshape(NHEAD, -1))
          for t in (ds, ds.abs(), torch.ones_like(ds))]
    return {k_: rows(t) for k_, t in outs.items()}, {k_: rows(t) for k_, t in mags.items()}, stat(lse), stat(lmag), gb


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


@pytest.mark.parametrize("geom,hot", [(c, False) for c in CASES] + [(CASES[0], True)],
                         ids=["ws7-partial-tile", "ws8-full-tile", "ws4", "ws2", "ws7-hot-wrapped-rows"])
def test_window_attention(geom, hot):
    H, W, ws, shift = geom
    qkv, g, bias = _case(*geom, hot)
    ref, f32 = _eval(qkv, g, bias, geom, torch.float64), _eval(qkv, g, bias, geom, torch.float32)
    st = L.WAttnState(B, H, W, C, NHEAD, ws, shift, DEV)
    xd, gd, bd = qkv.to(DEV), g.to(DEV), bias.to(DEV)
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    keep = ((ys >= shift) & (xs >= shift)).reshape(-1).repeat(B) if hot else None  # hot: the unwrapped rows
    out = torch.empty_like(gd)
    L.wattn_forward(xd, out, bd, B, NHEAD, st)
    _check(out, "O", ref, f32, keep)
    runs = []
    for prop in (True, True, False):
        dx, gb = torch.full_like(xd, -3.0), torch.zeros_like(bd)
        L.wattn_backward(gd, xd, dx, bd, gb, B, NHEAD, st, prop)
        runs.append((dx.cpu(), gb.cpu()))
    _check(runs[0][0][:, :C], "dQ", ref, f32, keep)
    if hot:
        return
    lse = st.lse.view(B, NHEAD, H * W).double().cpu()
    dl = (lse - ref[2]).abs() / (2.0 ** -17 * (1 + ref[3]) + 2.0 ** -23 * float(bias.abs().max()))
    print("lse: worst d/bound %.3f" % float(dl.max()))
    assert bool(torch.isfinite(lse).all()) and float(dl.max()) <= 1.0
    for s, name in enumerate(("dK", "dV"), 1):
        _check(runs[0][0][:, s * C:(s + 1) * C], name, ref, f32)
    gbias, gabs, terms = ref[4]
    bound = terms * 2.0 ** -24 * gabs + 4 * float((f32[4][0].double() - gbias).abs().max())
    dgb = (runs[0][1].double() - gbias).abs() / bound
    print("gbias: worst d/bound %.3f" % float(dgb.max()))
    assert float(dgb.max()) <= 1.0
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    assert bool((runs[2][0] == -3.0).all()), "prop_grad false wrote the gradient"
    assert torch.equal(runs[2][1], runs[0][1]), "prop_grad false: another bias gradient"
    inplace, gb = xd.clone(), torch.zeros_like(bd)
    L.wattn_backward(gd, inplace, inplace, bd, gb, B, NHEAD, st, True)
    assert torch.equal(inplace.cpu(), runs[0][0]) and torch.equal(gb.cpu(), runs[0][1]), \
        "the in-place gradient differs from the out-of-place one"
