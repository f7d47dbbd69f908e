"""attention (csrc/kernels/attn_kernels.hip) through ops.layer_ops, element by element against
float64 computed from the same bf16 inputs.

Bound per element: 2^-8 |ref| (the output's rounding) + 2^-8 sum |a||b| over the product whose
operand the kernel rounds to bf16 (P for O and dV, dS for dQ and dK) + 4 times the largest error,
over the element's row, of the same formulas evaluated by torch in fp32 + 2^-126 (below bf16's
smallest normal the relative terms mean nothing).  The log-sum-exp is fp32 end to end: its bound is
2^-17 (1 + max_j sum_c |q_ic k_jc| / sqrt(d)), a d-term fp32 dot product (d 2^-24 <= 2^-18) doubled
for the log2e multiply and v_exp_f32 / v_log_f32.
Measured on an MI355X, worst d/bound over the ten cases: O 0.54, lse 0.04, dQ 0.98 (d = 32, T = 64),
dK 0.59, dV 0.55."""
import functools

import pytest
import torch

from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -8
B, NHEAD = 2, 3  # an odd head count: a wrong head offset lands on another head's columns


@functools.lru_cache(maxsize=None)
def _tokens(d):
    rows, keys = L.attn_tile(d)
    return (1, rows, rows + 1, 2 * keys + 3, 196)


def _case(T, d):
    """qkv [B T][3 C] and dO [B T][C], standard normal in bf16; from T = 3 on, per sample and head:
    query 0 scaled by 8 with its match q / 2 as the LAST key (the running max moves in the final
    chunk, logits in the hundreds), query 1 all zeros (uniform probabilities), key 1 all zeros."""
    gen = torch.Generator().manual_seed(T * 100 + d)
    x = torch.randn(B, T, 3, NHEAD, d, generator=gen)
    if T >= 3:
        x[:, 0, 0] *= 8.0
        x[:, 1, 0] = 0.0
        x[:, 1, 1] = 0.0
        x[:, T - 1, 1] = x[:, 0, 0] / 2
    g = torch.randn(B * T, NHEAD * d, generator=gen)
    return x.reshape(B * T, 3 * NHEAD * d).to(torch.bfloat16), g.to(torch.bfloat16)


def _eval(qkv, g, T, d, dt):
    """the layer's formulas in dtype dt: O, lse, dQ, dK, dV as [B, nhead, T, .] and, per output, the
    sum |a||b| of the product whose operand the kernel rounds; plus the lse's magnitude term"""
    x = qkv.to(dt).view(B, T, 3, NHEAD, d).permute(2, 0, 3, 1, 4)
    q, k, v = x[0], x[1], x[2]
    do = g.to(dt).view(B, T, NHEAD, d).permute(0, 2, 1, 3)
    sc = 1.0 / d ** 0.5
    s = q @ k.transpose(-1, -2) * sc
    lse = torch.logsumexp(s, -1, keepdim=True)
    p = torch.exp(s - lse)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    outs = dict(O=p @ v, dQ=ds @ k * sc, dK=ds.transpose(-1, -2) @ q * sc, dV=p.transpose(-1, -2) @ do)
    mags = dict(O=p @ v.abs(), dQ=ds.abs() @ k.abs() * sc, dK=ds.abs().transpose(-1, -2) @ q.abs() * sc,
                dV=p.transpose(-1, -2) @ do.abs())
    return outs, mags, lse.squeeze(-1), (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) * sc


def _rows(t):  # [B, nhead, T, d] -> [B T][C]
    return t.permute(0, 2, 1, 3).reshape(t.shape[0] * t.shape[2], -1)


def _check(got, name, ref, f32):
    r, m, e = _rows(ref[0][name]), _rows(ref[1][name]), (_rows(f32[0][name]).double() - _rows(ref[0][name])).abs()
    bound = U * r.abs() + U * m + 4 * e.amax(-1, keepdim=True) + 2.0 ** -126
    dist = (got.double().cpu() - r).abs()
    assert bool(torch.isfinite(got).all()), name + ": non-finite output"
    print("%s: worst d/bound %.3f" % (name, float((dist / bound).max())))
    bad = ~(dist <= bound)
    assert not bool(bad.any()), "%s: %d outside the bound, first at %s" % (name, int(bad.sum()), torch.nonzero(bad)[0].tolist())


@pytest.mark.parametrize("which", range(5), ids=["one", "tile", "tile-plus-one", "two-chunks-plus-three", "t196"])
@pytest.mark.parametrize("d", [32, 64])
def test_attention(d, which):
    T, C = _tokens(d)[which], NHEAD * d
    qkv, g = _case(T, d)
    ref, f32 = _eval(qkv, g, T, d, torch.float64), _eval(qkv, g, T, d, torch.float32)
    st = L.AttnState(B, T, C, NHEAD, DEV)
    xd, gd = qkv.to(DEV), g.to(DEV)
    out = torch.empty_like(gd)
    L.attn_forward(xd, out, B, NHEAD, st)
    _check(out, "O", ref, f32)
    lse = st.lse.view(B, NHEAD, T).double().cpu()
    dl = (lse - ref[2]).abs() / (2.0 ** -17 * (1 + ref[3]))
    print("lse: worst d/bound %.3f" % float(dl.max()))
    assert bool(torch.isfinite(lse).all()) and float(dl.max()) <= 1.0
    runs = []
    for prop in (True, True, False):
        dx = torch.full_like(xd, -3.0)
        L.attn_backward(gd, xd, dx, B, NHEAD, st, prop)
        if prop:
            runs.append(dx.cpu())
        else:
            assert bool((dx == -3.0).all()), "prop_grad false wrote the gradient"
    for s, name in enumerate(("dQ", "dK", "dV")):
        _check(runs[0][:, s * C:(s + 1) * C], name, ref, f32)
    assert torch.equal(runs[0], runs[1]), "two backward runs differ"
    inplace = xd.clone()
    L.attn_backward(gd, inplace, inplace, B, NHEAD, st, True)
    assert torch.equal(inplace.cpu(), runs[0]), "the in-place gradient differs from the out-of-place one"
