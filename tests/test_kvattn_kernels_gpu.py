"""kv_attention (csrc/kernels/kvattn_kernels.hip) through ops.layer_ops, element by element against
float64 computed from the same bf16 inputs.

Bound per element, as in test_attn_kernels_gpu.py: 2^-8 |ref| (the output's rounding) + 2^-8 sum
|a||b| over the product whose operand the kernel rounds to bf16 (P for O and dV, dS for dQ and dK)
+ 4 times the largest error, over the element's row, of the same formulas evaluated by torch in
fp32 + 2^-126.  The log-sum-exp is fp32 end to end: 2^-17 (1 + max_j sum_c |q_ic k_jc| / sqrt(d)).
Measured on an MI355X, worst d/bound over the ten cases: O 0.58, lse 0.03, dQ 0.88 (d = 32, two splits,
Tk = 17), dK 0.66, dV 0.58."""
import functools

import pytest
import torch

from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -8
B, NHEAD = 2, 3  # an odd head count: a wrong head offset lands on another head's columns


@functools.lru_cache(maxsize=None)
def _shapes(d):
    """(Tq, Tk): one query and key; a full tile against 64 keys; a tile plus one; the smallest Tq
    with two splits plus 3 against a partial 16-key tile; three tiles plus 5"""
    r = L.kvattn_tile(d, 1)[0]
    two = next(t for t in range(1, 16385, r) if L.kvattn_tile(d, t)[1] == 2)
    return ((1, 1), (r, 64), (r + 1, 49), (two + 3, 17), (3 * r + 5, 33))


def _case(Tq, Tk, d):
    """q [B Tq][C], kv [B Tk][2 C] and dO [B Tq][C], standard normal in bf16; where there is room,
    per sample and head: query 0 scaled by 8 with its match q / 2 as the LAST valid key (logits in
    the hundreds), query 1 all zeros (uniform probabilities), key 1 all zeros."""
    gen = torch.Generator().manual_seed(Tq * 100 + Tk + d)
    q = torch.randn(B, Tq, NHEAD, d, generator=gen)
    kv = torch.randn(B, Tk, 2, NHEAD, d, generator=gen)
    if Tq >= 2 and Tk >= 3:
        q[:, 0] *= 8.0
        q[:, 1] = 0.0
        kv[:, 1, 0] = 0.0
        kv[:, Tk - 1, 0] = q[:, 0] / 2
    g = torch.randn(B * Tq, NHEAD * d, generator=gen)
    return [t.to(torch.bfloat16) for t in (q.reshape(B * Tq, -1), kv.reshape(B * Tk, -1), g)]


def _eval(q, kv, g, d, dt, nb=B):
    """the layer's formulas in dtype dt: O, lse, dQ, dK, dV as [B, nhead, T, .] and, per output, the
    sum |a||b| of the product whose operand the kernel rounds; plus the lse's magnitude term"""
    q = q.to(dt).view(nb, -1, NHEAD, d).permute(0, 2, 1, 3)
    k, v = kv.to(dt).view(nb, -1, 2, NHEAD, d).permute(2, 0, 3, 1, 4)
    do = g.to(dt).view(nb, -1, NHEAD, d).permute(0, 2, 1, 3)
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


@pytest.mark.parametrize("which", range(5), ids=["one", "tile-64", "tile-plus-one-49", "two-splits-17", "three-tiles-33"])
@pytest.mark.parametrize("d", [32, 64])
def test_kv_attention(d, which):
    (Tq, Tk), C = _shapes(d)[which], NHEAD * d
    q, kv, g = _case(Tq, Tk, d)
    ref, f32 = _eval(q, kv, g, d, torch.float64), _eval(q, kv, g, d, torch.float32)
    st = L.KVAttnState(B, Tq, Tk, C, NHEAD, DEV)
    qd, kvd, gd = q.to(DEV), kv.to(DEV), g.to(DEV)
    out = torch.empty_like(gd)
    L.kvattn_forward(qd, kvd, out, B, NHEAD, st)
    _check(out, "O", ref, f32)
    lse = st.lse.view(B, NHEAD, Tq).double().cpu()
    dl = (lse - ref[2]).abs() / (2.0 ** -17 * (1 + ref[3]))
    print("lse: worst d/bound %.3f" % float(dl.max()))
    assert bool(torch.isfinite(lse).all()) and float(dl.max()) <= 1.0
    runs = []
    for prop in (True, True, False):
        dq, dkv = torch.full_like(qd, -3.0), torch.full_like(kvd, -3.0)
        L.kvattn_backward(gd, qd, kvd, dq, dkv, B, NHEAD, st, prop)
        if prop:
            runs.append((dq.cpu(), dkv.cpu()))
        else:
            assert bool((dq == -3.0).all()) and bool((dkv == -3.0).all()), "prop_grad false wrote a gradient"
    _check(runs[0][0], "dQ", ref, f32)
    _check(runs[0][1].view(B * Tk, 2, C)[:, 0], "dK", ref, f32)
    _check(runs[0][1].view(B * Tk, 2, C)[:, 1], "dV", ref, f32)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two backward runs differ"
    qi, kvi = qd.clone(), kvd.clone()
    L.kvattn_backward(gd, qi, kvi, qi, kvi, B, NHEAD, st, True)
    assert torch.equal(qi.cpu(), runs[0][0]) and torch.equal(kvi.cpu(), runs[0][1]), "in place differs from out of place"
    # the split does not depend on B: sample 1 alone, at batch 1, gives the same k / v gradient rows
    s1 = L.KVAttnState(1, Tq, Tk, C, NHEAD, DEV)
    q1, kv1, g1 = qd[Tq:].contiguous(), kvd[Tk:].contiguous(), gd[Tq:].contiguous()
    L.kvattn_forward(q1, kv1, torch.empty_like(g1), 1, NHEAD, s1)
    dq1, dkv1 = torch.empty_like(q1), torch.empty_like(kv1)
    L.kvattn_backward(g1, q1, kv1, dq1, dkv1, 1, NHEAD, s1, True)
    assert torch.equal(dkv1.cpu(), runs[0][1][Tk:]) and torch.equal(dq1.cpu(), runs[0][0][Tq:]), "batch 1 differs"
