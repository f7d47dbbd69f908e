"""layer_norm (csrc/kernels/ln_kernels.hip) and gelu (csrc/kernels/gelu_kernels.hip) through
ops.layer_ops, element by element against float64 computed from the same bf16 inputs.

Bound per element: half a bf16 ulp of the reference (2^-8 |ref|; outputs stored in fp32 -- gslope,
gbias -- have none) plus an fp32 term: 4 times the largest error, over the element's row (gelu: the tensor), of the same
formulas evaluated by torch in fp32 (ops.layer_ops' CPU path) against float64 on these inputs; the
4 covers another summation order.  Measured fp32 terms (before the factor 4), largest over the cases:
    layer_norm  y 1.8e-05   dx 7.5e-04 (the variance-0 row, rstd = 1000)   gslope 2.0e-05   gbias 4.8e-07
    gelu        y 3.0e-07   dx 2.6e-07
(each case computes its own at run time; these are for the reader)."""
import functools

import pytest
import torch

from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
U_BF16 = 2.0 ** -8
EPS = 1e-6


def _bound(ref, f32):
    """half a bf16 ulp of ref + 4 x the fp32 evaluation's largest error (layer_norm: over the element's
    row, so that the variance-0 row does not loosen the others; gelu: over the tensor)"""
    return U_BF16 * ref.abs() + 4 * (f32.double() - ref).abs().amax(-1, keepdim=True)


def _assert_within(got, ref, bound, what):
    d = (got.double().cpu() - ref).abs()
    assert bool(torch.isfinite(got).all()), what + ": non-finite output"
    bad = ~(d <= bound)
    print("%s: worst d/bound %.3f" % (what, float((d / bound).max())))
    assert not bool(bad.any()), "%s: %d outside the bound, first at %s" % (what, int(bad.sum()), torch.nonzero(bad)[0].tolist())


def _ln_case(rows, C):
    gen = torch.Generator().manual_seed(rows * 1000 + C)
    x = torch.randn(rows, C, generator=gen)
    if rows >= 3:
        x[1] = 3.0                                                       # variance 0
        x[2] = 100.0 + torch.randint(0, 3, (C,), generator=gen) * 0.5    # a large mean, a small spread
    g = torch.randn(rows, C, generator=gen)
    slope = 1.0 + 0.5 * torch.randn(C, generator=gen)
    bias = 0.1 * torch.randn(C, generator=gen)
    return x.to(torch.bfloat16), g.to(torch.bfloat16), slope, bias


def _ln_eval(x, g, slope, bias, dt):
    """(y, dx, gslope, gbias) onto zero gradients, the layer's formulas in dtype dt"""
    v, gv, s, b = x.to(dt), g.to(dt), slope.to(dt), bias.to(dt)
    C = v.shape[1]
    d = v - v.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + EPS)
    xh = d * rstd
    sg = gv * s
    dx = rstd * (sg - sg.sum(1, keepdim=True) / C - xh * (sg * xh).sum(1, keepdim=True) / C)
    return xh * s + b, dx, (gv * xh).sum(0), gv.sum(0)


@functools.lru_cache(maxsize=None)
def _rows_cases(C):
    return (1, 3, L.ln_rows_per_block(C) + 1)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["one-row", "three-rows", "block-plus-one"])
@pytest.mark.parametrize("C", [8, 20, 96, 768])
def test_layer_norm(C, which):
    rows = _rows_cases(C)[which]
    x, g, slope, bias = _ln_case(rows, C)
    ref, f32 = _ln_eval(x, g, slope, bias, torch.float64), _ln_eval(x, g, slope, bias, torch.float32)
    st = L.LNState(rows, C, DEV)
    xd, gd, sd, bd = x.to(DEV), g.to(DEV), slope.to(DEV), bias.to(DEV)
    y = torch.empty_like(xd)
    L.ln_forward(xd, y, sd, bd, EPS, st)
    _assert_within(y, ref[0], _bound(ref[0], f32[0]), "y")
    outs = []
    for prop in (True, True, False):
        dx = torch.full_like(xd, -3.0)
        gs, gb = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        L.ln_backward(gd, xd, dx, sd, gs, gb, st, prop)
        if prop:
            _assert_within(dx, ref[1], _bound(ref[1], f32[1]), "dx")
        else:
            assert bool((dx == -3.0).all()), "prop_grad false wrote dx"
        _assert_within(gs, ref[2], 4 * float((f32[2].double() - ref[2]).abs().max()) + 0 * ref[2], "gslope")
        _assert_within(gb, ref[3], 4 * float((f32[3].double() - ref[3]).abs().max()) + 0 * ref[3], "gbias")
        outs.append((gs.cpu(), gb.cpu()))
    assert all(torch.equal(outs[0][i], o[i]) for o in outs[1:] for i in (0, 1)), "parameter gradients differ between runs"


def _gelu_eval(x, g, dt):
    v, gv = x.to(dt), g.to(dt)
    cdf = 0.5 * torch.erfc(v * -0.7071067811865476)
    return v * cdf, gv * (cdf + v * 0.3989422804014327 * torch.exp(-0.5 * (v * v)))


def test_gelu():
    big = torch.finfo(torch.bfloat16).max
    x = torch.cat([torch.linspace(-40, 40, 8001), torch.linspace(-1.0, -0.5, 501),
                   torch.tensor([0.0, -0.0, big, -big, big / 2, -big / 2])]).to(torch.bfloat16)
    x = torch.cat([x, x[:2]])  # (n % 8 == 0: the vector path; the slice below takes the scalar one)
    g = torch.randn(x.numel(), generator=torch.Generator().manual_seed(7)).to(torch.bfloat16)
    for n in (x.numel(), x.numel() - 3):
        xs, gs = x[:n].contiguous(), g[:n].contiguous()
        ref, f32 = _gelu_eval(xs, gs, torch.float64), _gelu_eval(xs, gs, torch.float32)
        xd, gd = xs.to(DEV), gs.to(DEV)
        y, dx = torch.empty_like(xd), torch.empty_like(xd)
        L.gelu_forward(xd, y)
        L.gelu_backward(xd, gd, dx)
        _assert_within(y, ref[0], _bound(ref[0], f32[0]), "gelu y n=%d" % n)
        _assert_within(dx, ref[1], _bound(ref[1], f32[1]), "gelu dx n=%d" % n)
