"""The narrow-group kernels (csrc/kernels/gconv_kernels.hip) through gemm.conv_forward,
conv_backward_data and conv_backward_weight, element by element against the float64 references and
derived bounds of tests/bounds.py with groups = C / cg.  Dispatch keeps 32 channels per group on
the GEMM route (gemm.GC_ROUTED_WIDTHS); those cases call the kernels' own entry points.

A case is (N, C, cg, H, W, stride).  The kernels walk patches of R x 16 output pixels (R = 8 at
stride 1, 4 at stride 2; the stride-2 data gradient 16 x 32 pixels of dx): 19 x 20 at stride 1 is
3 x 2 patches with ragged last ones, 9 x 6 at stride 2 gives 5 output rows, two patch rows.  7 and 8
give the same 4 x 4 output at stride 2.  Every output is a view of a sentinel-filled buffer with one
more image and, in the slice cases, more channels on both sides (test_dwconv_kernels_gpu.py's)."""
import functools

import pytest
import torch

import bounds
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom
from test_dwconv_kernels_gpu import DEV, SENTINEL, _assert_guard, _guarded, _in, _out_slice, _rnd  # sentinel-guarded views

pytestmark = pytest.mark.gpu

GEOS = [(1, 1, 1), (2, 2, 1), (5, 7, 1), (19, 20, 1), (7, 7, 2), (8, 8, 2), (9, 6, 2)]  # (H, W, stride)
NCG = [(1, 16, 4), (3, 48, 4), (3, 48, 8), (2, 64, 16), (1, 128, 32), (2, 160, 32)]
CASES = [pytest.param(ncg + geo, id="n%dc%dg%d-%dx%d-s%d" % (ncg + geo)) for geo in GEOS for ncg in NCG]
SLICE_CASES = [pytest.param(c, id="n%dc%dg%d-%dx%d-s%d" % c)
               for c in [(3, 48, 4, 19, 20, 1), (2, 64, 16, 8, 8, 2), (2, 160, 32, 9, 6, 2)]]
# gconv_wgrad_partials: items = N ceil(Ho / R) ceil(Wo / 16), at most 512 // (C / (16 units)) slabs
SPLIT_CASE = (3, 48, 4, 19, 20, 1)  # 3 x 3 x 2 = 18 patches, three 16-channel slices: 18 slabs of one patch


def _geom(case):
    N, C, cg, H, W, S = case
    Ho, Wo = gemm.conv_out_size(H, W, 3, 3, S, 1, 1)
    return ConvGeom(N, H, W, C, Ho, Wo, C, 3, 3, S, 1, 1, C // cg)


@functools.lru_cache(maxsize=None)
def _operands(case):
    g = _geom(case)
    cg = g.C // g.groups
    x = _rnd((g.N, g.H, g.W, g.C), 1)
    w = _rnd((g.C, 3, 3, cg), 2, 0.3)
    b = torch.randn(g.C, generator=torch.Generator().manual_seed(3)) * 0.1
    dy = _rnd((g.N, g.Ho, g.Wo, g.C), 4)
    act = torch.relu(_rnd((g.N, g.H, g.W, g.C), 5))  # relu(z) of the node the data gradient is written to
    dw0 = torch.randn(g.C, 3, 3, cg, generator=torch.Generator().manual_seed(6))
    return x, w, b, dy, act, dw0


@functools.lru_cache(maxsize=None)
def _ref(case, what):
    g = _geom(case)
    x, w, b, dy, _, dw0 = _operands(case)
    kw = dict(stride=g.stride, pad=1, groups=g.groups)
    if what == "weight":
        return bounds.weight_grad_ref(x, dy, dw0, **kw)
    if what == "data":
        return bounds.data_grad_ref(dy, w, in_hw=(g.H, g.W), **kw)
    return bounds.forward_ref(x, w, b if what == "bias" else None, **kw)


def _fwd(x, w, b, y, g, relu):
    (gemm.conv_forward if gemm.gconv_served(g) else gemm.gconv_forward)(x, w, b, y, g, relu=relu)


def _bwd_data(dy, w, dx, g, mask):  # (conv_backward_data returns False: no bias-gradient epilogue)
    assert not (gemm.conv_backward_data if gemm.gconv_served(g) else gemm.gconv_backward_data)(dy, w, dx, g, mask_relu=mask)


def _bwd_weight(x, dy, dw, g):  # (likewise)
    assert not (gemm.conv_backward_weight if gemm.gconv_served(g) else gemm.gconv_backward_weight)(x, dy, dw, g)


def _check_forward(case, mode, sliced=False):
    g = _geom(case)
    x, w, b = _operands(case)[:3]
    bias, relu = mode != "nobias", mode == "bias_relu"
    ref, bound = _ref(case, "bias" if bias else "nobias")
    shape, (lo, extra) = (g.N, g.Ho, g.Wo, g.C), _out_slice(sliced)
    yb, y = _guarded(shape, lo, extra)
    _fwd(_in(x, sliced), w.to(DEV), b.to(DEV) if bias else None, y, g, relu)
    torch.cuda.synchronize()
    _assert_guard(yb, shape, lo)
    worst = bounds.assert_within(y.cpu(), ref.clamp_min(0) if relu else ref, bound, "forward %s %s" % (case, mode))
    print("forward %s %s: max d/bound %.3f" % (case, mode, worst))


def _check_data(case, mode, sliced=False):
    g = _geom(case)
    _, w, _, dy, act, _ = _operands(case)
    ref, bound = _ref(case, "data")
    shape, (lo, extra) = (g.N, g.H, g.W, g.C), _out_slice(sliced)
    dxb, dx = _guarded(shape, lo, extra, fill=act if mode == "mask" else None)
    _bwd_data(_in(dy, sliced), w.to(DEV), dx, g, mode == "mask")
    torch.cuda.synchronize()
    _assert_guard(dxb, shape, lo)
    got = dx.cpu()
    what = "data gradient %s %s" % (case, mode)
    if mode == "mask":
        m = act > 0
        assert bool((~m).any()) and torch.count_nonzero(got[~m]) == 0, what + ": a masked element is not 0"
        ref, bound = ref * m.double(), bound * m.double()
    worst = bounds.assert_within(got, ref, bound, what)
    print("%s: max d/bound %.3f" % (what, worst))


def _run_weight(case, sliced=False):
    g = _geom(case)
    x, _, _, dy, _, dw0 = _operands(case)
    dw = dw0.to(DEV).clone()
    _bwd_weight(_in(x, sliced), _in(dy, sliced), dw, g)
    torch.cuda.synchronize()
    return dw.cpu()


def _check_weight(case, sliced=False):
    ref, bound = _ref(case, "weight")
    worst = bounds.assert_within(_run_weight(case, sliced), ref, bound, "weight gradient %s" % (case,), axes="cklg")
    print("weight gradient %s: max d/bound %.3f" % (case, worst))


@pytest.mark.parametrize("mode", ["nobias", "bias", "bias_relu"])
@pytest.mark.parametrize("case", CASES)
def test_forward(case, mode):
    _check_forward(case, mode)


@pytest.mark.parametrize("mode", ["plain", "mask"])
@pytest.mark.parametrize("case", CASES)
def test_data_grad(case, mode):
    _check_data(case, mode)


@pytest.mark.parametrize("case", CASES)
def test_weight_grad(case):
    _check_weight(case)


@pytest.mark.parametrize("case", SLICE_CASES)
def test_channel_slices(case):
    _check_forward(case, "bias_relu", sliced=True)
    _check_data(case, "mask", sliced=True)
    _check_weight(case, sliced=True)


def test_weight_grad_split_is_bitwise_reproducible():
    assert gemm.gconv_wgrad_partials(_geom(SPLIT_CASE))[0] == 18  # more than one slab, and two merge lanes
    for g in (_geom(p.values[0]) for p in CASES):
        assert gemm.is_narrow_group(g) and gemm.gconv_served(g) == (g.C // g.groups != 32)
        assert g.N * g.Ho * g.Wo <= 1500  # weight_grad_ref's bound still catches one missing term
    a, b = _run_weight(SPLIT_CASE), _run_weight(SPLIT_CASE)
    try:
        gemm.set_deterministic(True)
        c = _run_weight(SPLIT_CASE)
    finally:
        gemm.set_deterministic(False)
    assert torch.equal(a, b) and torch.equal(a, c)


# (C, Cout, groups, K, pad): what the kernels decline keeps the outcome it had, with the path on or off
DECLINED = {"groups2": (32, 32, 2, 3, 1), "pad0": (32, 32, 4, 3, 0), "k5": (32, 32, 4, 5, 2),
            "c_ne_cout": (32, 64, 4, 3, 1), "cg12": (48, 48, 4, 3, 1)}


@pytest.mark.parametrize("name", list(DECLINED))
def test_declined_geometries_keep_their_route(name, monkeypatch):
    C, Cout, G, K, pad = DECLINED[name]
    H = 9
    Ho, _ = gemm.conv_out_size(H, H, K, K, 1, pad, pad)
    g = ConvGeom(2, H, H, C, Ho, Ho, Cout, K, K, 1, pad, pad, G)
    assert not gemm.gconv_served(g)
    x = _rnd((2, H, H, C), 1).to(DEV)
    w = _rnd((Cout, K, K, C // G), 2, 0.3).to(DEV)
    outs = []
    for on in (True, False):
        monkeypatch.setattr(gemm, "_GC", on)
        y = torch.full((2, Ho, Ho, Cout), SENTINEL, device=DEV, dtype=torch.bfloat16)
        gemm.conv_forward(x, w, None, y, g)
        outs.append(y.cpu())
    assert torch.equal(outs[0], outs[1])
    ref, bound = bounds.forward_ref(x.cpu(), w.cpu(), None, stride=1, pad=pad, groups=G)
    bounds.assert_within(outs[0], ref, bound, "declined %s" % name)
