"""The depthwise kernels (csrc/kernels/dwconv_kernels.hip) through the ops layer, element by element
against the float64 references and derived bounds of tests/bounds.py with groups = C: forward
(no bias / bias / bias + relu), data gradient (plain / relu'-masked) and weight gradient (onto a
non-zero dw0, with and without the bias gradient onto a non-zero init).  There are only K K taps,
so the forward and data-gradient bounds sit within a few percent of one bf16 rounding.

A case is (N, C, H, W, K, stride, pad_y, pad_x).  The geometries are the smallest places a defect
can hide: a non-square map, maps smaller than the kernel (almost every tap is padding), the two
input sizes 7 and 8 that give the same 4 x 4 output at stride 2 (the data gradient must fill row
and column 7 of the larger one), pad 0 at stride 2, unequal pads, both kernel sizes at both
strides and, at stride 2, both parities of pad_x (the data gradient's column forms).  C = 8 is
one 8-channel vector, 24 a vector count that is no power of two (85 item lanes, one lane idle),
136 = 17 vectors (15 item lanes).

Every output is a view of a sentinel-filled buffer with one more image and, in the slice cases,
more channels on both sides (pixel stride > C, the input a channel slice as well): nothing may be
written outside the view."""
import functools

import pytest
import torch

import bounds
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -3.0

# (H, W, K, stride, pad_y, pad_x)
GEOS = [
    (5, 7, 3, 1, 1, 1),    # non-square; two runs per row, the second ragged
    (1, 1, 3, 1, 1, 1),    # the map smaller than the kernel: one tap of nine is inside
    (2, 2, 3, 1, 1, 1),
    (7, 7, 3, 2, 1, 1),    # -> 4 x 4
    (8, 8, 3, 2, 1, 1),    # -> 4 x 4 as well: dx row / column 7 get the kh = kw = 0 taps only
    (9, 6, 3, 2, 0, 0),    # -> 4 x 2, pad 0 (even column parity), the last input column unused
    (6, 5, 3, 1, 1, 0),    # unequal pads -> 6 x 3
    (6, 6, 5, 1, 2, 2),
    (9, 9, 5, 2, 2, 2),    # -> 5 x 5
    (9, 8, 5, 2, 2, 1),    # -> 5 x 3, odd column parity at 5 x 5
]
NC = [(1, 8), (3, 24), (1, 136)]
CASES = [pytest.param((n, c) + geo, id="n%dc%d-%dx%d-k%ds%dp%d%d" % ((n, c) + geo)) for geo in GEOS for n, c in NC]
SLICE_CASES = [pytest.param((3, 24) + GEOS[i], id="n3c24-%dx%d-k%ds%dp%d%d" % GEOS[i]) for i in (0, 4, 9)]
# Weight-gradient reduction split, from the formula the Python side mirrors
# (gemm.dwconv_wgrad_partials): items R = N Ho ceil(Wo / 2) (runs of 2 pixels); a block takes
# ipb = max(ceil(R / 512), 4 RL) items, RL = 256 // (C / 8).  N Ho Wo = 1140 <= 1500.  The merge
# kernel gives each of its 16 lanes ceil(P / 16) consecutive slabs: one lane at P <= 1, ten at 10.
SPLIT_CASES = {
    (3, 24, 5, 7, 3, 1, 1, 1): 1,       # R = 60, RL = 85, ipb = 340: one slab
    (3, 136, 19, 20, 3, 1, 1, 1): 10,   # R = 570, RL = 15, ipb = 60: 9 slabs of 60 items and one of 30
    (3, 136, 19, 20, 5, 1, 2, 2): 10,   # the same split at 5 x 5
    (3, 136, 19, 20, 3, 2, 1, 1): 3,    # Ho x Wo = 10 x 10: R = 150: slabs of 60, 60 and 30
    (3, 512, 19, 20, 3, 1, 1, 1): 36,   # RL = 4, ipb = 16: 35 slabs of 16 and one of 10; 12 merge lanes of 3 slabs
}


def _geom(case):
    N, C, H, W, K, S, py, px = case
    Ho, Wo = gemm.conv_out_size(H, W, K, K, S, py, px)
    return ConvGeom(N, H, W, C, Ho, Wo, C, K, K, S, py, px, C)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


# operands (CPU) and float64 references, computed once per case and shared by the epilogues
@functools.lru_cache(maxsize=None)
def _operands(case):
    g = _geom(case)
    x = _rnd((g.N, g.H, g.W, g.C), 1)
    w = _rnd((g.C, g.KH, g.KW, 1), 2, 0.3)
    b = torch.randn(g.C, generator=torch.Generator().manual_seed(3)) * 0.1
    dy = _rnd((g.N, g.Ho, g.Wo, g.C), 4)
    act = torch.relu(_rnd((g.N, g.H, g.W, g.C), 5))  # relu(z) of the node the data gradient is written to
    dw0 = torch.randn(g.C, g.KH, g.KW, 1, generator=torch.Generator().manual_seed(6))
    return x, w, b, dy, act, dw0


@functools.lru_cache(maxsize=None)
def _forward_ref(case, bias):
    g = _geom(case)
    x, w, b = _operands(case)[:3]
    return bounds.forward_ref(x, w, b if bias else None, stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.C)


@functools.lru_cache(maxsize=None)
def _data_ref(case):
    g = _geom(case)
    _, w, _, dy, _, _ = _operands(case)
    return bounds.data_grad_ref(dy, w, stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.C, in_hw=(g.H, g.W))


@functools.lru_cache(maxsize=None)
def _weight_ref(case):
    g = _geom(case)
    x, _, _, dy, _, dw0 = _operands(case)
    return bounds.weight_grad_ref(x, dy, dw0, stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.C)


def _guarded(shape, lo=0, extra=0, fill=None):
    """(buffer, view): images [:N], channels [lo : lo + C] of a sentinel-filled buffer with one more
    image and `extra` more channels."""
    N, H, W, C = shape
    buf = torch.full((N + 1, H, W, C + extra), SENTINEL, device=DEV, dtype=torch.bfloat16)
    view = buf[:N, :, :, lo:lo + C]
    if fill is not None:
        view.copy_(fill.to(DEV))
    return buf, view


def _assert_guard(buf, view_shape, lo=0):
    N, C = view_shape[0], view_shape[3]
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[:N, :, :, lo:lo + C] = False
    touched = outside & (buf != SENTINEL)
    if bool(touched.any()):
        idx = torch.nonzero(touched)
        raise AssertionError("%d elements written outside the output view, first (n, h, w, c) = %s, last %s" % (
            idx.shape[0], idx[0].tolist(), idx[-1].tolist()))


def _sliced_input(t, lo, extra):
    g = torch.Generator().manual_seed(99)
    buf = torch.randn(*t.shape[:3], t.shape[3] + extra, generator=g).to(torch.bfloat16).to(DEV)
    buf[..., lo:lo + t.shape[3]] = t.to(DEV)
    return buf[..., lo:lo + t.shape[3]]


def _in(t, sliced):
    return _sliced_input(t, 8, 24) if sliced else t.to(DEV)


def _out_slice(sliced):
    return (16, 40) if sliced else (0, 0)  # (lo, extra): 24 sentinel channels behind the view


def _check_forward(case, mode, sliced=False):
    g = _geom(case)
    x, w, b = _operands(case)[:3]
    bias, relu = mode != "nobias", mode == "bias_relu"
    ref, bound = _forward_ref(case, bias)
    lo, extra = _out_slice(sliced)
    shape = (g.N, g.Ho, g.Wo, g.C)
    yb, y = _guarded(shape, lo, extra)
    gemm.conv_forward(_in(x, sliced), w.to(DEV), b.to(DEV) if bias else None, y, g, relu=relu)
    torch.cuda.synchronize()
    _assert_guard(yb, shape, lo)
    worst = bounds.assert_within(y.cpu(), ref.clamp_min(0) if relu else ref, bound, "forward %s %s" % (case, mode))
    print("forward %s %s%s: max d/bound %.3f" % (case, mode, " sliced" if sliced else "", worst))


def _check_data(case, mode, sliced=False):
    g = _geom(case)
    _, w, _, dy, act, _ = _operands(case)
    ref, bound = _data_ref(case)
    lo, extra = _out_slice(sliced)
    shape = (g.N, g.H, g.W, g.C)
    dxb, dx = _guarded(shape, lo, extra, fill=act if mode == "mask" else None)
    assert gemm.conv_backward_data(_in(dy, sliced), w.to(DEV), dx, g, mask_relu=mode == "mask") is False
    torch.cuda.synchronize()
    _assert_guard(dxb, shape, lo)
    got = dx.cpu()
    what = "data gradient %s %s" % (case, mode)
    if mode == "mask":
        m = act > 0
        assert bool((~m).any()) and torch.count_nonzero(got[~m]) == 0, what + ": a masked element is not 0"
        ref, bound = ref * m.double(), bound * m.double()
    worst = bounds.assert_within(got, ref, bound, what)
    print("%s%s: max d/bound %.3f" % (what, " sliced" if sliced else "", worst))


def _run_weight(case, with_db, sliced=False):
    g = _geom(case)
    x, _, _, dy, _, dw0 = _operands(case)
    dw = dw0.to(DEV).clone()
    db = torch.full((g.C,), 0.5, device=DEV) if with_db else None
    done = gemm.conv_backward_weight(_in(x, sliced), _in(dy, sliced), dw, g, db=db)
    torch.cuda.synchronize()
    assert done is with_db
    return dw.cpu(), db.cpu() if with_db else None


def _check_weight(case, with_db, sliced=False):
    dy = _operands(case)[3]
    ref, bound = _weight_ref(case)
    dw, db = _run_weight(case, with_db, sliced)
    what = "weight gradient %s db %d" % (case, with_db)
    worst = bounds.assert_within(dw, ref, bound, what, axes="ckl1")
    print("%s%s: max d/bound %.3f" % (what, " sliced" if sliced else "", worst))
    if with_db:
        dref, dbound = bounds.dbias_ref(dy, 0.5)
        worst = bounds.assert_within(db, dref, dbound, what + " dbias", axes="c")
        print("%s dbias: max d/bound %.3g" % (what, worst))


@pytest.mark.parametrize("mode", ["nobias", "bias", "bias_relu"])
@pytest.mark.parametrize("case", CASES)
def test_forward(case, mode):
    _check_forward(case, mode)


@pytest.mark.parametrize("mode", ["plain", "mask"])
@pytest.mark.parametrize("case", CASES)
def test_data_grad(case, mode):
    _check_data(case, mode)


@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_weight_grad(case, with_db):
    _check_weight(case, with_db)


@pytest.mark.parametrize("case", SLICE_CASES)
def test_channel_slices(case):
    """Every activation operand a channel slice of a wider buffer: inputs at channels 8.. of a
    buffer 24 wider, outputs at channels 16.. of a buffer 40 wider, one sentinel image after the
    last."""
    _check_forward(case, "bias_relu", sliced=True)
    _check_data(case, "mask", sliced=True)
    _check_weight(case, True, sliced=True)


def test_split_cases_split():
    assert {c: gemm.dwconv_wgrad_partials(_geom(c))[0] for c in SPLIT_CASES} == SPLIT_CASES
    for c in SPLIT_CASES:
        g = _geom(c)
        assert g.N * g.Ho * g.Wo <= 1500  # weight_grad_ref's bound still catches one missing term


@pytest.mark.parametrize("with_db", [False, True])
@pytest.mark.parametrize("case", [pytest.param(c, id="n%dc%d-%dx%d-k%ds%dp%d%d-P%d" % (c + (p,)))
                                  for c, p in SPLIT_CASES.items()])
def test_weight_grad_reduction_split(case, with_db):
    _check_weight(case, with_db)


def test_weight_grad_is_bitwise_reproducible():
    case = (3, 136, 19, 20, 3, 1, 1, 1)  # ten slabs
    a, b = _run_weight(case, True), _run_weight(case, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    try:
        gemm.set_deterministic(True)
        c = _run_weight(case, True)
    finally:
        gemm.set_deterministic(False)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


# (C, Cout, K, stride): a channel multiplier of 2, C no multiple of 8, 7 x 7, stride 3
@pytest.mark.parametrize("C,Cout,K,S", [(8, 16, 3, 1), (12, 12, 3, 1), (8, 8, 7, 1), (8, 8, 3, 3)],
                         ids=["multiplier2", "c12", "k7", "stride3"])
def test_unserved_depthwise_geometries_raise(C, Cout, K, S):
    H = 9
    Ho, _ = gemm.conv_out_size(H, H, K, K, S, K // 2, K // 2)
    g = ConvGeom(2, H, H, C, Ho, Ho, Cout, K, K, S, K // 2, K // 2, C)
    assert gemm.is_depthwise(g) and not gemm.dwconv_served(g)
    x = torch.zeros(2, H, H, C, device=DEV, dtype=torch.bfloat16)
    dy = torch.zeros(2, Ho, Ho, Cout, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(Cout, K, K, 1, device=DEV, dtype=torch.bfloat16)
    y = torch.full_like(dy, SENTINEL)
    dx = torch.full_like(x, SENTINEL)
    dw = torch.full((Cout, K, K, 1), SENTINEL, device=DEV)
    with pytest.raises(ValueError, match="served"):
        gemm.conv_forward(x, w, None, y, g)
    with pytest.raises(ValueError, match="served"):
        gemm.conv_backward_data(dy, w, dx, g)
    with pytest.raises(ValueError, match="served"):
        gemm.conv_backward_weight(x, dy, dw, g)
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((dx == SENTINEL).all()) and bool((dw == SENTINEL).all())
