"""The large-kernel depthwise kernels (csrc/kernels/dwconv_lk_kernels.hip) through ops.gemm.dwlk_*,
element by element against the float64 references and derived bounds of tests/bounds.py with
groups = C -- the bound test_dwconv_kernels_gpu.py applies at K = 3 / 5: half a bf16 ulp of the
reference plus the fp32 accumulation term over K K + 1 products (weight gradient: fp32 out, the
term count is the pixels summed, N Ho Wo <= 578 here).

A case is (N, C, H, W, K, pad_y, pad_x).  P = gemm.DWLK_PATCH (16) is the block patch; a map of at
most 8 x 8 takes the 8 x 8 patch with 16 channel groups per block, anything else 16 x 16 with 8."""
import functools

import pytest
import torch

import bounds
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -3.0
P = gemm.DWLK_PATCH

CASES = [
    (2, 8, 7, 7, 7, 3, 3),            # every output touches every border; the small patch, one lane group
    (2, 136, 7, 7, 7, 3, 3),          # the small patch, two channel blocks (16 + 1 groups)
    (2, 24, P + 1, P + 1, 7, 3, 3),   # two patches per axis, the second one pixel; a partial channel block
    (2, 24, P + 1, P + 1, 9, 4, 4),
    (2, 24, P + 1, P + 1, 11, 5, 5),
    (2, 24, P + 1, P + 4, 7, 3, 0),   # pad (3, 0) -> 17 x 14
    (2, 8, 12, 9, 7, 0, 0),           # pad (0, 0) -> 6 x 3, non-square
    (2, 136, 9, P + 1, 7, 3, 3),      # non-square, three channel blocks (8 + 8 + 1 groups)
]
IDS = ["n%dc%d-%dx%d-k%dp%d%d" % c for c in CASES]
SLICED = [CASES[1], CASES[2]]


def _geom(case):
    N, C, H, W, K, py, px = case
    Ho, Wo = gemm.conv_out_size(H, W, K, K, 1, py, px)
    return ConvGeom(N, H, W, C, Ho, Wo, C, K, K, 1, py, px, C)


def _rnd(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _operands(case):
    g = _geom(case)
    x = _rnd((g.N, g.H, g.W, g.C), 1)
    w = _rnd((g.C, g.KH, g.KW, 1), 2, 0.2)
    b = torch.randn(g.C, generator=torch.Generator().manual_seed(3)) * 0.1
    dy = _rnd((g.N, g.Ho, g.Wo, g.C), 4)
    act = torch.relu(_rnd((g.N, g.H, g.W, g.C), 5))  # relu(z) of the node the data gradient is written to
    dw0 = torch.randn(g.C, g.KH, g.KW, 1, generator=torch.Generator().manual_seed(6))
    return x, w, b, dy, act, dw0


@functools.lru_cache(maxsize=None)
def _refs(case):
    g = _geom(case)
    x, w, b, dy, _, dw0 = _operands(case)
    kw = dict(stride=1, pad=(g.pad_y, g.pad_x), groups=g.C)
    return (bounds.forward_ref(x, w, b, **kw), bounds.data_grad_ref(dy, w, in_hw=(g.H, g.W), **kw),
            bounds.weight_grad_ref(x, dy, dw0, **kw), bounds.dbias_ref(dy, 0.5))


def _in(t, sliced):
    """t on the device; sliced: channels 8 .. of a buffer 24 channels wider (pixel stride > C)"""
    if not sliced:
        return t.to(DEV)
    buf = _rnd(t.shape[:3] + (t.shape[3] + 24,), 99).to(DEV)
    buf[..., 8:8 + t.shape[3]] = t.to(DEV)
    return buf[..., 8:8 + t.shape[3]]


def _out(shape, sliced, fill=None):
    """(buffer, view) of a sentinel-filled buffer with one more image and, sliced, 16 + 24 more channels"""
    N, H, W, C = shape
    lo, extra = (16, 40) if sliced else (0, 0)
    buf = torch.full((N + 1, H, W, C + extra), SENTINEL, device=DEV, dtype=torch.bfloat16)
    view = buf[:N, :, :, lo:lo + C]
    if fill is not None:
        view.copy_(fill.to(DEV))
    return buf, view


def _assert_guard(buf, view):
    keep = buf.clone()
    view.fill_(SENTINEL)
    assert bool((buf == SENTINEL).all()), "written outside the output view"
    buf.copy_(keep)


def _check(case, sliced):
    g = _geom(case)
    x, w, b, dy, act, dw0 = _operands(case)
    (fref, fbound), (dref, dbound), (wref, wbound), (bref, bbound) = _refs(case)
    assert gemm.dwlk_served(g) and not gemm.dwconv_served(g)
    wd = w.to(DEV)
    # forward: bias + relu
    yb, y = _out((g.N, g.Ho, g.Wo, g.C), sliced)
    gemm.dwlk_forward(_in(x, sliced), wd, b.to(DEV), y, g, relu=True)
    got = y.cpu()
    _assert_guard(yb, y)
    print("forward d/bound %.3f" % bounds.assert_within(got, fref.clamp_min(0), fbound, "forward %s" % (case,)))
    # data gradient: plain, then relu'-masked
    for masked in (False, True):
        dxb, dx = _out((g.N, g.H, g.W, g.C), sliced, fill=act if masked else None)
        gemm.dwlk_backward_data(_in(dy, sliced), wd, dx, g, mask_relu=masked)
        got = dx.cpu()
        _assert_guard(dxb, dx)
        m = (act > 0).double() if masked else torch.ones_like(dref)
        assert not masked or torch.count_nonzero(got[act <= 0]) == 0
        print("dgrad d/bound %.3f" % bounds.assert_within(got, dref * m, dbound * m, "dgrad %s mask %d" % (case, masked)))
    # weight gradient onto a non-zero start, without and with db, twice: the same bits
    runs = []
    for with_db in (False, True, True):
        dw = dw0.to(DEV).clone()
        db = torch.full((g.C,), 0.5, device=DEV) if with_db else None
        gemm.dwlk_backward_weight(_in(x, sliced), _in(dy, sliced), dw, g, db=db)
        print("wgrad d/bound %.3f" % bounds.assert_within(dw.cpu(), wref, wbound, "wgrad %s" % (case,), axes="ckl1"))
        if with_db:
            bounds.assert_within(db.cpu(), bref, bbound, "dbias %s" % (case,), axes="c")
            runs.append((dw.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_directions(case):
    _check(case, sliced=False)


@pytest.mark.parametrize("case", SLICED, ids=["small", "big"])
def test_channel_slices(case):
    _check(case, sliced=True)


@pytest.mark.parametrize("N,H,slabs", [(1100, 7, 367), (260, P + 1, 347)], ids=["small", "big"])
def test_blocks_walk_several_patches(N, H, slabs):
    """1100 (small patch) / 1040 (big patch, 4 per image) patches for at most 1024 stencil blocks and
    512 weight-gradient slabs: blocks take a second patch (3 per slab).  Operands in {-1, 0, 1}:
    every sum is an integer fp32 and bf16 hold exactly, so all three results equal the float64 ones
    whatever the order."""
    g = _geom((N, 8, H, H, 7, 3, 3))
    assert gemm.dwlk_wgrad_partials(g)[0] == slabs
    gen = torch.Generator().manual_seed(11)
    x, dy = (torch.randint(-1, 2, (g.N, H, H, 8), generator=gen).to(torch.bfloat16) for _ in range(2))
    w = torch.randint(-1, 2, (8, 7, 7, 1), generator=gen).to(torch.bfloat16)
    kw = dict(stride=1, pad=(3, 3), groups=8)
    xd, dyd, wd = x.to(DEV), dy.to(DEV), w.to(DEV)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    dw, db = torch.zeros(8, 7, 7, 1, device=DEV), torch.zeros(8, device=DEV)
    gemm.dwlk_forward(xd, wd, None, y, g)
    gemm.dwlk_backward_data(dyd, wd, dx, g)
    gemm.dwlk_backward_weight(xd, dyd, dw, g, db=db)
    assert torch.equal(y.cpu().double(), bounds.forward_ref(x, w, None, **kw)[0])
    assert torch.equal(dx.cpu().double(), bounds.data_grad_ref(dy, w, in_hw=(H, H), **kw)[0])
    assert torch.equal(dw.cpu().double(), bounds.weight_grad_ref(x, dy, torch.zeros(8, 7, 7, 1), **kw)[0])
    assert torch.equal(db.cpu().double(), dy.double().sum((0, 1, 2)))


@pytest.mark.parametrize("C,K,S", [(8, 7, 2), (12, 7, 1), (8, 5, 1)], ids=["stride2", "c12", "k5"])
def test_not_served(C, K, S):
    Ho, _ = gemm.conv_out_size(9, 9, K, K, S, K // 2, K // 2)
    g = ConvGeom(2, 9, 9, C, Ho, Ho, C, K, K, S, K // 2, K // 2, C)
    assert not gemm.dwlk_served(g)
    x = torch.zeros(2, 9, 9, C, device=DEV, dtype=torch.bfloat16)
    y = torch.full((2, Ho, Ho, C), SENTINEL, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="served"):
        gemm.dwlk_forward(x, torch.zeros(C, K, K, 1, device=DEV, dtype=torch.bfloat16), None, y, g)
    assert bool((y == SENTINEL).all())
