"""The LRN kernels (lrn_fwd_shfl / lrn_fwd, lrn_bwd_shfl / lrn_bwd_lds / lrn_bwd, lrn_bwd_db) and the
fused max-pool -> LRN pair (pool_lrn_fwd, lrn_pool_bwd), element by element against the float64
references and derived bounds of tests/bounds.py, through cxxnet_amd.ops only.

The inputs (tests/norm_cases.py) are exact bf16 values with alpha in [0.25, 1] on x of scale 2:
the norm runs from 1 to ~40, so a wrong window -- a halo channel lost at a lane boundary, a
window that runs into the neighbouring pixel, a band that misses the row above it -- moves the
output by many times the bf16 rounding the bound allows; at the nets' alpha = 1e-3 the
normalisation could be deleted under the earlier thresholds (tests/test_norm_bounds_cpu.py).
The shapes walk the lane layouts: one lane per pixel, C / 8 not dividing 64 (idle lanes), one
pixel per wave (the shuffles wrap at lanes 0 and 63), partial last waves and blocks, more groups
than blocks (grid stride), the scalar-edge and LDS forms past C = 512, and, fused, half windows,
half cells, partial last bands and every band height."""
import pytest
import torch

import bounds
import norm_cases as nc
from cxxnet_amd import ops
from cxxnet_amd.ops import gemm

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

# (C, npix)
LRN_CASES = [
    (8, 67),      # one lane per pixel (no neighbour lanes) and a partial wave
    (24, 43),     # 3 lanes per pixel, 21 pixels per wave, lane 63 idle
    (40, 25),     # 5 lanes per pixel
    (96, 11),     # 12 lanes per pixel
    (256, 5),     # two pixels per wave, odd count
    (512, 3),     # one pixel per wave: the shuffles wrap at lanes 0 and 63
    (520, 7),     # forward: lrn_fwd's scalar edge loads; backward: lrn_bwd_lds, 3 pixels per block, an idle fourth
    (2048, 3),    # lrn_bwd_lds, one pixel per block
    (2056, 3),    # the generic lrn_bwd: out of place only
]
BIG = (512, 4 * 4096 + 5)  # one pixel per wave, 4 per group: more than 4096 groups, 8.4M elements


def _prm(*keys):
    return nc.LRN_PARAMS[sum(keys) % len(nc.LRN_PARAMS)]


def _nan_like(t):
    return torch.full_like(t, NAN)


@pytest.mark.parametrize("n", nc.LRN_SIZES)
@pytest.mark.parametrize("C,npix", LRN_CASES)
def test_lrn_forward_backward_within_bound(C, npix, n):
    prm = _prm(LRN_CASES.index((C, npix)), nc.LRN_SIZES.index(n))
    for mask in (False, True):
        x, dy = nc.lrn_inputs(npix, C, 3 * C + n, relu=mask)
        assert bounds.lrn_rel_err(x, n, *prm) <= bounds.LRN_E_MAX
        what = "C %d npix %d n %d %s%s" % (C, npix, n, prm, " mask" if mask else "")
        xd, dyd = x.to(DEV), dy.to(DEV)
        y = _nan_like(xd)
        ops.lrn_forward(xd, y, n, *prm)
        wf = bounds.assert_within(y, *bounds.lrn_forward_ref(x, n, *prm), "lrn forward " + what)
        dx = _nan_like(xd)
        ops.lrn_backward(xd, dyd, dx, n, *prm, mask_relu=mask)
        wb = bounds.assert_within(dx, *bounds.lrn_backward_ref(x, dy, n, *prm, mask_relu=mask), "lrn backward " + what)
        print("d/bound lrn_fwd %.3f lrn_bwd %.3f  %s" % (wf, wb, what))
        xi = xd.clone()
        if C // 8 > 256:  # the generic kernel reads its neighbours' x from memory: it must refuse dx is x
            with pytest.raises(RuntimeError):
                ops.lrn_backward(xi, dyd, xi, n, *prm, mask_relu=mask)
            torch.cuda.synchronize()
            assert torch.equal(xi, xd)
        else:
            ops.lrn_backward(xi, dyd, xi, n, *prm, mask_relu=mask)
            assert torch.equal(xi, dx)


def test_lrn_forward_grid_stride():
    C, npix = BIG
    n, prm = 5, nc.LRN_PARAMS[0]
    x, _ = nc.lrn_inputs(npix, C, 77)
    y = _nan_like(x.to(DEV))
    ops.lrn_forward(x.to(DEV), y, n, *prm)
    w = bounds.assert_within(y, *bounds.lrn_forward_ref(x, n, *prm), "lrn forward, %d pixels of %d" % (npix, C))
    print("d/bound lrn_fwd %.3f  grid stride" % w)


@pytest.mark.parametrize("C,npix,n,mask", [(64, 37, 5, False), (192, 50, 3, True), (512, 9, 9, True), BIG + (5, True)])
def test_lrn_backward_bias_within_bound(C, npix, n, mask):
    """lrn_bwd_db: dx as the plain backward's, and db += the column sums of the stored dx from a
    non-zero start, in place as out of place"""
    prm = _prm(C // 64, n)
    x, dy = nc.lrn_inputs(npix, C, C + npix, relu=mask)
    assert bounds.lrn_rel_err(x, n, *prm) <= bounds.LRN_E_MAX
    xd, dyd = x.to(DEV), dy.to(DEV)
    init = torch.linspace(-1.0, 1.0, C)
    db, dx = init.to(DEV), _nan_like(xd)
    assert ops.lrn_backward_bias(xd, dyd, dx, n, *prm, db, mask_relu=mask)
    what = "C %d npix %d n %d %s" % (C, npix, n, prm)
    wx = bounds.assert_within(dx, *bounds.lrn_backward_ref(x, dy, n, *prm, mask_relu=mask), "lrn_bwd_db dx " + what)
    wd = bounds.assert_within(db, *bounds.dbias_ref(dx, init), "lrn_bwd_db db " + what, axes="c")
    print("d/bound lrn_bwd_db dx %.3f db %.3g  %s" % (wx, wd, what))
    xi, db2 = xd.clone(), init.to(DEV)
    assert ops.lrn_backward_bias(xi, dyd, xi, n, *prm, db2, mask_relu=mask)
    assert torch.equal(xi, dx)
    bounds.assert_within(db2, *bounds.dbias_ref(dx, init), "lrn_bwd_db db in place " + what, axes="c")


# ------------------------------------------------------------------ fused max-pool -> LRN
# (H, W, C), N = 2
POOL_CASES = [
    (8, 9, 8),      # an even and an odd edge: half windows and half cells
    (13, 13, 40),   # 4 cell rows per band: two bands, the last partial
    (13, 14, 96),
    (9, 9, 256),    # 2 cell rows per band, a partial last band
    (27, 27, 512),  # LDS leaves one cell row per band
    (3, 3, 16),     # one window
]
POOL_PARAMS = [(H, W, C, n) for H, W, C in POOL_CASES for n in ((3, 5, 9) if C == 40 else (3, 5))]
_pool_cache = {}


def _pool_case(H, W, C, flags):
    """inputs and the flag's pooling reference, computed once per (case, flags)"""
    key = (H, W, C, flags)
    if key not in _pool_cache:
        x, dY = nc.pool_inputs(2, H, W, C, H * W + C + flags, nonneg=flags == 6)
        _pool_cache[key] = (x, dY) + bounds.pool3s2_first_max(x, flags)
    return _pool_cache[key]


@pytest.mark.parametrize("flags", [0, 2, 3, 6])
@pytest.mark.parametrize("H,W,C,n", POOL_PARAMS)
def test_pool_lrn_forward_backward_within_bound(H, W, C, n, flags):
    N = 2
    prm = _prm(POOL_CASES.index((H, W, C)), n, flags)
    x, dY, Pr, sr = _pool_case(H, W, C, flags)
    Ho, Wo = Pr.shape[1], Pr.shape[2]
    what = "%dx%dx%d n %d flags %d %s" % (H, W, C, n, flags, prm)
    xd, dYd = x.to(DEV), dY.to(DEV)
    P = torch.full((N, Ho, Wo, C), NAN, device=DEV, dtype=torch.bfloat16)
    st = torch.full((N, Ho, Wo, C), 255, device=DEV, dtype=torch.uint8)
    Y = _nan_like(P)
    assert ops.pool_lrn_forward(xd, P, st, Y, flags, n, *prm)
    assert torch.equal(P.cpu().double(), Pr), what
    assert torch.equal(st.cpu(), sr), what
    assert bounds.lrn_rel_err(P, n, *prm) <= bounds.LRN_E_MAX
    wf = bounds.assert_within(Y, *bounds.lrn_forward_ref(P, n, *prm), "pool_lrn forward " + what)
    R = N * Ho * Wo
    rows = ops.lrn_pool_backward_rows(x.shape, P.shape, n)
    assert rows > 0
    part = torch.empty(rows, C, device=DEV)
    init = torch.linspace(-1.0, 1.0, C)
    wx = wd = 0.0
    for relu_bit in (0, 1):
        r = bounds.pool_lrn_backward_ref(x, dY, n, *prm, flags, relu_bit=bool(relu_bit),
                                         dbias_init=init if R <= 100 else None)
        dx = _nan_like(xd)  # every pixel must be written
        assert ops.lrn_pool_backward(P, dYd, st, dx, relu_bit, n, *prm)
        wx = max(wx, bounds.assert_within(dx, r["dx"], r["dx_bound"], "lrn_pool backward bit %d " % relu_bit + what))
        if R > 100:
            continue
        for det in (True, False):
            gemm.set_deterministic(det)
            db, dx2 = init.to(DEV), _nan_like(xd)
            assert ops.lrn_pool_backward(P, dYd, st, dx2, relu_bit, n, *prm, dbias=db, part=part)
            assert torch.equal(dx2, dx)
            wd = max(wd, bounds.assert_within(db, r["dbias"], r["dbias_bound"],
                                              "lrn_pool dbias bit %d det %d " % (relu_bit, det) + what, axes="c"))
    print("d/bound pool_lrn_fwd %.3f lrn_pool_bwd dx %.3f dbias %.3f  %s" % (wf, wx, wd, what))
