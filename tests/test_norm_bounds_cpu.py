"""Self-test, without a GPU, of the LRN / fused pool -> LRN / softmax / loss-gradient references in
tests/bounds.py.  The "kernel" is the kernels' own formula in fp32 torch (log2 / exp2 powers, fp32
sums in the kernels' order of operations, outputs rounded to bf16) at the input recipes of the GPU
tests (tests/norm_cases.py): it must stay inside every bound, and fill the bf16 ones to more than
0.3 (they are not slack).  Each seeded defect of the kind these kernels can make -- a halo channel
lost at a lane boundary, a window that runs over its row's end, an unwritten last pixel or cell
row, a band that misses the window row above it, an ignored relu bit, one image routed by
another's offsets, a bias sum short of a band, a softmax sum short of its tail, a per-lane
maximum, a bf16 copy from the wrong row -- must produce violations.

The evidence that the old assertions needed replacing: at the existing tests' alpha = 1e-3 the
LRN with its normalisation deleted altogether (y = x, dx = dy, pool -> LRN without the LRN) and
the lost halo channel pass the relerr / norm-ratio thresholds of tests/test_kernels_gpu.py and
tests/test_fused_pool_lrn_gpu.py, and a softmax sum that misses its tail element passes relerr
< 1e-2.  (The coarser defects -- a pixel left zero, a per-lane maximum -- fail the old checks
too; they are here so that the bound is known to name their place.)"""
import pytest
import torch

import bounds
import norm_cases as nc
from cxxnet_amd import ops

C0, NPIX0 = 40, 75  # tpp 5: lane boundaries at channels 8, 16, 24, 32


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def relerr(a, b):  # the old assertion of tests/test_kernels_gpu.py
    a, b = a.float(), b.float()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-6)).item()


def _window_matrix(C, h, drop=()):
    """W[c][c'] = 1 where c' is in the window of c; drop: (c, c') pairs left out"""
    i = torch.arange(C)
    W = ((i[:, None] - i[None, :]).abs() <= h).float()
    for c, c2 in drop:
        W[c, c2] = 0.0
    return W


def _winsum(W, h, spill=False):
    """v [npix][C] -> window sums.  spill: channel 0 also takes the previous pixel's last h
    channels (the window not clipped at the row's start: what a shuffle without the cv > 0 guard
    would fetch from the lane below)"""
    def f(v):
        s = v @ W.t()
        if spill and h > 0:
            s = s.clone()
            s[1:, 0] += v[:-1, v.shape[1] - h:].sum(1)
        return s
    return f


def emu_lrn(x, dy, n, alpha, beta, k, mask=False, winsum=None, identity=False):
    """(y, dx) bf16 of the emulated kernels (lrn_fwd_shfl / lrn_bwd_shfl's arithmetic in fp32)"""
    C = x.shape[-1]
    xf, g = x.float().reshape(-1, C), dy.float().reshape(-1, C)
    h = n // 2
    ws = winsum or _winsum(_window_matrix(C, h), h)
    sa, b, kk = _f32(alpha) / n, _f32(beta), _f32(k)
    if identity:  # the normalisation deleted
        y, dx = xf, g
    else:
        lg = torch.log2(kk + sa * ws(xf * xf))
        p = torch.exp2(-b * lg)
        y = xf * p
        t = g * xf * p * torch.exp2(-lg)
        dx = g * p - 2.0 * b * sa * xf * ws(t)
    if mask:
        dx = torch.where(xf > 0, dx, torch.zeros_like(dx))
    return y.to(torch.bfloat16).reshape(x.shape), dx.to(torch.bfloat16).reshape(x.shape)


def _refs(x, dy, n, prm, mask=False):
    return bounds.lrn_forward_ref(x, n, *prm), bounds.lrn_backward_ref(x, dy, n, *prm, mask_relu=mask)


# ------------------------------------------------------------------ LRN: the emulation fits
@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("prm", nc.LRN_PARAMS, ids=nc.LRN_PARAM_IDS)
@pytest.mark.parametrize("n", nc.LRN_SIZES)
def test_lrn_emulation_within_bound(n, prm, mask):
    x, dy = nc.lrn_inputs(NPIX0, C0, 100 + n, relu=mask)
    assert bounds.lrn_rel_err(x, n, *prm) <= bounds.LRN_E_MAX
    (yr, yb), (dr, db) = _refs(x, dy, n, prm, mask)
    y, dx = emu_lrn(x, dy, n, *prm, mask=mask)
    wf = bounds.assert_within(y, yr, yb, "lrn forward n %d" % n)
    wb = bounds.assert_within(dx, dr, db, "lrn backward n %d" % n)
    print("lrn n", n, prm, "mask" if mask else "", "max d/bound fwd %.3f bwd %.3f" % (wf, wb))
    assert wf > 0.3 and wb > 0.3  # bf16 rounding fills the bound: it is not slack
    if mask:
        dead = x.double() <= 0
        assert dead.float().mean() > 0.3
        assert torch.count_nonzero(dr[dead]) == 0 and torch.count_nonzero(db[dead]) == 0


def test_lrn_forward_u_is_tight():
    """with u = 2^-9 in place of 2^-8 the correct emulation violates"""
    x, dy = nc.lrn_inputs(NPIX0, C0, 7)
    ref, _ = bounds.lrn_forward_ref(x, 5, 0.25, 0.75, 1.0)
    y, _ = emu_lrn(x, dy, 5, 0.25, 0.75, 1.0)
    assert bounds.violations(y, ref, bounds.U_BF16 / 2 * ref.abs() * 1.001)[0] > 0


def test_cpu_executor_uses_the_kernels_window():
    """ops.lrn_forward / lrn_backward on CPU tensors (the fp32 executor) at an even local size:
    the window is c - h .. c + h as in the kernels, five channels at n = 4, not c - h .. c + h - 1."""
    x, dy = nc.lrn_inputs(NPIX0, C0, 11)
    for n in (4, 5):
        prm = (0.5, 0.75, 1.0)
        (yr, yb), (dr, db) = _refs(x, dy, n, prm)
        y, dx = torch.empty(x.shape), torch.empty(x.shape)
        ops.lrn_forward(x.float(), y, n, *prm)
        ops.lrn_backward(x.float(), dy.float(), dx, n, *prm)
        bounds.assert_within(y.to(torch.bfloat16), yr, yb, "cpu executor forward n %d" % n)
        bounds.assert_within(dx.to(torch.bfloat16), dr, db, "cpu executor backward n %d" % n)


# ------------------------------------------------------------------ LRN: seeded defects
def _cols(idx, shape):
    return set(torch.unravel_index(idx, shape)[-1].tolist())


@pytest.mark.parametrize("prm", nc.LRN_PARAMS, ids=nc.LRN_PARAM_IDS)
def test_lrn_normalisation_deleted(prm):
    x, dy = nc.lrn_inputs(NPIX0, C0, 21)
    (yr, yb), (dr, db) = _refs(x, dy, 5, prm)
    y, dx = emu_lrn(x, dy, 5, *prm, identity=True)
    assert bounds.violations(y, yr, yb)[0] > 0.9 * y.numel()
    assert bounds.violations(dx, dr, db)[0] > 0.9 * y.numel()


@pytest.mark.parametrize("C,n,fwd_thr,bwd_thr", [(64, 9, 1e-2, 2e-2), (96, 5, None, 2e-2)])
def test_old_lrn_thresholds_pass_without_normalisation(C, n, fwd_thr, bwd_thr):
    """tests/test_kernels_gpu.py::test_lrn's inputs, parameters and assertion with the kernel
    replaced by y = x, dx = dy.  (At C 96, n 5 the forward is just over its 1e-2: 0.0151.)"""
    g = lambda s, sc: (torch.randn(2, 13, 13, C, generator=torch.Generator().manual_seed(s)) * sc).to(torch.bfloat16).float()  # noqa: E731
    x, dy = g(15, 2.0), g(16, 1.0)
    y_ref, dx_ref = torch.empty_like(x), torch.empty_like(x)
    ops.lrn_forward(x, y_ref, n, 0.001, 0.75, 1.0)
    ops.lrn_backward(x, dy, dx_ref, n, 0.001, 0.75, 1.0)
    ef, eb = relerr(x.to(torch.bfloat16), y_ref), relerr(dy.to(torch.bfloat16), dx_ref)
    print("old test_lrn C %d n %d with the LRN deleted: relerr fwd %.4f bwd %.4f" % (C, n, ef, eb))
    if fwd_thr is not None:
        assert ef < fwd_thr
    assert eb < bwd_thr
    # the new bound at the old parameters still sees it (|y - x| ~ 1e-2 |x| against u = 2^-8)
    ref, bound = bounds.lrn_forward_ref(x, n, 0.001, 0.75, 1.0)
    assert bounds.violations(x.to(torch.bfloat16), ref, bound)[0] > 0


@pytest.mark.parametrize("prm", nc.LRN_PARAMS, ids=nc.LRN_PARAM_IDS)
@pytest.mark.parametrize("n", [3, 4, 5, 9])
def test_lrn_halo_channel_dropped(n, prm):
    """the window of channel 8 (first of a lane) without channel 7 (last of the lane below), in
    the forward sum and in both backward sums.  Forward only channel 8 moves; backward channel 8
    and, through the wrong norm in t[8], at most the channels whose window holds channel 8."""
    h = n // 2
    x, dy = nc.lrn_inputs(NPIX0, C0, 30 + n)
    (yr, yb), (dr, db) = _refs(x, dy, n, prm)
    ws = _winsum(_window_matrix(C0, h, drop=[(8, 7)]), h)
    y, dx = emu_lrn(x, dy, n, *prm, winsum=ws)
    cf, _, idf = bounds.violations(y, yr, yb)
    cb, _, idb = bounds.violations(dx, dr, db)
    print("halo dropped n", n, prm, "violations fwd %d bwd %d of %d" % (cf, cb, NPIX0))
    assert cf > NPIX0 // 2 and _cols(idf, y.shape) == {8}
    assert cb > NPIX0 // 2 and _cols(idb, y.shape) <= set(range(8 - h, 9 + h))
    assert (torch.unravel_index(idb, y.shape)[-1] == 8).sum() > NPIX0 // 2
    with pytest.raises(AssertionError, match=r"c 8\.\.8"):
        bounds.assert_within(y, yr, yb)


@pytest.mark.parametrize("defect", ["halo", "spill"])
def test_lrn_window_defects_pass_old_threshold_at_old_alpha(defect):
    """the two window defects at alpha = 1e-3 under the old assertion (relerr < 1e-2 forward, 2e-2
    backward): invisible; and mostly invisible to any per-element bound at that alpha (the
    output moves by ~6e-4, six times below bf16 rounding), which is why the new tests change
    alpha"""
    prm = (0.001, 0.75, 1.0)
    x, dy = nc.lrn_inputs(NPIX0, C0, 35)
    good = emu_lrn(x, dy, 5, *prm)
    ws = _winsum(_window_matrix(C0, 2, drop=[(8, 7)] if defect == "halo" else ()), 2, spill=defect == "spill")
    bad = emu_lrn(x, dy, 5, *prm, winsum=ws)
    (yr, yb), (dr, db) = _refs(x, dy, 5, prm)
    assert relerr(bad[0], yr) < 1e-2 and relerr(bad[1], dr) < 2e-2
    assert not torch.equal(bad[0], good[0]) or not torch.equal(bad[1], good[1])
    assert bounds.violations(bad[0], yr, yb)[0] < NPIX0 // 2


@pytest.mark.parametrize("n", [3, 5, 9])
def test_lrn_window_not_clipped_at_row_end(n):
    prm = nc.LRN_PARAMS[0]
    h = n // 2
    x, dy = nc.lrn_inputs(NPIX0, C0, 40 + n)
    (yr, yb), (dr, db) = _refs(x, dy, n, prm)
    y, dx = emu_lrn(x, dy, n, *prm, winsum=_winsum(_window_matrix(C0, h), h, spill=True))
    cf, _, idf = bounds.violations(y, yr, yb)
    cb, _, idb = bounds.violations(dx, dr, db)
    assert cf > NPIX0 // 2 and _cols(idf, y.shape) == {0}
    assert cb > NPIX0 // 2 and _cols(idb, y.shape) <= set(range(h + 1))  # (t[0] sits in their windows)
    assert (torch.unravel_index(idb, y.shape)[-1] == 0).sum() > NPIX0 // 2
    pix = torch.unravel_index(idf, y.shape)[2]
    assert int(pix.min()) >= 1  # pixel 0 has no pixel before it


def test_lrn_last_pixel_of_partial_wave_left_zero():
    prm = nc.LRN_PARAMS[1]
    x, dy = nc.lrn_inputs(NPIX0, C0, 50)
    (yr, yb), (dr, db) = _refs(x, dy, 5, prm)
    y, dx = emu_lrn(x, dy, 5, *prm)
    y[0, 0, -1], dx[0, 0, -1] = 0, 0
    for got, ref, bound in ((y, yr, yb), (dx, dr, db)):
        cnt, _, idx = bounds.violations(got, ref, bound)
        assert cnt > C0 * 3 // 4 and set(torch.unravel_index(idx, y.shape)[2].tolist()) == {NPIX0 - 1}
    with pytest.raises(AssertionError, match=r"w %d\.\.%d" % (NPIX0 - 1, NPIX0 - 1)):
        bounds.assert_within(y, yr, yb)


def test_lrn_mask_ignored_is_an_infinite_excess():
    prm = nc.LRN_PARAMS[0]
    x, dy = nc.lrn_inputs(NPIX0, C0, 55, relu=True)
    dr, db = bounds.lrn_backward_ref(x, dy, 5, *prm, mask_relu=True)
    _, dx = emu_lrn(x, dy, 5, *prm, mask=False)  # dx = dy p where x = 0: not 0
    cnt, worst, _ = bounds.violations(dx, dr, db)
    assert cnt > 0.3 * dx.numel() and worst == float("inf")


# ------------------------------------------------------------------ fused pool -> LRN
PN, PH, PW, PC = 2, 13, 13, 40  # R = 4 cell rows per band: HC = 7 -> two bands, the last of 3 rows
PR = 4


def _route32(v, tap, hw, skip=None):
    """fp32 routing of window values to the input pixels their tap names; skip(ho, kh, kw) -> bool
    drops contributions"""
    N, Ho, Wo, C = v.shape
    out = torch.zeros((N, hw[0], hw[1], C))
    for ho in range(Ho):
        for kh in range(3):
            for kw in range(3):
                if 2 * ho + kh >= hw[0] or (skip is not None and skip(ho, kh, kw)):
                    continue
                o = out[:, 2 * ho + kh, kw::2][:, :Wo]
                nw = o.shape[1]
                o += torch.where(tap[:, ho, :nw] == kh * 3 + kw, v[:, ho, :nw], torch.zeros(()))
    return out


def emu_fused(x, dY, n, prm, flags, relu_bit, tap=None, skip=None, ignore_bit=False):
    """(P, state, Y, gp, dx) of the emulated fused kernels"""
    P64, state = bounds.pool3s2_first_max(x, flags)
    P = P64.to(torch.bfloat16)  # a maximum of bf16 values: exact
    Y, gp = emu_lrn(P, dY, n, *prm)
    gp = gp.float()
    if relu_bit and not ignore_bit:
        gp = torch.where(state >= 128, torch.zeros(()), gp)
    t = (state & 127) if tap is None else tap
    return P, state, Y, gp, _route32(gp, t, x.shape[1:3], skip).to(torch.bfloat16)


@pytest.mark.parametrize("flags", [0, 2, 3, 6])
@pytest.mark.parametrize("n", [3, 5, 9])
def test_fused_emulation_within_bound(n, flags):
    prm = nc.LRN_PARAMS[n % 3]
    x, dY = nc.pool_inputs(PN, PH, PW, PC, 60 + n, nonneg=flags == 6)
    for relu_bit in (0, 1):
        r = bounds.pool_lrn_backward_ref(x, dY, n, *prm, flags, relu_bit=bool(relu_bit), dbias_init=0.5)
        P, state, Y, gp, dx = emu_fused(x, dY, n, prm, flags, relu_bit)
        assert torch.equal(P.double(), r["P"]) and torch.equal(state, r["state"])
        yr, yb = bounds.lrn_forward_ref(P, n, *prm)
        bounds.assert_within(Y, yr, yb, "fused forward")
        w = bounds.assert_within(dx, r["dx"], r["dx_bound"], "fused backward flags %d bit %d" % (flags, relu_bit))
        db = 0.5 + gp.reshape(-1, PC).sum(0)
        wd = bounds.assert_within(db, r["dbias"], r["dbias_bound"], "fused dbias", axes="c")
        print("fused n", n, "flags", flags, "bit", relu_bit, "max d/bound dx %.3f dbias %.3f" % (w, wd))
        assert w > 0.3
        unchosen = bounds._route(torch.ones_like(r["gp"]), r["state"] & 127, x.shape[1:3]) == 0
        assert unchosen.any() and torch.count_nonzero(r["dx_bound"][unchosen]) == 0
    if flags & 2:
        assert (state >= 128).float().mean() > 0.02  # the relu bit is exercised


def test_first_max_reference_matches_torch_where_torch_is_defined():
    """the explicit first-max pooling against F.max_pool2d's values (not its indices) and the
    executor's _pool_ref offsets on tie-free input"""
    x, _ = nc.pool_inputs(2, 8, 9, 8, 70, nonneg=False)
    P, state = bounds.pool3s2_first_max(x, 0)
    pr = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1)
    assert torch.equal(P.float(), pr)
    # ties: the first tap in kh * 3 + kw order wins, -0.0 ties with 0.0
    t = torch.zeros(1, 3, 3, 8, dtype=torch.bfloat16)
    t[0, 0, 1], t[0, 2, 2] = -0.0, 0.0
    P, state = bounds.pool3s2_first_max(t, 2)
    assert int(state.max()) == 128 and int(state.min()) == 128  # tap 0, max not > 0
    t[0, 1, 2], t[0, 2, 0] = 1.0, 1.0
    assert bounds.pool3s2_first_max(t, 2)[1].unique().tolist() == [5]


def _fused_case(flags=2, n=5, relu_bit=1):
    prm = nc.LRN_PARAMS[0]
    x, dY = nc.pool_inputs(PN, PH, PW, PC, 80, nonneg=False)
    r = bounds.pool_lrn_backward_ref(x, dY, n, *prm, flags, relu_bit=bool(relu_bit), dbias_init=0.5)
    return prm, x, dY, r


def _rows(idx, shape):
    return set(torch.unravel_index(idx, shape)[1].tolist())


def test_fused_last_band_cell_row_not_written():
    prm, x, dY, r = _fused_case()
    dx = emu_fused(x, dY, 5, prm, 2, 1)[4]
    dx[:, 2 * ((PH + 1) // 2 - 1):] = 0  # cell row HC - 1 = input row 12
    cnt, _, idx = bounds.violations(dx, r["dx"], r["dx_bound"])
    assert cnt > 0 and _rows(idx, dx.shape) == {12}


def test_fused_window_row_above_band_missing():
    """band 1 starts at cell row 4 (input rows 8, 9); window row 3 reaches input row 8 with its
    kh = 2 taps: without the recomputed row those contributions are lost"""
    prm, x, dY, r = _fused_case()
    dx = emu_fused(x, dY, 5, prm, 2, 1, skip=lambda ho, kh, kw: ho == PR - 1 and kh == 2)[4]
    cnt, _, idx = bounds.violations(dx, r["dx"], r["dx_bound"])
    assert cnt > PW * PC // 20 and _rows(idx, dx.shape) == {2 * PR}


def test_fused_relu_bit_ignored():
    prm, x, dY, r = _fused_case()
    dx = emu_fused(x, dY, 5, prm, 2, 1, ignore_bit=True)[4]
    cnt, worst, _ = bounds.violations(dx, r["dx"], r["dx_bound"])
    assert cnt > 0 and worst > 10


def test_fused_image_1_routed_by_image_0():
    prm, x, dY, r = _fused_case()
    tap = (r["state"] & 127).clone()
    tap[1] = tap[0]
    dx = emu_fused(x, dY, 5, prm, 2, 1, tap=tap)[4]
    cnt, _, idx = bounds.violations(dx, r["dx"], r["dx_bound"])
    assert cnt > dx[1].numel() // 10 and set(torch.unravel_index(idx, dx.shape)[0].tolist()) == {1}


def test_fused_dbias_without_one_band():
    prm, x, dY, r = _fused_case()
    gp = emu_fused(x, dY, 5, prm, 2, 1)[3]
    db = 0.5 + gp.reshape(-1, PC).sum(0)
    assert bounds.violations(db, r["dbias"], r["dbias_bound"])[0] == 0
    short = 0.5 + gp[:, :PR].reshape(-1, PC).sum(0)  # window rows 4, 5 (band 1) of both images missing
    assert bounds.violations(short, r["dbias"], r["dbias_bound"])[0] > PC * 3 // 4
    # one window's term missing from one column: a term of the column's median size
    col = 17
    terms = gp.reshape(-1, PC)[:, col]
    live = terms[terms != 0]
    term = live[live.abs().argsort()[live.numel() // 2]]
    one = db.clone()
    one[col] -= term
    cnt, _, idx = bounds.violations(one, r["dbias"], r["dbias_bound"])
    assert cnt == 1 and idx.tolist() == [col]


def test_old_fused_thresholds_pass_without_the_lrn():
    """tests/test_fused_pool_lrn_gpu.py::test_pool_lrn_kernels_vs_torch's assertion (norm ratio
    < 1e-2 forward, < 2e-2 backward) at its parameters (alpha 1e-3, n 5, relu'd input of scale 1)
    with the LRN deleted from both kernels: Y = P, dx = unpool(dY)"""
    N, H, C, n, prm = 3, 13, 64, 5, (1e-3, 0.75, 1.0)
    x = torch.randn(N, H, H, C, generator=torch.Generator().manual_seed(H)).clamp_min(0).to(torch.bfloat16)
    Ho = bounds.pool3s2_out(H)
    dY = nc.bf16_randn((N, Ho, Ho, C), 5)
    r = bounds.pool_lrn_backward_ref(x, dY, n, *prm, 2)
    P = r["P"]
    yr, yb = bounds.lrn_forward_ref(P, n, *prm)
    live = (r["state"] < 128).double()
    dx_bad = bounds._route(dY.double() * live, r["state"] & 127, (H, H))
    ef = ((P - yr).norm() / yr.norm()).item()
    eb = ((dx_bad - r["dx"]).norm() / r["dx"].norm()).item()
    print("old fused test with the LRN deleted: norm ratio fwd %.4f bwd %.4f" % (ef, eb))
    assert ef < 1e-2 and eb < 2e-2


# ------------------------------------------------------------------ softmax / loss gradient
LOG2E = 1.4426950408889634


def emu_softmax(x, tail_dropped=False, lane_max=False):
    """(p32, p bf16) as softmax_rows_reg computes them; tail_dropped: the sum without the last
    K % 64 elements; lane_max: each of the 64 lanes subtracts its own maximum"""
    xf = x.float()
    rows, K = xf.shape
    if lane_max:
        pad = torch.full((rows, (K + 63) // 64 * 64), float("-inf"))
        pad[:, :K] = xf
        m = pad.reshape(rows, -1, 64).max(1, keepdim=True).values.expand(rows, pad.shape[1] // 64, 64).reshape(rows, -1)[:, :K]
    else:
        m = xf.max(1, keepdim=True).values
    e = torch.exp2((xf - m) * _f32(LOG2E))
    s = (e[:, :K - K % 64] if tail_dropped else e).sum(1, keepdim=True)
    p = e * (1.0 / s)
    return p, p.to(torch.bfloat16)


@pytest.mark.parametrize("recipe", nc.SOFTMAX_RECIPES)
@pytest.mark.parametrize("K", nc.SOFTMAX_K)
def test_softmax_emulation_within_bound(K, recipe):
    rows = 5
    x = nc.softmax_input(recipe, rows, K)
    p, b32, b16 = bounds.softmax_ref(x)
    p32, pb = emu_softmax(x)
    w32 = bounds.assert_within(p32, p, b32, "softmax fp32 K %d %s" % (K, recipe), axes="rk")
    w16 = bounds.assert_within(pb, p, b16, "softmax bf16 K %d %s" % (K, recipe), axes="rk")
    assert torch.isfinite(p32).all()
    assert ((p32.double().sum(1) - 1).abs() <= bounds.softmax_sum_bound(x)).all()
    print("softmax K", K, recipe, "max d/bound fp32 %.3f bf16 %.3f" % (w32, w16))
    if K > 1 and recipe in ("scale3", "scale8"):  # (random probabilities: bf16 rounding fills the bound)
        assert w16 > 0.3
    for scale in (0.5, 1.0 / 256):
        lab = nc.softmax_labels(rows, K)
        ref, bound = bounds.loss_grad_ref(p32, lab, scale)
        oh = torch.zeros_like(p32).scatter_(1, lab.long(), 1.0)
        g = ((p32 - oh) * _f32(scale)).to(torch.bfloat16)
        bounds.assert_within(g, ref, bound, "loss gradient", axes="rk")


def test_softmax_tail_element_left_out_of_the_sum():
    """K = 65: the last element (K % 64 = 1) missing from the sum moves every probability of its
    row by the factor 1 / (1 - p_last).  The last element is put 6 under the row's maximum, so
    p_last is between 1e-4 and e^-6 = 2.5e-3: under the old relerr < 1e-2, and two orders over the
    fp32 bound (~1e-5 relative at K = 65) at every element."""
    x = nc.softmax_input("scale3", 5, 65)
    x[:, -1] = (x[:, :-1].float().max(1).values - 6.0).to(torch.bfloat16)
    p, b32, b16 = bounds.softmax_ref(x)
    p32, pb = emu_softmax(x, tail_dropped=True)
    assert 1e-4 < float(p[:, -1].min()) and float(p[:, -1].max()) < 2.5e-3
    assert relerr(p32, p) < 1e-2 and relerr(pb, p) < 1e-2  # the old assertion passes
    assert bounds.violations(emu_softmax(x)[0], p, b32)[0] == 0
    assert bounds.violations(p32, p, b32)[0] == 5 * 65
    assert ((p32.double().sum(1) - 1).abs() > bounds.softmax_sum_bound(x)).all()
    x = nc.softmax_input("scale3", 5, 1025)
    p, b32, b16 = bounds.softmax_ref(x)
    # a small probability wrong by half: invisible to max-error over max-value
    q = emu_softmax(x)[0]
    k = int(q[0].argmin())
    q[0, k] *= 1.5
    assert relerr(q, p) < 1e-2
    cnt, _, idx = bounds.violations(q, p, b32)
    assert cnt == 1 and idx.tolist() == [k]


def test_softmax_lane_max_on_a_row_with_one_large_value():
    x = nc.softmax_input("peak_lane", 5, 257)
    p, b32, b16 = bounds.softmax_ref(x)
    p32, pb = emu_softmax(x, lane_max=True)
    assert bounds.violations(p32, p, b32)[0] > 0 and bounds.violations(pb, p, b16)[0] > 0


def test_softmax_bf16_copy_from_another_row():
    x = nc.softmax_input("scale3", 5, 300)
    p, b32, b16 = bounds.softmax_ref(x)
    p32, pb = emu_softmax(x)
    bad = pb.clone()
    bad[4] = pb[3]
    assert bounds.violations(p32, p, b32)[0] == 0
    cnt, _, idx = bounds.violations(bad, p, b16)
    assert cnt > 300 // 2 and set(torch.unravel_index(idx, p.shape)[0].tolist()) == {4}


@pytest.mark.parametrize("kind", ["l2", "multi_logistic"])
def test_loss_grad_kinds_with_wide_labels(kind):
    rows, K = 5, 65
    pred = torch.sigmoid(nc.bf16_randn((rows, K), 90).float()).to(torch.bfloat16)
    lab = (torch.rand(rows, K, generator=torch.Generator().manual_seed(91)) > 0.5).float()
    ref, bound = bounds.loss_grad_ref(pred, lab, 0.5, kind=kind)
    g = ((pred.float() - lab) * 0.5).to(torch.bfloat16)
    bounds.assert_within(g, ref, bound, kind, axes="rk")
    g[rows - 1, K - 1] = ((pred.float()[rows - 1, K - 1] - lab[rows - 1, 0]) * 0.5 + 0.25).to(torch.bfloat16)
    assert bounds.violations(g, ref, bound)[0] == 1
