"""Self-test of tests/bounds.py without a GPU.  The "kernel" is an fp32 CPU convolution rounded
to bf16 (fp32 sums for the bias and weight gradients): for every formula it must stay inside
the derived bound, and each seeded defect of the kind a direct kernel can make -- a tap dropped
at one border pixel, one image's last row taken from the neighbouring image, one relu' mask bit
flipped, one dW element missing one pixel's term, a bias gradient that skips the last image --
must produce violations.  This is the evidence that the GPU tests built on the helper fail on a
subtly wrong kernel, where the whole-tensor norm they replace does not."""
import pytest
import torch
import torch.nn.functional as F

import bounds

# (N, H, C, Cout, groups, KS): K = KS KS C / groups from 288 to 3456
SHAPES = [
    (3, 13, 32, 64, 1, 3),     # K = 288
    (3, 14, 128, 64, 1, 3),    # K = 1152
    (2, 27, 96, 96, 2, 5),     # K = 1200
    (5, 13, 384, 128, 2, 3),   # K = 1728
    (2, 13, 384, 64, 1, 3),    # K = 3456
]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _fwd_operands(shape):
    N, H, C, Cout, groups, KS = shape
    x = _rnd((N, H, H, C), 1)
    w = _rnd((Cout, KS, KS, C // groups), 2, 0.05)
    b = torch.randn(Cout, generator=torch.Generator().manual_seed(3)) * 0.1
    return x, w, b


def _emu_forward(x, w, b, groups, relu):
    """fp32 pre-activation (NHWC) of the emulated kernel and its stored bf16 output"""
    z = _nhwc(F.conv2d(_nchw(x), _nchw(w), b, padding=w.shape[1] // 2, groups=groups))
    return z, (z.clamp_min(0) if relu else z).to(torch.bfloat16)


def _dgrad_operands(shape):
    N, H, C, Cout, groups, KS = shape
    dy = _rnd((N, H, H, Cout), 4)
    w = _rnd((Cout, KS, KS, C // groups), 5, 0.05)
    act = torch.relu(_rnd((N, H, H, C), 6))
    return dy, w, act


def _emu_dgrad(dy, w, groups, mask=None):
    v = _nhwc(F.conv_transpose2d(_nchw(dy), _nchw(w), padding=w.shape[1] // 2, groups=groups))
    if mask is not None:
        v = v * mask
    return v


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_emulation_within_bound(shape, relu):
    x, w, b = _fwd_operands(shape)
    ref, bound = bounds.forward_ref(x, w, b, pad=shape[5] // 2, groups=shape[4], relu=relu)
    _, y = _emu_forward(x, w, b, shape[4], relu)
    worst = bounds.assert_within(y, ref, bound, "forward %s" % (shape,))
    print("forward", shape, "relu" if relu else "", "max d/bound %.3f" % worst)
    assert worst > 0.3  # the bound is not slack by an order of magnitude: bf16 rounding fills it


def test_u_bf16_is_tight():
    """With u = 2^-9 a correct fp32 computation violates the bound."""
    shape = SHAPES[0]
    x, w, b = _fwd_operands(shape)
    ref, bound = bounds.forward_ref(x, w, b, pad=1)
    _, y = _emu_forward(x, w, b, 1, False)
    gA = (bound - bounds.U_BF16 * ref.abs()) / (1 + bounds.U_BF16)
    assert bounds.violations(y, ref, bounds.U_BF16 / 2 * (ref.abs() + gA) + gA)[0] > 0


@pytest.mark.parametrize("mode", ["plain", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_data_grad_emulation_within_bound(shape, mode):
    dy, w, act = _dgrad_operands(shape)
    mask = act > 0 if mode == "mask" else None
    ref, bound = bounds.data_grad_ref(dy, w, pad=shape[5] // 2, groups=shape[4], mask=mask)
    dx = _emu_dgrad(dy, w, shape[4], mask).to(torch.bfloat16)
    worst = bounds.assert_within(dx, ref, bound, "data gradient %s" % (shape,))
    print("data gradient", shape, mode, "max d/bound %.3f" % worst)
    if mask is not None:
        assert torch.count_nonzero(ref[~mask]) == 0 and torch.count_nonzero(bound[~mask]) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dbias_emulation_within_bound(shape):
    dy, w, act = _dgrad_operands(shape)
    dx = _emu_dgrad(dy, w, shape[4], act > 0).to(torch.bfloat16)
    ref, bound = bounds.dbias_ref(dx, 0.5)
    db = torch.full((shape[2],), 0.5) + dx.float().reshape(-1, shape[2]).sum(0)
    bounds.assert_within(db, ref, bound, "dbias %s" % (shape,), axes="c")


# (N, H, W, C, Cout): K = N H W up to ~1500
WGRAD = [(1, 13, 13, 64, 64), (3, 14, 14, 64, 128), (2, 20, 37, 64, 64)]


def _wgrad_operands(case):
    N, H, W, C, Cout = case
    x, dy = _rnd((N, H, W, C), 7), _rnd((N, H, W, Cout), 8)
    dw0 = torch.randn(Cout, 3, 3, C, generator=torch.Generator().manual_seed(9))
    dw = dw0 + _nhwc(torch.nn.grad.conv2d_weight(_nchw(x), (Cout, C, 3, 3), _nchw(dy), padding=1))
    return x, dy, dw0, dw


@pytest.mark.parametrize("case", WGRAD, ids=lambda c: "x".join(map(str, c)))
def test_weight_grad_emulation_within_bound_and_missing_term(case):
    N, H, W, C, Cout = case
    x, dy, dw0, dw = _wgrad_operands(case)
    ref, bound = bounds.weight_grad_ref(x, dy, dw0, pad=1)
    worst = bounds.assert_within(dw, ref, bound, "weight gradient %s" % (case,), axes=("co", "kh", "kw", "ci"))
    print("weight gradient", case, "max d/bound %.3g" % worst)
    # defect: one element, dw[co][0][2][ci], misses one pixel's term -- a pixel of the bottom row,
    # whose term has the median magnitude of the row's (not the largest: a typical term)
    co, ci, n, h = Cout - 1, C - 3, N - 1, H - 1
    terms = dy[n, h, :W - 1, co].float() * x[n, h - 1, 1:, ci].float()  # tap (kh 0, kw 2): x[h - 1][w + 1]
    wpix = int(terms.abs().argsort()[terms.numel() // 2])
    bad = dw.clone()
    bad[co, 0, 2, ci] -= terms[wpix]
    cnt, _, idx = bounds.violations(bad, ref, bound)
    assert cnt == 1 and idx.tolist() == [((co * 3 + 0) * 3 + 2) * C + ci]
    with pytest.raises(AssertionError, match=r"1 of \d+ elements outside"):
        bounds.assert_within(bad, ref, bound, axes=("co", "kh", "kw", "ci"))
    # ... and a wholly wrong element, which the 1e-2 norm these tests used alone hides
    bad = dw.clone()
    bad[0, 1, 1, 0] = 0.0
    assert ((bad - ref.float()).norm() / ref.float().norm()).item() < 1e-2
    assert bounds.violations(bad, ref, bound)[0] == 1


def test_dropped_tap_at_corner_of_last_image():
    """One tap dropped at the corner pixel of the last image, every output channel (the issue's
    first case, N = 87, 32 -> 384): the norm the tests used stays under its threshold, the
    elementwise bound flags most of the channels."""
    N, H, C, Cout = 87, 13, 32, 384
    x, w, b = _fwd_operands((N, H, C, Cout, 1, 3))
    ref, bound = bounds.forward_ref(x, w, b, pad=1, relu=True)
    z, y = _emu_forward(x, w, b, 1, True)
    assert bounds.violations(y, ref, bound)[0] == 0
    z[N - 1, 0, 0] -= (w[:, 1, 1, :].float() * x[N - 1, 0, 0].float()).sum(1)  # the centre tap of pixel (0, 0)
    bad = z.clamp_min(0).to(torch.bfloat16)
    norm = ((bad.double() - ref).norm() / ref.norm()).item()
    assert norm < 5e-3  # invisible to the old assertion
    cnt, _, idx = bounds.violations(bad, ref, bound)
    assert cnt > Cout // 3
    where = torch.unravel_index(idx, ref.shape)
    assert set(where[0].tolist()) == {N - 1} and set(where[1].tolist()) == {0} and set(where[2].tolist()) == {0}
    with pytest.raises(AssertionError, match=r"n 86\.\.86, h 0\.\.0, w 0\.\.0"):
        bounds.assert_within(bad, ref, bound)


@pytest.mark.parametrize("relu", [False, True])
def test_last_row_from_neighbouring_image(relu):
    """An odd batch whose last image's bottom row holds the previous image's."""
    shape = (5, 13, 64, 64, 1, 3)
    x, w, b = _fwd_operands(shape)
    ref, bound = bounds.forward_ref(x, w, b, pad=1, relu=relu)
    _, y = _emu_forward(x, w, b, 1, relu)
    y[4, 12] = y[3, 12]
    cnt, _, idx = bounds.violations(y, ref, bound)
    where = torch.unravel_index(idx, ref.shape)
    assert cnt > 13 * 64 // 3
    assert set(where[0].tolist()) == {4} and set(where[1].tolist()) == {12}


def test_mask_bit_flipped():
    shape = (3, 13, 64, 64, 1, 3)
    dy, w, act = _dgrad_operands(shape)
    mask = act > 0
    ref, bound = bounds.data_grad_ref(dy, w, pad=1, mask=mask)
    plain = _emu_dgrad(dy, w, 1)
    good = (plain * mask).to(torch.bfloat16)
    assert bounds.violations(good, ref, bound)[0] == 0
    # a masked element stored anyway: any non-zero value violates (its bound is 0)
    off = torch.nonzero(~mask)[-1].tolist()
    bad = good.clone()
    bad[tuple(off)] = plain[tuple(off)].to(torch.bfloat16)
    assert bad[tuple(off)] != 0
    cnt, worst, idx = bounds.violations(bad, ref, bound)
    assert cnt == 1 and worst == float("inf")
    assert list(torch.unravel_index(idx[0], ref.shape)) == off
    # a live element masked away: the first one of the last image
    on = torch.nonzero(mask[2])[0].tolist()
    bad = good.clone()
    bad[(2, *on)] = 0
    assert bounds.violations(bad, ref, bound)[0] == 1


def test_dbias_skips_last_image():
    shape = (3, 13, 64, 64, 1, 3)
    dy, w, act = _dgrad_operands(shape)
    dx = _emu_dgrad(dy, w, 1, act > 0).to(torch.bfloat16)
    ref, bound = bounds.dbias_ref(dx, 0.5)
    db = 0.5 + dx[:2].float().reshape(-1, 64).sum(0)
    assert bounds.violations(db, ref, bound)[0] > 64 * 3 // 4
    # one pixel's term missing from one column
    db = 0.5 + dx.float().reshape(-1, 64).sum(0)
    pix = dx[2, 12, 12].float()
    col = int(pix.abs().argmax())
    db[col] -= pix[col]
    cnt, _, idx = bounds.violations(db, ref, bound)
    assert cnt == 1 and idx.tolist() == [col]


def test_nan_is_a_violation():
    ref, bound = torch.zeros(2, 2, dtype=torch.float64), torch.ones(2, 2, dtype=torch.float64)
    got = torch.zeros(2, 2)
    got[1, 0] = float("nan")
    assert bounds.violations(got, ref, bound)[0] == 1
    with pytest.raises(AssertionError):
        bounds.assert_within(got, ref, bound, axes="ab")


# ------------------------------------------------------------------ GEMM references (fc, SGD step)
# (B, nin, nout): the shapes of tests/test_gemm_tiles_bounds_gpu.py
FC = [(37, 200, 280), (37, 1088, 280), (5, 64, 121), (300, 72, 24), (333, 136, 72)]
FC_IDS = ["x".join(map(str, s)) for s in FC]


def _fc_operands(case):
    B, nin, nout = case
    x, w, dy = _rnd((B, nin), 11), _rnd((nout, nin), 12, 0.05), _rnd((B, nout), 13)
    b = torch.randn(nout, generator=torch.Generator().manual_seed(14)) * 0.1
    return x, w, dy, b


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", FC, ids=FC_IDS)
def test_fc_forward_emulation_and_zeroed_chunk(case, relu):
    B, nin, nout = case
    x, w, _, b = _fc_operands(case)
    ref, bound = bounds.fc_forward_ref(x, w, b, relu=relu)
    emu = lambda xx: (xx.float() @ w.float().t() + b)  # noqa: E731
    post = lambda z: (z.clamp_min(0) if relu else z).to(torch.bfloat16)  # noqa: E731
    worst = bounds.assert_within(post(emu(x)), ref, bound, "fc forward %s" % (case,), axes="bo")
    print("fc forward", case, "max d/bound %.3f" % worst)
    # one 16-byte DMA of x lost: 8 k of the last batch row read as zero
    bad = x.clone()
    bad[B - 1, nin - 16:nin - 8] = 0
    cnt, _, idx = bounds.violations(post(emu(bad)), ref, bound)
    rows = torch.unravel_index(idx, ref.shape)[0]
    live = int((ref[B - 1] > 0).sum()) if relu else nout
    assert cnt > live // 2 and set(rows.tolist()) == {B - 1}, (cnt, live)


@pytest.mark.parametrize("case", FC, ids=FC_IDS)
def test_fc_data_grad_emulation_and_zeroed_chunk(case):
    B, nin, nout = case
    x, w, dy, _ = _fc_operands(case)
    mask = x > 0
    ref, bound = bounds.fc_data_grad_ref(dy, w, alpha=2.0, mask=mask)
    emu = lambda d: ((d.float() @ w.float()) * 2.0 * mask).to(torch.bfloat16)  # noqa: E731
    worst = bounds.assert_within(emu(dy), ref, bound, "fc data gradient %s" % (case,), axes="bi")
    print("fc data gradient", case, "max d/bound %.3f" % worst)
    assert torch.count_nonzero(bound[~mask]) == 0
    bad = dy.clone()
    bad[0, :8] = 0
    cnt, _, idx = bounds.violations(emu(bad), ref, bound)
    assert cnt > int(mask[0].sum()) // 2 and set(torch.unravel_index(idx, ref.shape)[0].tolist()) == {0}


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("case", FC, ids=FC_IDS)
def test_fc_weight_grad_emulation_and_zeroed_chunk(case, acc):
    B, nin, nout = case
    x, _, dy, _ = _fc_operands(case)
    dw0 = torch.randn(nout, nin, generator=torch.Generator().manual_seed(15)) if acc else None
    ref, bound = bounds.fc_weight_grad_ref(x, dy, dw0)
    emu = lambda xx: (dy.float().t() @ xx.float()) + (dw0 if acc else 0)  # noqa: E731
    worst = bounds.assert_within(emu(x), ref, bound, "fc weight gradient %s" % (case,), axes="oi")
    print("fc weight gradient", case, "max d/bound %.3g" % worst)
    # MN-major operand: one 16-byte DMA is 8 consecutive nin columns of one batch row (one k)
    bad = x.clone()
    bad[B - 1, nin - 8:] = 0
    cnt, _, idx = bounds.violations(emu(bad), ref, bound)
    cols = torch.unravel_index(idx, ref.shape)[1]
    assert cnt > nout * 8 // 3 and int(cols.min()) >= nin - 8, (cnt, nout * 8)


@pytest.mark.parametrize("case", [(37, 200, 280), (333, 136, 72)], ids=["37x200x280", "333x136x72"])
def test_sgd_step_emulation_and_zeroed_chunk(case):
    B, nin, nout = case
    x, _, dy, _ = _fc_operands(case)
    g = torch.Generator().manual_seed(16)
    w, m = torch.randn(nout, nin, generator=g) * 0.02, torch.randn(nout, nin, generator=g) * 0.01
    lr, wd, mom = 0.01, 5e-4, 0.9
    refs = bounds.sgd_step_ref(x, dy, w, m, lr, wd, mom)

    def emu(xx):
        grad = dy.float().t() @ xx.float()
        m1 = mom * m - lr * (grad + wd * w)
        w1 = w + m1
        return m1, w1, w1.to(torch.bfloat16)
    for name, got, (ref, bound) in zip(("m", "w", "wb"), emu(x), refs):
        worst = bounds.assert_within(got, ref, bound, "sgd %s %s" % (name, case), axes="oi")
        print("sgd step", case, name, "max d/bound %.3g" % worst)
    bad = x.clone()
    bad[B - 1, nin - 8:] = 0
    for name, got, (ref, bound) in zip(("m", "w", "wb"), emu(bad), refs):
        cnt, _, idx = bounds.violations(got, ref, bound)
        cols = torch.unravel_index(idx, ref.shape)[1]
        assert cnt > nout * 8 // 3 and int(cols.min()) >= nin - 8, (name, cnt)


def test_conv_refs_take_tuple_padding_stride_and_nonsquare_kernels():
    """forward_ref with a 1 x 3 kernel and (0, 1) padding, data_grad_ref with forward stride 2 at
    a size where the output_padding is not 0, against fp32 torch (conv2d / conv2d_input)."""
    x, w = _rnd((2, 12, 10, 32), 21), _rnd((64, 1, 3, 32), 22, 0.05)
    ref, bound = bounds.forward_ref(x, w, None, pad=(0, 1))
    y = _nhwc(F.conv2d(_nchw(x), _nchw(w), padding=(0, 1))).to(torch.bfloat16)
    assert tuple(ref.shape) == (2, 12, 10, 64)
    bounds.assert_within(y, ref, bound, "1x3 forward")
    dy = _rnd((2, 12, 10, 64), 23)
    ref, bound = bounds.data_grad_ref(dy, w, pad=(0, 1))
    dx = _nhwc(torch.nn.grad.conv2d_input((2, 32, 12, 10), _nchw(w), _nchw(dy), padding=(0, 1))).to(torch.bfloat16)
    bounds.assert_within(dx, ref, bound, "1x3 data gradient")
    # stride 2, 3 x 3, pad 1 on 16 x 12: Ho x Wo = 8 x 6, output_padding (1, 1)
    w, dy = _rnd((72, 3, 3, 16), 24, 0.05), _rnd((3, 8, 6, 72), 25)
    ref, bound = bounds.data_grad_ref(dy, w, stride=2, pad=1, in_hw=(16, 12))
    assert tuple(ref.shape) == (3, 16, 12, 16)
    dx = _nhwc(torch.nn.grad.conv2d_input((3, 16, 16, 12), _nchw(w), _nchw(dy), stride=2, padding=1)).to(torch.bfloat16)
    bounds.assert_within(dx, ref, bound, "strided data gradient")
    dx[2, 15, 11] = 0  # the last row / column exists only through the output_padding
    assert bounds.violations(dx, ref, bound)[0] > 0


def test_emulated_gemm_gate_defects_are_located():
    """Two defects of the implicit-GEMM tiles, emulated on geometry G4 of
    tests/test_gemm_tiles_bounds_gpu.py (3 x 13 x 13, 2 groups of 24 -> 40 channels, 3 x 3):
    the store gate of a 64-row tile dropped (rows 40..63 staged for group 0 are group 1's first
    24 weight rows, and land on group 1's channels), and the K tail lost (kdim 216 = 3 K-tiles
    and a 24 tail: the last tap's channels).  The violations name the place."""
    x, w = _rnd((3, 13, 13, 48), 31), _rnd((80, 3, 3, 24), 32, 0.05)
    b = torch.randn(80, generator=torch.Generator().manual_seed(33)) * 0.1
    ref, bound = bounds.forward_ref(x, w, b, pad=1, groups=2)
    emu = lambda ww: _nhwc(F.conv2d(_nchw(x), _nchw(ww), b, padding=1, groups=2))  # noqa: E731
    good = emu(w).to(torch.bfloat16)
    assert bounds.violations(good, ref, bound)[0] == 0
    # (a) group 0's tile stores 64 rows: group 1's weight rows 0..23 against group 0's input, no bias
    bad = good.clone()
    bad[..., 40:64] = _nhwc(F.conv2d(_nchw(x[..., :24]), _nchw(w[40:64]), padding=1)).to(torch.bfloat16)
    cnt, _, idx = bounds.violations(bad, ref, bound)
    ch = torch.unravel_index(idx, ref.shape)[3]
    assert cnt > 3 * 13 * 13 * 24 * 0.9 and int(ch.min()) == 40 and int(ch.max()) == 63
    with pytest.raises(AssertionError, match=r"c 40\.\.63"):
        bounds.assert_within(bad, ref, bound)
    # (b) k = (kh, kw, c) >= 192 is tap (2, 2): every pixel that has the tap inside the image
    tail = w.clone()
    tail[:, 2, 2, :] = 0
    cnt, _, idx = bounds.violations(emu(tail).to(torch.bfloat16), ref, bound)
    n, h, ww_, c = torch.unravel_index(idx, ref.shape)
    assert cnt > 3 * 12 * 12 * 80 // 2 and int(h.max()) == 11 and int(ww_.max()) == 11
