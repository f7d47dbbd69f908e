"""Every tile of the LDS-DMA GEMM (csrc/kernels/gemm_glds.hip: 19 K-major tiles, 6 MN-major tiles),
the one-wave-per-SIMD tile 114 and every compiled row of the register-staged kernel's dispatch
(gemm_mfma.hip), element by element against a float64 reference under the derived bounds of
tests/bounds.py, in the operand and epilogue forms training runs: conv forward (bias, bias + relu,
channel slices, two destinations), conv data gradient (plain, relu'-masked, masked with the bias
gradient, with a second gradient added), the row-gather forward, fc forward (bf16 and split-K slabs),
fc weight gradient (store, +=, fused SGD step) and conv weight gradient (atomic split-K, row-run).

Conventions of every case: the tile is forced and the case asserts that it ran (gemm.LAST_GLDS, or
the library's return code where the call is made directly) -- a tile that declines would otherwise
pass on a fallback kernel; the output is a view of a sentinel-filled buffer with one more image /
row (and, for channel slices, more channels), and nothing outside the view may change; CPU
operands and float64 references are cached per shape; the worst d / bound is printed.

The shapes are small on purpose (K <= ~1500, where one missing term still exceeds the bound:
tests/test_bounds_cpu.py) and chosen for the edges: G1's 588 pixels and 280 channels are ragged
against every BM / BN, its kdim 216 is 3 K-tiles and a 24 tail; G2 has Cg 8 (a K-tile spans 8 taps)
and 44 output channels (scalar stores); G3 a single partial K-tile; G4 two groups of 40 output
channels (rows staged past a group are the next group's weights: only the store gate keeps them
out); G5 stride 2 on a non-square map; G6 a 1 x 3 kernel with asymmetric padding; G7 25 taps; D1 a
12-channel data gradient."""
import contextlib
import functools

import pytest
import torch

import bounds
from test_tile_table_cpu import OP_FORMS, glds_served_matrix
from cxxnet_amd import native
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom, conv_out_size

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -3.0
KK = (1, 7, 10, 15, 21, 25, 30, 31, 34, 37, 38, 39, 72, 75, 76, 77, 78, 79, 82)
MM = (1, 2, 17, 23, 40, 41)
EPI_F32_ACC_REG = gemm.EPI_F32_ACC  # (the two kernels number this epilogue alike)

# (N, H, W, C, Cout, KH, KW, stride, pad_y, pad_x, groups)
GEOMS = {
    "G1": (3, 14, 14, 24, 280, 3, 3, 1, 1, 1, 1),
    "G2": (3, 14, 9, 8, 44, 3, 3, 1, 1, 1, 1),
    "G2w": (3, 14, 9, 8, 48, 3, 3, 1, 1, 1, 1),   # G2 with 48 output channels (MN-major rows % 8)
    "G3": (5, 7, 7, 16, 24, 1, 1, 1, 0, 0, 1),
    "G4": (3, 13, 13, 48, 80, 3, 3, 1, 1, 1, 2),
    "G5": (3, 15, 11, 16, 72, 3, 3, 2, 1, 1, 1),
    "G6": (2, 12, 10, 32, 64, 1, 3, 1, 0, 1, 1),
    "G7": (2, 9, 9, 16, 32, 5, 5, 1, 2, 2, 1),
    "D1": (3, 14, 9, 12, 48, 3, 3, 1, 1, 1, 1),
    "W4": (2, 12, 12, 12, 40, 3, 3, 1, 1, 1, 1),   # 12 channels: the register kernel's 4-wide loads
    "F1": (3, 13, 13, 64, 192, 3, 3, 1, 1, 1, 1),  # tile 114: Cg % 64, kdim % 64
    "F2": (4, 7, 7, 128, 64, 1, 1, 1, 0, 0, 1),
    "S1": (3, 14, 14, 16, 280, 1, 1, 1, 0, 0, 1),  # two-destination forward
    "S2": (5, 7, 7, 16, 280, 1, 1, 1, 0, 0, 1),
    "R1": (2, 23, 23, 4, 96, 11, 11, 4, 0, 0, 1),  # row gathers
    "R2": (2, 19, 19, 4, 64, 7, 7, 2, 0, 0, 1),
    "R3": (2, 23, 24, 3, 96, 11, 11, 4, 0, 0, 1),
}
# (B, nin, nout)
FC_FWD = [(37, 200, 280), (37, 1088, 280), (5, 64, 121), (300, 72, 24)]
FC_WG = [(37, 200, 280), (333, 136, 72)]
FC_ID = lambda c: "x".join(map(str, c))  # noqa: E731
LR, WD, MOM = 0.01, 5e-4, 0.9


def _geom(name):
    N, H, W, C, Cout, KH, KW, s, py, px, G = GEOMS[name]
    Ho, Wo = conv_out_size(H, W, KH, KW, s, py, px)
    return ConvGeom(N, H, W, C, Ho, Wo, Cout, KH, KW, s, py, px, G)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def _f32(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------ cached CPU operands and references
@functools.lru_cache(maxsize=None)
def _conv_operands(name):
    g = _geom(name)
    xs = (g.N, g.H, g.W, g.C)
    return dict(x=_rnd(xs, 1), w=_rnd((g.Cout, g.KH, g.KW, g.cg_in), 2, 0.05), b=_f32((g.Cout,), 3, 0.1),
                dy=_rnd((g.N, g.Ho, g.Wo, g.Cout), 4), act=torch.relu(_rnd(xs, 6)), add=_rnd(xs, 7),
                dw0=_f32((g.Cout, g.KH, g.KW, g.cg_in), 9))


@functools.lru_cache(maxsize=None)
def _fwd_ref(name):
    """float64 reference / bound of the pre-activation"""
    g, o = _geom(name), _conv_operands(name)
    return bounds.forward_ref(o["x"], o["w"], o["b"], stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.groups)


@functools.lru_cache(maxsize=None)
def _dgrad_ref(name, with_add):
    g, o = _geom(name), _conv_operands(name)
    return bounds.data_grad_ref(o["dy"], o["w"], stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.groups,
                                in_hw=(g.H, g.W), add=o["add"] if with_add else None)


@functools.lru_cache(maxsize=None)
def _wgrad_ref(name):
    g, o = _geom(name), _conv_operands(name)
    return bounds.weight_grad_ref(o["x"], o["dy"], o["dw0"], stride=g.stride, pad=(g.pad_y, g.pad_x), groups=g.groups)


@functools.lru_cache(maxsize=None)
def _fc_operands(case):
    B, nin, nout = case
    return dict(x=_rnd((B, nin), 11), w=_rnd((nout, nin), 12, 0.05), b=_f32((nout,), 14, 0.1), dy=_rnd((B, nout), 13),
                act=torch.relu(_rnd((B, nin), 17)), dw0=_f32((nout, nin), 15), w32=_f32((nout, nin), 16, 0.02),
                m32=_f32((nout, nin), 18, 0.01))


@functools.lru_cache(maxsize=None)
def _fc_fwd_ref(case):
    o = _fc_operands(case)
    return bounds.fc_forward_ref(o["x"], o["w"], o["b"])


@functools.lru_cache(maxsize=None)
def _fc_dgrad_ref(case, alpha):
    o = _fc_operands(case)
    return bounds.fc_data_grad_ref(o["dy"], o["w"], alpha=alpha, mask=o["act"] > 0)


@functools.lru_cache(maxsize=None)
def _fc_wgrad_ref(case, acc):
    o = _fc_operands(case)
    return bounds.fc_weight_grad_ref(o["x"], o["dy"], o["dw0"] if acc else None)


@functools.lru_cache(maxsize=None)
def _sgd_ref(case):
    o = _fc_operands(case)
    return bounds.sgd_step_ref(o["x"], o["dy"], o["w32"], o["m32"], LR, WD, MOM)


# ------------------------------------------------------------------------ guards, forcing, report
def _guarded(shape, dtype=torch.bfloat16, lo=0, extra=0, fill=None):
    """(buffer, view): the view is [:shape[0]] (channels [lo : lo + shape[-1]] when extra) of a
    sentinel-filled buffer with one more leading row / image and `extra` more channels."""
    buf = torch.full((shape[0] + 1,) + tuple(shape[1:-1]) + (shape[-1] + extra,), SENTINEL, device=DEV, dtype=dtype)
    view = buf[:shape[0], ..., lo:lo + shape[-1]]
    if fill is not None:
        view.copy_(fill.to(DEV))
    return buf, view


def _assert_guard(buf, shape, lo=0, what=""):
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[:shape[0], ..., lo:lo + shape[-1]] = False
    touched = outside & (buf != SENTINEL)
    if bool(touched.any()):
        idx = torch.nonzero(touched)
        raise AssertionError("%s: %d elements written outside the output view, first %s, last %s" % (
            what, idx.shape[0], idx[0].tolist(), idx[-1].tolist()))


def _sliced_input(t, lo, extra):
    g = torch.Generator().manual_seed(99)
    buf = torch.randn(*t.shape[:-1], t.shape[-1] + extra, generator=g).to(torch.bfloat16).to(DEV)
    buf[..., lo:lo + t.shape[-1]] = t.to(DEV)
    return buf[..., lo:lo + t.shape[-1]]


@contextlib.contextmanager
def _forced(tile, ops=None):
    """Force the LDS-DMA tile (and optionally the op classes routed to the kernel) for the block."""
    saved = (gemm._glds_cfg["tile"], gemm._glds_cfg["ops"])
    gemm._glds_cfg["tile"] = tile
    if ops is not None:
        gemm._glds_cfg["ops"] = set(saved[1]) | set(ops)
    gemm.LAST_GLDS[0] = None
    try:
        yield
    finally:
        gemm._glds_cfg["tile"], gemm._glds_cfg["ops"] = saved


def _ran(tile, what):
    assert gemm.LAST_GLDS[0] == tile, "%s: forced tile %s did not run (last LDS-DMA tile: %s)" % (
        what, tile, gemm.LAST_GLDS[0])


def _report(form, what, worst):
    print("d/bound [%s] %s: %.3f" % (form, what, worst))


def _within(form, got, ref, bound, what, axes="nhwc"):
    torch.cuda.synchronize()
    _report(form, what, bounds.assert_within(got.cpu(), ref, bound, what, axes=axes))


# ------------------------------------------------------------------------------- conv forward
def _glds_forward(tile):
    def launch(x, w, b, y, g, relu, what):
        with _forced(tile):
            gemm.conv_forward(x, w, b, y, g, relu=relu)
        _ran(tile, what)
    return launch


def _reg_forward(tile, va):
    def launch(x, w, b, y, g, relu, what):
        A, B = gemm._fwd_operands(x, w, g)
        gemm._gemm(A, B, gemm.DIRECT_K, gemm.GATHER_K, va, va, y, g.cg_out, gemm._pix(y), bias=b, bias_gstride=g.cg_out,
                   relu=relu, tile=tile, epi=gemm.EPI_BF16, groups=g.groups)
    return launch


def _check_forward(form, name, launch, relu, sliced=False):
    g, o = _geom(name), _conv_operands(name)
    ref, bound = _fwd_ref(name)
    what = "%s forward %s relu %d%s" % (form, name, relu, " sliced" if sliced else "")
    x = _sliced_input(o["x"], 8, 16) if sliced else o["x"].to(DEV)
    lo, extra = (64, 96) if sliced else (0, 0)
    shape = (g.N, g.Ho, g.Wo, g.Cout)
    yb, y = _guarded(shape, lo=lo, extra=extra)
    launch(x, o["w"].to(DEV), o["b"].to(DEV), y, g, relu, what)
    _within(form, y, ref.clamp_min(0) if relu else ref, bound, what)
    _assert_guard(yb, shape, lo, what)


@pytest.mark.parametrize("tile", KK)
@pytest.mark.parametrize("name", ["G1", "G2", "G3", "G4", "G5", "G6", "G7"])
def test_conv_forward(name, tile):
    for relu in (False, True):
        _check_forward("cf", name, _glds_forward(tile), relu)


@pytest.mark.parametrize("tile", KK)
def test_conv_forward_channel_slices(tile):
    """x at channels 8.. of a buffer 16 wider, y at channels 64.. of a buffer 96 wider."""
    _check_forward("cf", "G1", _glds_forward(tile), True, sliced=True)


@pytest.mark.parametrize("tile", KK)
@pytest.mark.parametrize("split", [8, 136])
@pytest.mark.parametrize("name", ["S1", "S2"])
def test_conv_forward_split(name, split, tile, monkeypatch):
    """conv_forward_split: output channels [0, split) into a channel slice of a wider buffer, the
    rest into a second buffer; split 136 lies inside an i-tile for every BM."""
    g, o = _geom(name), _conv_operands(name)
    ref, bound = _fwd_ref(name)
    what = "cfs %s split %d tile %d" % (name, split, tile)

    def no_fallback(*a, **k):
        raise AssertionError(what + ": the two-destination tile declined (two-GEMM fallback)")
    monkeypatch.setattr(gemm, "conv_forward", no_fallback)
    s1, s2 = (g.N, g.Ho, g.Wo, split), (g.N, g.Ho, g.Wo, g.Cout - split)
    yb, y = _guarded(s1, lo=32, extra=64)
    y2b, y2 = _guarded(s2)
    with _forced(tile):
        gemm.conv_forward_split(o["x"].to(DEV), o["w"].to(DEV), o["b"].to(DEV), y, y2, split, g, relu=True)
    _ran(tile, what)
    _within("cfs", torch.cat([y, y2], -1), ref.clamp_min(0), bound, what)
    _assert_guard(yb, s1, 32, what)
    _assert_guard(y2b, s2, 0, what)


@pytest.mark.parametrize("tile", KK)
@pytest.mark.parametrize("name", ["R1", "R2", "R3"])
def test_rowgather_forward(name, tile, monkeypatch):
    """The K_ROWGATHER forward ("cr"), with the direct row-run kernels in front of it off."""
    monkeypatch.setattr(gemm, "_ROWRUN_FWD2", False)
    monkeypatch.setattr(gemm, "_ROWRUN_DIRECT", False)
    for relu in (False, True):
        _check_forward("cr", name, _glds_forward(tile), relu)


# -------------------------------------------------------------------------- conv data gradient
DGRAD_MODES = ("plain", "mask", "mask_db", "add")


def _glds_dgrad(tile):
    def launch(dy, w, dx, g, mode, db, add, what):
        wt = torch.empty_like(w)
        with _forced(tile):
            if mode == "add":
                ok = gemm.conv_backward_data_add(dy, w, dx, add, g, wt, mask_relu=True)
            else:
                ok = gemm.conv_backward_data(dy, w, dx, g, wt_buf=wt, mask_relu=mode != "plain", dbias=db)
        if mode in ("add", "mask_db"):
            assert ok, what + ": the epilogue was not served"
        _ran(tile, what)
    return launch


def _reg_dgrad(tile):
    def launch(dy, w, dx, g, mode, db, add, what):
        A, B = gemm._dgrad_operands(dy, w, torch.empty_like(w), g, False)
        gemm._gemm(A, B, gemm.DIRECT_K, gemm.GATHER_K, 8, 8, dx, g.cg_in, gemm._pix(dx), epi=gemm.EPI_BF16,
                   groups=g.groups, mask_relu=mode != "plain", tile=tile)
    return launch


def _check_dgrad(form, name, launch, mode):
    g, o = _geom(name), _conv_operands(name)
    what = "%s data gradient %s %s" % (form, name, mode)
    ref, bound = _dgrad_ref(name, mode == "add")
    shape = (g.N, g.H, g.W, g.C)
    dxb, dx = _guarded(shape, fill=o["act"] if mode != "plain" else None)
    db = torch.full((g.C,), 0.5, device=DEV) if mode == "mask_db" else None
    launch(o["dy"].to(DEV), o["w"].to(DEV), dx, g, mode, db, o["add"].to(DEV) if mode == "add" else None, what)
    torch.cuda.synchronize()
    got = dx.cpu()
    if mode != "plain":
        m = o["act"] > 0
        assert torch.count_nonzero(got[~m]) == 0, what + ": a masked element is not 0"
        ref, bound = ref * m.double(), bound * m.double()
    _within(form, got, ref, bound, what)
    _assert_guard(dxb, shape, 0, what)
    if db is not None:
        dref, dbound = bounds.dbias_ref(got, 0.5)
        _within(form + " dbias", db, dref, dbound, what + " dbias", axes="c")


@pytest.mark.parametrize("tile", KK)
@pytest.mark.parametrize("name", ["G1", "G3", "G4", "G6", "G7", "D1"])
def test_conv_data_grad(name, tile):
    for mode in DGRAD_MODES:
        if name == "D1" and mode == "add":
            continue  # (12 channels: the add epilogue takes 8-channel rows only, see below)
        _check_dgrad("cd", name, _glds_dgrad(tile), mode)


def test_data_grad_add_declines_unaligned_rows():
    """conv_backward_data_add on a 12-channel dx (row stride not a multiple of 8) is refused
    before anything is written: the caller takes the separate sum."""
    g, o = _geom("D1"), _conv_operands("D1")
    dxb, dx = _guarded((g.N, g.H, g.W, g.C), fill=o["act"])
    w = o["w"].to(DEV)
    with _forced(1):
        assert not gemm.conv_backward_data_add(o["dy"].to(DEV), w, dx, o["add"].to(DEV), g, torch.empty_like(w))
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu(), o["act"])


# ------------------------------------------------------------------------------- fc forward
def _glds_fc_forward(tile):
    def launch(x, w, b, y, relu, what):
        with _forced(tile):
            gemm.fc_forward(x, w, b, y, relu=relu)
        _ran(tile, what)
    return launch


def _reg_fc_forward(tile, slab=False):
    def launch(x, w, b, y, relu, what):
        (B, nin), nout = x.shape, w.shape[0]
        A, Bo = gemm._op(w, 0, nin, nout, nin), gemm._op(x, 0, nin, B, nin)
        if not slab:
            gemm._gemm(A, Bo, gemm.DIRECT_K, gemm.DIRECT_K, 8, 8, y, 0, nout, bias=b, relu=relu, epi=gemm.EPI_BF16, tile=tile)
            return
        split = gemm._effective_split(nin, 2)
        assert split == 2
        ws = torch.full((split, B * nout), float("nan"), device=DEV)
        gemm._gemm(A, Bo, gemm.DIRECT_K, gemm.DIRECT_K, 8, 8, ws, 0, nout, epi=gemm.EPI_F32, ksplit=split, tile=tile,
                   kstride=B * nout)
        gemm._finalize(ws, split, B * nout, y, B, nout, b, relu, False, None)
    return launch


def _check_fc_forward(form, case, launch, relu):
    o = _fc_operands(case)
    ref, bound = _fc_fwd_ref(case)
    what = "%s fc forward %s relu %d" % (form, case, relu)
    shape = (case[0], case[2])
    yb, y = _guarded(shape)
    launch(o["x"].to(DEV), o["w"].to(DEV), o["b"].to(DEV), y, relu, what)
    _within(form, y, ref.clamp_min(0) if relu else ref, bound, what, axes="bo")
    _assert_guard(yb, shape, 0, what)


@pytest.mark.parametrize("tile", KK)
@pytest.mark.parametrize("case", FC_FWD, ids=FC_ID)
def test_fc_forward(case, tile):
    """(37, 1088, 280) takes the split-K slab path (2 slices of 9 + 8 K-tiles) and the finalize;
    (5, 64, 121) the scalar stores; (300, 72, 24) one partial i-tile under three j-tiles."""
    for relu in (False, True):
        _check_fc_forward("fc", case, _glds_fc_forward(tile), relu)


def test_fc_forward_split_k_is_taken():
    """The slab path of the case above really is the one _fc_glds_tile takes for every KK tile."""
    for t in KK:
        bm, bn = gemm.GLDS_TILES[t]
        tiles = -(-280 // bm) * -(-37 // bn)
        assert max(1, min(gemm.NUM_CU // tiles, -(-1088 // 64) // 8)) == 2
    assert gemm._effective_split(1088, 2) == 2


# --------------------------------------------------------------------------- fc weight gradient
def _glds_fc_wgrad(tile):
    def launch(x, dy, dw, acc, what):
        with _forced(tile):
            gemm.fc_backward_weight(x, dy, dw, overwrite=not acc)
        _ran(tile, what)
    return launch


def _reg_fc_wgrad(tile):
    def launch(x, dy, dw, acc, what):
        (B, nin), nout = x.shape, dy.shape[1]
        A, Bo = gemm._op(x, 0, nin, nin, B), gemm._op(dy, 0, nout, nout, B)
        gemm._gemm(A, Bo, gemm.DIRECT_MN, gemm.DIRECT_MN, 8, 8, dw, 0, nin,
                   epi=EPI_F32_ACC_REG if acc else gemm.EPI_F32, tile=tile)
    return launch


def _check_fc_wgrad(form, case, launch, acc):
    o = _fc_operands(case)
    ref, bound = _fc_wgrad_ref(case, acc)
    what = "%s fc weight gradient %s %s" % (form, case, "+=" if acc else "store")
    shape = (case[2], case[1])
    dwb, dw = _guarded(shape, torch.float32, fill=o["dw0"] if acc else None)
    launch(o["x"].to(DEV), o["dy"].to(DEV), dw, acc, what)
    _within(form, dw, ref, bound, what, axes="oi")
    _assert_guard(dwb, shape, 0, what)


@pytest.mark.parametrize("tile", MM)
@pytest.mark.parametrize("case", FC_WG, ids=FC_ID)
def test_fc_weight_grad(case, tile):
    """K is the batch: 37 is one partial K-tile, 333 five K-tiles and a 13 tail."""
    for acc in (False, True):
        _check_fc_wgrad("fw", case, _glds_fc_wgrad(tile), acc)


@pytest.mark.parametrize("tile", MM)
@pytest.mark.parametrize("case", FC_WG, ids=FC_ID)
def test_fc_weight_grad_sgd(case, tile):
    """EPI_F32_SGD on the tile dispatch (the streaming form switched off for the call)."""
    o = _fc_operands(case)
    what = "fws %s tile %d" % (case, tile)
    shape = (case[2], case[1])
    wb_, w = _guarded(shape, torch.float32, fill=o["w32"])
    mb_, m = _guarded(shape, torch.float32, fill=o["m32"])
    sb_, wb = _guarded(shape, fill=o["w32"].to(torch.bfloat16))
    k = native.kernels()
    old = k.cxn_gemm_set_sgd_stream(0)
    try:
        with _forced(tile):
            ok = gemm.fc_backward_weight_sgd(o["x"].to(DEV), o["dy"].to(DEV), w, m, wb, LR, WD, MOM, 0.0)
    finally:
        k.cxn_gemm_set_sgd_stream(old)
    assert ok, what + ": the tile declined"
    for nm, got, buf, (ref, bound) in zip(("m", "w", "wb"), (m, w, wb), (mb_, wb_, sb_), _sgd_ref(case)):
        _within("fws " + nm, got, ref, bound, what + " " + nm, axes="oi")
        _assert_guard(buf, shape, 0, what + " " + nm)


# ------------------------------------------------------------------------- conv weight gradient
def _check_wgrad(form, name, launch, what):
    g, o = _geom(name), _conv_operands(name)
    ref, bound = _wgrad_ref(name)
    shape = (g.Cout, g.KH, g.KW, g.cg_in)
    dwb, dw = _guarded(shape, torch.float32, fill=o["dw0"])
    launch(o["x"].to(DEV), o["dy"].to(DEV), dw, g)
    _within(form, dw, ref, bound, what, axes=("co", "kh", "kw", "ci"))
    _assert_guard(dwb, shape, 0, what)


@pytest.mark.parametrize("tile", MM)
@pytest.mark.parametrize("name", ["G1", "G4", "G5", "G2w"])
def test_conv_weight_grad(name, tile):
    """gemm._glds on gemm._wgrad_operands with an explicit K split onto a nonzero dw: G1's 588
    pixels are 10 K-tiles, so 4 slices are 3, 3, 3, 1 K-tiles and 64 clamps to 10."""
    for ksplit in (1, 2, 4, 64):
        what = "cw %s tile %d ksplit %d" % (name, tile, ksplit)

        def launch(x, dy, dw, g):
            A, B = gemm._wgrad_operands(x, dy, g)
            gemm.LAST_GLDS[0] = None
            assert gemm._glds(A, B, gemm.GL_MNG, gemm.GL_MN, dw, g.cg_out * g.kdim, g.kdim, epi=gemm.EPI_F32_ATOMIC_G,
                              groups=g.groups, ksplit=ksplit, tile=tile), what + ": the tile declined"
            _ran(tile, what)
        _check_wgrad("cw", name, launch, what)


@pytest.mark.parametrize("tile", MM)
def test_conv_weight_grad_wiring(tile):
    """Once through conv_backward_weight (its operands, group strides and K split)."""
    what = "cw G1 tile %d through conv_backward_weight" % tile

    def launch(x, dy, dw, g):
        with _forced(tile):
            gemm.conv_backward_weight(x, dy, dw, g)
        _ran(tile, what)
    _check_wgrad("cw", "G1", launch, what)


@pytest.mark.parametrize("tile", [1, 17])
@pytest.mark.parametrize("name", ["R1", "R3"])
def test_rowrun_weight_grad(name, tile):
    """The row-run weight gradient ("cwr") of the few-channel first layers."""
    what = "cwr %s tile %d" % (name, tile)

    def launch(x, dy, dw, g):
        with _forced(tile, ops=("cwr",)):
            gemm.conv_backward_weight(x, dy, dw, g)
        _ran(tile, what)
    _check_wgrad("cwr", name, launch, what)


# ------------------------------------------------------------------------------------ tile 114
@pytest.mark.parametrize("name", ["F1", "F2"])
def test_tile_114(name):
    for relu in (False, True):
        _check_forward("cf 114", name, _glds_forward(114), relu)
    for mode in ("plain", "mask"):
        _check_dgrad("cd 114", name, _glds_dgrad(114), mode)


# ------------------------------------------------------------------------------ register kernel
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", ["G1", "G4", "G5"])
def test_register_conv_forward(name, tile):
    for relu in (False, True):
        _check_forward("reg cf", name, _reg_forward(tile, 8), relu)


@pytest.mark.parametrize("tile", [0, 2, 3, 4])
def test_register_conv_forward_4wide(tile):
    for relu in (False, True):
        _check_forward("reg cf va4", "W4", _reg_forward(tile, 4), relu)


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4])
def test_register_strided_data_grad(tile):
    """The register kernel serves the strided data gradient (dy dilated by the forward stride)."""
    for mode in ("plain", "mask"):
        _check_dgrad("reg cd", "G5", _reg_dgrad(tile), mode)


@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "slabs"])
@pytest.mark.parametrize("tile", gemm.WGRAD_TILES)
@pytest.mark.parametrize("name", ["G1", "G4", "W4"])
def test_register_weight_grad(name, tile, det, ksplit):
    """Atomic split-K, and the deterministic per-slice slabs + cxn_splitk_accumulate; W4 takes the
    4-wide gather."""
    what = "reg cw %s tile %d %s ksplit %d" % (name, tile, "slabs" if det else "atomic", ksplit)

    def launch(x, dy, dw, g):
        va = 8 if g.cg_in % 8 == 0 else 4
        A, B = gemm._wgrad_operands(x, dy, g)
        kd = g.kdim
        if not det:
            gemm._gemm(A, B, gemm.GATHER_MN, gemm.DIRECT_MN, va, 8, dw, g.cg_out * kd, kd, epi=gemm.EPI_F32_ATOMIC,
                       groups=g.groups, ksplit=ksplit, tile=tile)
            return
        split = gemm._effective_split(g.N * g.Ho * g.Wo, ksplit)
        slab = g.Cout * kd
        ws = torch.full((split * slab,), float("nan"), device=DEV)
        gemm._gemm(A, B, gemm.GATHER_MN, gemm.DIRECT_MN, va, 8, ws, g.cg_out * kd, kd, epi=gemm.EPI_F32, groups=g.groups,
                   ksplit=split, tile=tile, kstride=slab)
        native.check(native.kernels().cxn_splitk_accumulate(ws.data_ptr(), split, slab, dw.data_ptr(), gemm._stream()),
                     "splitk_accumulate")
    _check_wgrad("reg cw", name, launch, what)


@pytest.mark.parametrize("tile", gemm.FC_TILES)
@pytest.mark.parametrize("case", FC_FWD, ids=FC_ID)
def test_register_fc(case, tile):
    """fc forward, data gradient (alpha = 2, relu'-masked) and weight gradient (store, +=)."""
    for relu in (False, True):
        _check_fc_forward("reg fc", case, _reg_fc_forward(tile), relu)
    B, nin, nout = case
    o = _fc_operands(case)
    ref, bound = _fc_dgrad_ref(case, 2.0)
    what = "reg fc data gradient %s tile %d" % (case, tile)
    dxb, dx = _guarded((B, nin), fill=o["act"])
    w, dy = o["w"].to(DEV), o["dy"].to(DEV)
    gemm._gemm(gemm._op(w, 0, nin, nin, nout), gemm._op(dy, 0, nout, B, nout), gemm.DIRECT_MN, gemm.DIRECT_K, 8, 8, dx, 0,
               nin, mask_relu=True, alpha=2.0, tile=tile)
    torch.cuda.synchronize()
    assert torch.count_nonzero(dx.cpu()[~(o["act"] > 0)]) == 0, what + ": a masked element is not 0"
    _within("reg fc dgrad", dx, ref, bound, what, axes="bi")
    _assert_guard(dxb, (B, nin), 0, what)
    if nin % 8 == 0 and nout % 8 == 0:
        for acc in (False, True):
            _check_fc_wgrad("reg fw", case, _reg_fc_wgrad(tile), acc)


@pytest.mark.parametrize("tile", gemm.FC_TILES)
def test_register_fc_slab_finalize(tile):
    """The fp32-slab + finalize path of the fc forward (two K slices)."""
    for relu in (False, True):
        _check_fc_forward("reg fc slabs", (37, 1088, 280), _reg_fc_forward(tile, slab=True), relu)


# ------------------------------------------------------------------------------- served matrix
def _matrix_launchers():
    """form -> launch(tile) -> (served, [output buffers, sentinel-filled before the call]); small
    operands, one launcher per CXG_CASE row of gemm_glds.hip's dispatch()."""
    k = native.kernels()
    g3, o3 = _geom("G3"), _conv_operands("G3")
    x3, w3, dy3, b3 = o3["x"].to(DEV), o3["w"].to(DEV), o3["dy"].to(DEV), o3["b"].to(DEV)
    gr, orr = _geom("R1"), _conv_operands("R1")
    xr, wr = orr["x"].to(DEV), orr["w"].to(DEV)
    B, nin, nout = 5, 128, 24
    fx, fw, fdy = _rnd((B, nin), 31).to(DEV), _rnd((nout, nin), 32, 0.05).to(DEV), _rnd((B, nout), 33).to(DEV)
    full = lambda shape, dtype=torch.bfloat16: torch.full(shape, SENTINEL, device=DEV, dtype=dtype)  # noqa: E731

    def cf(t):
        y = full((g3.N, g3.Ho, g3.Wo, g3.Cout))
        A, Bv = gemm._fwd_operands(x3, w3, g3)
        return gemm._glds(A, Bv, gemm.GL_K, gemm.GL_KG, y, g3.cg_out, g3.Cout, bias=b3, bias_gstride=g3.cg_out, tile=t), [y]

    def dgrad_ops():
        return gemm._dgrad_operands(dy3, w3, torch.empty_like(w3), g3, False)

    def cd_db(t):
        dx, db = full((g3.N, g3.H, g3.W, g3.C)), full((g3.C,), torch.float32)
        A, Bv = dgrad_ops()
        ws = torch.empty((Bv.rows // 16 + 9) * g3.C, device=DEV)
        return gemm._glds(A, Bv, gemm.GL_K, gemm.GL_KG, dx, g3.cg_in, g3.C, tile=t, epi=gemm.EPI_BF16_DB_G,
                          bias_gstride=g3.cg_in, dbias=db, dws=ws, dws_ld=g3.C), [dx, db]

    def cd_add(t):
        dx = full((g3.N, g3.H, g3.W, g3.C))
        A, Bv = dgrad_ops()
        add = o3["add"].to(DEV)
        rc = k.cxn_gemm_glds_add(A, Bv, gemm.GL_K, gemm.GL_KG, dx.data_ptr(), g3.cg_in, g3.C, add.data_ptr(), 0, t, 1,
                                 gemm._stream())
        torch.cuda.synchronize()  # (add is read by the launch)
        return gemm.served(rc, "gemm_glds_add"), [dx]

    def cr(t):
        y = full((gr.N, gr.Ho, gr.Wo, gr.Cout))
        wp, lp = gemm._row_padded_weights(wr, gr)
        kr = gr.KH * lp
        Ar = gemm._op(wp, 0, kr, gr.Cout, kr)
        Br = gemm._op(xr, 0, 0, gr.N * gr.Ho * gr.Wo, kr, H=gr.H, W=gr.W, C=gr.C, Ho=gr.Ho, Wo=gr.Wo, KH=gr.KH, KW=gr.KW,
                      stride=gr.stride, pad_h=0, pad_w=0, dil=1, Cg=gr.C)
        return gemm._glds(Ar, Br, gemm.GL_K, gemm.GL_KR, y, 0, gr.Cout, tile=t), [y]

    def fc(t):
        y = full((B, nout))
        return gemm._glds(gemm._op(fw, 0, nin, nout, nin), gemm._op(fx, 0, nin, B, nin), gemm.GL_K, gemm.GL_K, y, 0, nout,
                          tile=t), [y]

    def fc_slab(t):
        ws = full((2, B * nout), torch.float32)
        return gemm._glds(gemm._op(fw, 0, nin, nout, nin), gemm._op(fx, 0, nin, B, nin), gemm.GL_K, gemm.GL_K, ws, 0, nout,
                          epi=gemm.EPI_F32, ksplit=2, kstride=B * nout, tile=t), [ws]

    def cw(t):
        dw = full((g3.Cout, g3.KH, g3.KW, g3.cg_in), torch.float32)
        A, Bv = gemm._wgrad_operands(x3, dy3, g3)
        return gemm._glds(A, Bv, gemm.GL_MNG, gemm.GL_MN, dw, g3.cg_out * g3.kdim, g3.kdim, epi=gemm.EPI_F32_ATOMIC_G,
                          tile=t), [dw]

    def fw_ops():
        return gemm._op(fx, 0, nin, nin, B), gemm._op(fdy, 0, nout, nout, B)

    def fwg(epi):
        def run(t):
            dw = full((nout, nin), torch.float32)
            A, Bv = fw_ops()
            return gemm._glds(A, Bv, gemm.GL_MN, gemm.GL_MN, dw, 0, nin, epi=epi, tile=t), [dw]
        return run

    def fw_sgd(t):
        w, m, wb = full((nout, nin), torch.float32), full((nout, nin), torch.float32), full((nout, nin))
        A, Bv = fw_ops()
        old = k.cxn_gemm_set_sgd_stream(0)
        try:
            rc = k.cxn_gemm_glds_sgd(A, Bv, nin, 1.0, w.data_ptr(), m.data_ptr(), wb.data_ptr(), LR, WD, MOM, 0.0, None, t,
                                     gemm._stream())
        finally:
            k.cxn_gemm_set_sgd_stream(old)
        return gemm.served(rc, "gemm_glds_sgd"), [w, m, wb]

    return {("K_DIRECT", "K_GATHER", "EPI_BF16"): cf, ("K_DIRECT", "K_GATHER", "EPI_BF16_DB"): cd_db,
            ("K_DIRECT", "K_GATHER", "EPI_BF16_ADD"): cd_add, ("K_DIRECT", "K_ROWGATHER", "EPI_BF16"): cr,
            ("K_DIRECT", "K_DIRECT", "EPI_BF16"): fc, ("K_DIRECT", "K_DIRECT", "EPI_F32"): fc_slab,
            ("MN_GATHER", "MN_DIRECT", "EPI_F32_ATOMIC"): cw, ("MN_DIRECT", "MN_DIRECT", "EPI_F32"): fwg(gemm.EPI_F32),
            ("MN_DIRECT", "MN_DIRECT", "EPI_F32_ACC"): fwg(gemm.EPI_F32_ACC_G), ("MN_DIRECT", "MN_DIRECT", "EPI_F32_SGD"): fw_sgd}


ALL_FORMS = sorted({f for fs in OP_FORMS.values() for f in fs})


@pytest.mark.parametrize("form", ALL_FORMS, ids="-".join)
def test_served_matrix(form):
    """Every (form, tile) of gemm_glds.hip's dispatch as the source says: a tile of the form's
    set is served (and recorded in LAST_GLDS), any other tile of the switches returns "not
    served" and leaves a sentinel-filled output untouched."""
    kk, mm, forms = glds_served_matrix()
    assert kk == set(KK) and mm == set(MM)
    launch = _matrix_launchers()[form]
    serving = kk if forms[form] == "KK" else mm
    direct = form[2] in ("EPI_BF16_ADD", "EPI_F32_SGD")  # (called below gemm._glds: no LAST_GLDS record)
    for t in sorted(kk | mm):
        gemm.LAST_GLDS[0] = None
        ok, outs = launch(t)
        torch.cuda.synchronize()
        if t in serving:
            assert ok, (form, t, "declined")
            assert direct or gemm.LAST_GLDS[0] == t, (form, t, gemm.LAST_GLDS[0])
            assert all(bool((o != SENTINEL).any()) for o in outs), (form, t, "served but an output is untouched")
        else:
            assert not ok, (form, t, "served a tile the form does not compile")
            assert gemm.LAST_GLDS[0] is None
            assert all(bool((o == SENTINEL).all()) for o in outs), (form, t, "declined but wrote")
