"""Every form of cxn_conv_direct (csrc/kernels/conv_direct.hip), element by element against a
float64 reference under the derived bound of tests/bounds.py: launch_cd at 13 x 13 and 14 x 14
with variants 0 / 1 / 2 (the schedules the shipped table's pseudo-tiles 200 / 201 / 202 pick),
version 2 (variant 3) in its 128- / 96-channel forms at 13 x 13 and its 128- / 48-channel forms
at 27 x 27, and the paired-tap form with 64- and 48-channel blocks; each with the epilogues
training runs -- forward bias and bias + relu, data gradient plain, relu'-masked, and masked with
the bias-gradient sum.

A case is written in the kernel's terms, (N, Kin, Kout, groups, H, KS): the forward runs it as
the convolution Kin -> Kout, the data gradient as the gradient of a convolution Kout -> Kin
(dy has Kin channels, dx Kout), so both directions run the same kernel form on the same item
count.  The item-walk cases are sized from the launchers' own formulas
(launch_cd: ceil(N / 2) groups Kout_g / 64; version 2: ceil(N / IPB) NB groups Kout_g / block)
to 256 < nitems < 512: the grid is capped at 256 blocks, so some blocks walk two items -- the
second item's first stage lands under the first one's last taps -- and others one.

Every output is a view of a buffer with one more image (and, in the slice tests, more channels)
filled with a sentinel: the absent image of an odd batch must not be stored and nothing may be
written outside the view.  Variants 0 / 1 / 2 of launch_cd run the same stage body (same tap and
stage order into the same accumulators, same partial-row layout for the bias gradient) and differ
only in who issues the DMAs and how many stage buffers there are, so their outputs are asserted
bitwise equal."""
import functools

import pytest
import torch

import bounds
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -3.0

# form -> (variants, [(N, Kin, Kout, groups, H, KS), ...]); the last case(s) of a persistent form
# walk items (nitems in the comment)
FORMS = {
    "cd13": ((0, 1, 2), [
        (1, 64, 64, 1, 13, 3),       # one item
        (5, 192, 128, 1, 13, 3),     # six stages, odd N
        (7, 128, 128, 2, 13, 3),     # grouped, odd N
        (87, 32, 384, 1, 13, 3),     # 44 x 6 = 264 items, one stage, odd N
        (45, 64, 768, 1, 13, 3),     # 23 x 12 = 276 items, two stages, odd N
    ]),
    "cd14": ((0, 1, 2), [
        (5, 128, 128, 1, 14, 3),
        (3, 64, 128, 2, 14, 3),
        (87, 32, 384, 1, 14, 3),     # 264 items
    ]),
    "c2_13_128": ((3,), [
        (1, 96, 128, 1, 13, 3),      # six 16-channel chunks
        (5, 64, 256, 2, 13, 3),
        (131, 64, 512, 2, 13, 3),    # 66 x 2 x 2 = 264 items
    ]),
    "c2_13_96": ((3,), [
        (7, 64, 192, 1, 13, 3),
        (3, 64, 384, 2, 13, 3),
        (131, 64, 384, 2, 13, 3),    # 66 x 2 x 2 = 264 items
    ]),
    "c2_27_128": ((3,), [
        (3, 16, 128, 1, 27, 5),
        (1, 96, 256, 2, 27, 5),      # three chunks
        (33, 32, 512, 2, 27, 5),     # 33 x 2 bands x 2 x 2 = 264 items
    ]),
    "c2_27_48": ((3,), [
        (3, 32, 48, 1, 27, 5),
        (5, 96, 96, 2, 27, 5),
        (23, 32, 288, 2, 27, 5),     # 23 x 2 bands x 2 x 3 = 276 items
    ]),
    "cp_64": ((0,), [(3, 64, 128, 1, 27, 5), (5, 32, 128, 2, 27, 5)]),   # (one block per item: no walk)
    "cp_48": ((0,), [(1, 16, 48, 1, 27, 5), (3, 96, 96, 2, 27, 5)]),
}
RUNS = [pytest.param(case, v, id="%s-%s-v%d" % (form, "x".join(map(str, case[:4])), v))
        for form, (variants, cases) in FORMS.items() for case in cases for v in variants]
SLICE_RUNS = [pytest.param(cases[0 if form != "cd13" else 1], v, id="%s-v%d" % (form, v))
              for form, (variants, cases) in FORMS.items() for v in variants]
EQUAL_RUNS = [pytest.param(case, id="%s-%s" % (form, "x".join(map(str, case[:4]))))
              for form in ("cd13", "cd14") for case in FORMS[form][1]]


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


# Operands (CPU) and float64 references are cached per case: the variant and epilogue parameters
# (the inner loops of the parametrization) do not recompute them.
@functools.lru_cache(maxsize=2)
def _forward_operands(case):
    N, Kin, Kout, groups, H, KS = case
    x = _rnd((N, H, H, Kin), 1)
    w = _rnd((Kout, KS, KS, Kin // groups), 2, 0.05)
    b = torch.randn(Kout, generator=torch.Generator().manual_seed(3)) * 0.1
    return x, w, b


@functools.lru_cache(maxsize=2)
def _forward_ref(case):
    """float64 reference / bound of the pre-activation"""
    return bounds.forward_ref(*_forward_operands(case), pad=case[5] // 2, groups=case[3])


@functools.lru_cache(maxsize=2)
def _data_operands(case):
    N, Kin, Kout, groups, H, KS = case
    dy = _rnd((N, H, H, Kin), 4)
    w = _rnd((Kin, KS, KS, Kout // groups), 5, 0.05)  # the weights of the convolution Kout -> Kin
    act = torch.relu(_rnd((N, H, H, Kout), 6))        # relu(z) of the node the gradient is written to
    return dy, w, act


@functools.lru_cache(maxsize=2)
def _data_ref(case):
    dy, w, _ = _data_operands(case)
    return bounds.data_grad_ref(dy, w, pad=case[5] // 2, groups=case[3])


def _nitems(case, variant):
    N, Kin, Kout, groups, H, KS = case
    cog = Kout // groups
    if variant == 3:
        if H == 27:
            return N * 2 * groups * (cog // (128 if cog % 128 == 0 else 48))
        return (N + 1) // 2 * groups * (cog // (128 if cog % 128 == 0 else 96))
    if H == 27:
        return N * 2 * groups * (cog // (64 if cog % 64 == 0 else 48))
    return (N + 1) // 2 * groups * (cog // 64)


def test_item_walk_cases_walk():
    """The last case of every persistent form gives 256 < nitems < 512 (the launchers' formulas)."""
    got = {form: _nitems(cases[-1], variants[0]) for form, (variants, cases) in FORMS.items() if not form.startswith("cp")}
    assert got == {"cd13": 276, "cd14": 264, "c2_13_128": 264, "c2_13_96": 264, "c2_27_128": 264, "c2_27_48": 276}
    assert _nitems(FORMS["cd13"][1][-2], 0) == 264


def _guarded(N, H, C, lo=0, extra=0, fill=None):
    """(buffer, view): the view is images [:N], channels [lo : lo + C] of a sentinel-filled buffer
    with one more image and `extra` more channels; fill (CPU, the view's shape) is copied in."""
    buf = torch.full((N + 1, H, H, C + extra), SENTINEL, device=DEV, dtype=torch.bfloat16)
    view = buf[:N, :, :, lo:lo + C] if extra else buf[:N]
    if fill is not None:
        view.copy_(fill.to(DEV))
    return buf, view


def _assert_guard(buf, N, C, lo=0):
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


def _run_forward(case, variant, relu, sliced=False):
    N, Kin, Kout, groups, H, KS = case
    x, w, b = _forward_operands(case)
    g = ConvGeom(N, H, H, Kin, H, H, Kout, KS, KS, 1, KS // 2, KS // 2, groups)
    xd = _sliced_input(x, 32, 64) if sliced else x.to(DEV)
    lo, extra = (64, 96) if sliced else (0, 0)
    yb, y = _guarded(N, H, Kout, lo, extra)
    assert gemm.conv_direct_forward(xd, w.to(DEV), b.to(DEV), y, g, relu=relu, variant=variant)
    torch.cuda.synchronize()
    _assert_guard(yb, N, Kout, lo)
    return y.cpu()


def _run_data(case, variant, mode, sliced=False):
    N, Kin, Kout, groups, H, KS = case
    dy, w, act = _data_operands(case)
    g = ConvGeom(N, H, H, Kout, H, H, Kin, KS, KS, 1, KS // 2, KS // 2, groups)
    wd = w.to(DEV)
    wt = torch.empty_like(wd)
    gemm.conv_weight_flip_multi([(wd, wt, g)])
    dyd = _sliced_input(dy, 32, 64) if sliced else dy.to(DEV)
    lo, extra = (64, 96) if sliced else (0, 0)
    dxb, dx = _guarded(N, H, Kout, lo, extra, fill=act if mode != "plain" else None)
    db = torch.full((Kout,), 0.5, device=DEV) if mode == "mask_db" else None
    assert gemm.conv_direct_data(dyd, wt, dx, g, mask_relu=mode != "plain", dbias=db, variant=variant)
    torch.cuda.synchronize()
    _assert_guard(dxb, N, Kout, lo)
    return dx.cpu(), db.cpu() if db is not None else None


def _check_forward(case, variant, relu, sliced=False):
    ref, bound = _forward_ref(case)
    y = _run_forward(case, variant, relu, sliced)
    worst = bounds.assert_within(y, ref.clamp_min(0) if relu else ref, bound,
                                 "forward %s variant %d relu %d" % (case, variant, relu))
    print("forward %s variant %d relu %d%s: max d/bound %.3f" % (case, variant, relu, " sliced" if sliced else "", worst))


def _check_data(case, variant, mode, sliced=False):
    act = _data_operands(case)[2]
    ref, bound = _data_ref(case)
    dx, db = _run_data(case, variant, mode, sliced)
    what = "data gradient %s variant %d %s" % (case, variant, mode)
    if mode != "plain":
        m = act > 0
        assert torch.count_nonzero(dx[~m]) == 0, what + ": a masked element is not 0"
        m = m.double()
        ref, bound = ref * m, bound * m
    worst = bounds.assert_within(dx, ref, bound, what)
    print("%s%s: max d/bound %.3f" % (what, " sliced" if sliced else "", worst))
    if db is not None:
        dref, dbound = bounds.dbias_ref(dx, 0.5)
        worst = bounds.assert_within(db, dref, dbound, what + " dbias", axes="c")
        print("%s dbias: max d/bound %.3g" % (what, worst))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case,variant", RUNS)
def test_forward(case, variant, relu):
    _check_forward(case, variant, relu)


@pytest.mark.parametrize("mode", ["plain", "mask", "mask_db"])
@pytest.mark.parametrize("case,variant", RUNS)
def test_data_grad(case, variant, mode):
    _check_data(case, variant, mode)


@pytest.mark.parametrize("case,variant", SLICE_RUNS)
def test_channel_slices(case, variant):
    """Both operands channel slices of wider buffers (zero-copy concat): x at channels 32.. of a
    buffer 64 wider, the output at channels 64.. of a buffer 96 wider (32 sentinel channels behind
    it), one sentinel image after the last."""
    _check_forward(case, variant, True, sliced=True)
    _check_data(case, variant, "mask_db", sliced=True)


@pytest.mark.parametrize("case", EQUAL_RUNS)
def test_variants_bitwise_equal(case):
    """launch_cd's variants share the accumulation order (see the module docstring)."""
    ys = [_run_forward(case, v, True) for v in (0, 1, 2)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    ds = [_run_data(case, v, "mask_db") for v in (0, 1, 2)]
    for dx, db in ds[1:]:
        assert torch.equal(ds[0][0], dx) and torch.equal(ds[0][1], db)
