"""The kernels that move data between the layers (csrc/kernels/copy_kernels.hip, layout_kernels.hip, reduce_kernels.hip), bit for bit against
the explicit-index references of tests/move_refs.py: both transposes, the weight flip (single and
multi), concat forward / backward, channel_copy and channel_copy8 in their three modes,
pad_interior (both widths), pad_rows, add_rows_f32, fanout, sum_bf16 (aliased, relu'-masked,
chained), cast, add, the NCHW <-> NHWC conversions, copy and zero.

A permutation, a copy and an op that rounds once can only be right or wrong bit for bit, so every
assertion is equality of the bit patterns, an exact zero, or an untouched guard: every written
tensor is a view into a sentinel-filled buffer (move_refs.Guarded), and an op that writes a channel
slice has the channels on both sides of the slice guarded as well.  test_move_refs_cpu.py runs
the same cases through the CPU executor."""
import pytest
import torch

import move_refs as mr
from cxxnet_amd import native, ops
from cxxnet_amd.ops import gemm, nn
from cxxnet_amd.ops.gemm import ConvGeom

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------ transposes
@pytest.mark.parametrize("case", mr.TRANSPOSE_TILED, ids=str)
def test_transpose_tiled(case):
    mr.check_transpose(case, DEV)


@pytest.mark.parametrize("case", mr.TRANSPOSE_ITEM, ids=str)
def test_transpose_per_item(case):
    B, R, Cc = case
    assert B >= 64 and Cc % 4 == 0 and R % 2 == 0 and R * (Cc + 2) * 2 <= 48 * 1024
    mr.check_transpose(case, DEV)


@pytest.mark.parametrize("case", mr.TRANSPOSE_FALLBACK, ids=str)
def test_transpose_per_item_declined(case):
    B, R, Cc = case
    assert B >= 64 and (Cc % 4 or R % 2 or R * (Cc + 2) * 2 > 48 * 1024)
    mr.check_transpose(case, DEV)


# ------------------------------------------------------------------ weight flip
def _flip_operands(case, seed):
    n = case[0] * case[1] * case[2] * case[3] * case[4]
    w = mr.ramp_bf16(n, start=seed)
    return w, mr.flat_guard(n, device=DEV)


def _flip_geom(case):
    G, Co, KH, KW, Ci = case
    return ConvGeom(1, KH, KW, G * Ci, 1, 1, G * Co, KH, KW, 1, 0, 0, G)


def _flip_multi(cases):
    ws, outs = [], []
    for i, case in enumerate(cases):
        w, wt = _flip_operands(case, 11 + 97 * i)
        ws.append(w)
        outs.append(wt)
    gemm.conv_weight_flip_multi([(w.to(DEV), wt.view, _flip_geom(case)) for w, wt, case in zip(ws, outs, cases)])
    torch.cuda.synchronize()
    for i, (w, wt, case) in enumerate(zip(ws, outs, cases)):
        what = "conv_weight_flip_multi tensor %d of %d %s" % (i, len(cases), case)
        wt.check(what)
        mr.assert_bits_equal(wt.view, mr.weight_flip_ref(w, *case), what)


@pytest.mark.parametrize("case", mr.FLIP_CASES, ids=str)
def test_weight_flip_single(case):
    w, wt = _flip_operands(case, 5)
    native.check(native.kernels().cxn_conv_weight_flip(w.to(DEV).data_ptr(), wt.view.data_ptr(), *case, gemm._stream()),
                 "conv_weight_flip")
    torch.cuda.synchronize()
    wt.check("conv_weight_flip %s" % (case,))
    mr.assert_bits_equal(wt.view, mr.weight_flip_ref(w, *case), "conv_weight_flip %s" % (case,))


@pytest.mark.parametrize("case", mr.FLIP_CASES, ids=str)
def test_weight_flip_multi_alone(case):
    _flip_multi([case])


def test_weight_flip_multi_every_case_in_one_launch():
    assert len(mr.FLIP_CASES) <= 64
    _flip_multi(mr.FLIP_CASES)


def test_weight_flip_multi_second_batch():
    """70 tensors: 64 in the first table, 6 in a second launch"""
    assert len(mr.FLIP_MANY) == 70
    _flip_multi(mr.FLIP_MANY)


# ------------------------------------------------------------------ concat
def _concat_inputs(cs, npix):
    ins = []
    for k, c in enumerate(cs):
        t = mr.relu_out_bf16((npix, c), 60 + k) if npix * c >= 64 else mr.rnd_bf16((npix, c), 60 + k)
        if npix * c < 64:
            t[0, 0], t[0, 1], t[0, 2] = 0.0, -0.0, 1.5  # an exact zero, a -0.0 and a live element all the same
        ins.append(t)
    return ins


@pytest.mark.parametrize("cs,npix", mr.CONCAT_CASES, ids=str)
def test_concat_forward(cs, npix):
    ins = [mr.ramp_bf16(npix * c, start=1000 * k + 1).view(npix, c) for k, c in enumerate(cs)]
    out = mr.flat_guard(npix * sum(cs), device=DEV)
    srcs = [mr.flat_guard(t.numel(), device=DEV, fill=t.reshape(-1)) for t in ins]
    assert ops.concat_channels([s.view.view(npix, c) for s, c in zip(srcs, cs)], out.view.view(npix, sum(cs))) is True
    torch.cuda.synchronize()
    out.check("concat forward %s" % (cs,))
    mr.assert_bits_equal(out.view.view(npix, sum(cs)), mr.concat_forward_ref(ins), "concat forward %s x %d" % (cs, npix))
    for s, t in zip(srcs, ins):
        s.check("concat forward input")
        mr.assert_bits_equal(s.view, t.reshape(-1), "concat forward changed an input")


@pytest.mark.parametrize("which", ["none", "first", "last", "all"])
@pytest.mark.parametrize("cs,npix", mr.CONCAT_CASES, ids=str)
def test_concat_backward(cs, npix, which):
    n = len(cs)
    mask = {"none": (), "first": (0,), "last": (n - 1,), "all": tuple(range(n))}[which]
    ins = _concat_inputs(cs, npix)
    g = mr.rnd_bf16((npix, sum(cs)), 70)
    g[0, 1] = -0.0  # a gradient of -0.0 passes an unmasked input bit for bit
    outg = mr.flat_guard(g.numel(), device=DEV, fill=g.reshape(-1))
    dsts = [mr.flat_guard(t.numel(), device=DEV, fill=t.reshape(-1)) for t in ins]
    assert ops.concat_channels([d.view.view(npix, c) for d, c in zip(dsts, cs)], outg.view.view(npix, sum(cs)),
                               backward=True, mask=mask) is True
    torch.cuda.synchronize()
    outg.check("concat backward gradient")
    mr.assert_bits_equal(outg.view, g.reshape(-1), "concat backward changed the output gradient")
    for k, (d, want) in enumerate(zip(dsts, mr.concat_backward_ref(g, ins, mask))):
        what = "concat backward %s x %d mask %s input %d" % (cs, npix, mask, k)
        d.check(what)
        got = d.view.view(npix, cs[k]).cpu()
        if k in mask:
            dead = ~(ins[k] > 0)
            assert bool(dead.any()) and int(torch.count_nonzero(got[dead])) == 0, what + ": masked element not 0"
        mr.assert_bits_equal(got, want, what)


def _declined(ins, out):
    before = [t.clone() for t in ins] + [out.clone()]
    for backward in (False, True):
        assert ops.concat_channels(ins, out, backward=backward) is False
    torch.cuda.synchronize()
    for t, b in zip(list(ins) + [out], before):
        mr.assert_bits_equal(t, b, "a declined concat wrote something")


def test_concat_declines_what_it_does_not_serve():
    npix = 9
    mk = lambda c, k: mr.ramp_bf16(npix * c, start=k).view(npix, c).to(DEV)
    _declined([mk(8, 1), mk(12, 2)], mk(20, 3))                      # a channel count that is no multiple of 8
    _declined([mk(8, k) for k in range(5)], mk(40, 9))               # five inputs
    flat = mr.ramp_bf16(npix * 8 + 8, start=4).to(DEV)
    _declined([flat[4:4 + npix * 8].view(npix, 8), mk(8, 5)], mk(16, 6))   # an input 8 bytes off a 16-byte boundary
    wide = mr.ramp_bf16(npix * 16 + 8, start=7).to(DEV)
    _declined([mk(8, 1), mk(8, 2)], wide[1:1 + npix * 16].view(npix, 16))   # the output 2 bytes off


# ------------------------------------------------------------------ channel copies
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", mr.CHANNEL_COPY_VECTOR, ids=str)
def test_channel_copy_vector(case, mode):
    assert all(v % 8 == 0 for v in case[:5]) and case[6] == 8
    mr.check_channel_copy(case, mode, DEV)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", mr.CHANNEL_COPY_SCALAR, ids=str)
def test_channel_copy_scalar(case, mode):
    assert any(v % 8 for v in case[:5]) or case[6] % 8
    mr.check_channel_copy(case, mode, DEV)


@pytest.mark.parametrize("extra", [8, 4])
def test_rows_contiguous(extra):
    """the [rows][C] channel slice of a wider buffer that the bias gradient copies out: a row stride
    of C + 8 (16-byte items) and of C + 4 (2-byte items)"""
    rows, C = 105, 24
    lo = 8 if extra == 8 else 4
    wide = mr.ramp_bf16(rows * (C + extra), start=3).view(rows, C + extra)
    d = wide.to(DEV)[:, lo:lo + C]
    assert d.stride(0) == C + extra and not d.is_contiguous()
    got = nn._rows_contiguous(d)
    torch.cuda.synchronize()
    assert got.is_contiguous()
    mr.assert_bits_equal(got, wide[:, lo:lo + C], "_rows_contiguous stride C + %d" % extra)


# ------------------------------------------------------------------ pads
@pytest.mark.parametrize("C", mr.PAD_INTERIOR_C)
@pytest.mark.parametrize("geo", mr.PAD_INTERIOR_GEOS, ids=str)
def test_pad_interior(geo, C):
    mr.check_pad_interior(geo, C, DEV)


def test_pad_interior_base_4_byte_aligned():
    """C = 4 would take the 8-byte units; a base that is 4-byte but not 8-byte aligned may not"""
    mr.check_pad_interior(mr.PAD_INTERIOR_GEOS[0], 4, DEV, lead=2)


@pytest.mark.parametrize("rows,L,Lp", mr.PAD_ROWS, ids=str)
def test_pad_rows(rows, L, Lp):
    src = mr.rnd_bf16((rows, L), 80)
    dst = mr.flat_guard(rows * Lp, device=DEV)
    native.check(native.kernels().cxn_pad_rows(src.to(DEV).data_ptr(), dst.view.data_ptr(), rows, L, Lp, gemm._stream()),
                 "pad_rows")
    torch.cuda.synchronize()
    dst.check("pad_rows")
    got = dst.view.view(rows, Lp).cpu()
    assert int(torch.count_nonzero(mr.bits(got[:, L:]))) == 0, "pad_rows: a tail is not exactly 0"
    mr.assert_bits_equal(got, mr.pad_rows_ref(src, rows, L, Lp), "pad_rows %s" % ((rows, L, Lp),))


@pytest.mark.parametrize("rows,L,Lp", mr.PAD_ROWS, ids=str)
def test_add_rows_f32(rows, L, Lp):
    """src rows of Ls = Lp elements whose tails hold a sentinel that must not leak, onto a non-zero dst"""
    g = torch.Generator().manual_seed(81)
    src = torch.randn(rows, Lp, generator=g)
    src[:, L:] = 1.0e30
    dst0 = torch.randn(rows, L, generator=g)
    dst = mr.flat_guard(rows * L, torch.float32, DEV, fill=dst0.reshape(-1))
    gemm._add_rows(src.to(DEV), dst.view, rows, L, Lp)
    torch.cuda.synchronize()
    dst.check("add_rows_f32")
    mr.assert_bits_equal(dst.view.view(rows, L), mr.add_rows_ref(src, dst0, rows, L, Lp), "add_rows_f32 %s" % ((rows, L, Lp),))


@pytest.mark.parametrize("rows,L", [(0, 8), (5, 0)])
def test_add_rows_f32_of_nothing(rows, L):
    src = torch.full((64,), 7.0, device=DEV)
    dst = mr.flat_guard(64, torch.float32, DEV, fill=torch.arange(64.0))
    gemm._add_rows(src, dst.view, rows, L, 8)
    torch.cuda.synchronize()
    dst.check("add_rows_f32 of nothing")
    mr.assert_bits_equal(dst.view, torch.arange(64.0), "add_rows_f32 of nothing")


# ------------------------------------------------------------------ split forward / backward
@pytest.mark.parametrize("n", mr.FAN_N)
@pytest.mark.parametrize("nd", mr.FAN_ND)
def test_fanout_copy(nd, n):
    mr.check_fanout(nd, n, DEV)


@pytest.mark.parametrize("alias", [False, True], ids=["apart", "aliased"])
@pytest.mark.parametrize("n", mr.FAN_N)
@pytest.mark.parametrize("nd", mr.FAN_ND)
def test_sum_into(nd, n, alias):
    mr.check_sum_into(nd, n, DEV, alias=alias)


@pytest.mark.parametrize("n", mr.FAN_N)
@pytest.mark.parametrize("nd", [1, 2, 4, 5])
def test_sum_into_masked(nd, n):
    """1: the channel copy; 2 and 4: the kernel; 5: the torch path, one rounding"""
    mr.check_sum_into(nd, n, DEV, mask_relu=True)


def test_fanout_and_sum_into_large():
    """more than 2^20 16-byte items: a second trip of the grid-stride loop"""
    mr.check_fanout(2, mr.FAN_BIG, DEV)
    mr.check_sum_into(2, mr.FAN_BIG, DEV, alias=True)


# ------------------------------------------------------------------ cast, add, layout, copy, zero
@pytest.mark.parametrize("n", mr.ELEMENTWISE_N)
def test_cast_and_add(n):
    mr.check_cast_add(n, DEV)


@pytest.mark.parametrize("case", mr.LAYOUT_CASES, ids=str)
def test_input_to_nhwc_and_back(case):
    mr.check_layout(case, DEV)


def test_nhwc_to_nchw_of_a_channel_slice():
    mr.check_nhwc_to_nchw_slice(DEV)


@pytest.mark.parametrize("n", mr.COPY_ELEMS)
def test_copy_and_zero(n):
    mr.check_copy_zero(n, DEV)
