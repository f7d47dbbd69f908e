"""The references of tests/move_refs.py against the CPU executor and against themselves.

Every case of the GPU tests (test_move_exact_gpu.py, test_colsum_exact_gpu.py,
test_image_input_bounds_gpu.py) runs here through the CPU branch of cxxnet_amd.ops under the same
equality or bound, which pins the references and the CPU executor to each other; the references of
ops without a CPU branch (weight flip, concat, pad_rows, add_rows) are compared with a second,
differently written torch formulation.  Then the conditions the GPU assertions rest on: the
exactness condition of every integer column-sum case, the validity of the image bound (an fp32
emulation of the kernel's arithmetic, unfused and fused, stays inside it) and the power of both
(a dropped row, a shifted mask, a mean read one column off, an ignored mirror, a dropped crop
offset or a neighbour's contrast must show)."""
import pytest
import torch

import move_refs as mr
from cxxnet_amd import ops

CPU = "cpu"


# ------------------------------------------------------------------ references against a second formulation
@pytest.mark.parametrize("case", mr.TRANSPOSE_TILED + mr.TRANSPOSE_ITEM + mr.TRANSPOSE_FALLBACK, ids=str)
def test_transpose(case):
    B, R, Cc = case
    x = mr.ramp_bf16(B * R * Cc, start=5)
    mr.assert_bits_equal(mr.transpose_ref(x, B, R, Cc), x.view(B, R, Cc).transpose(1, 2).reshape(-1))
    mr.check_transpose(case, CPU)


@pytest.mark.parametrize("case", mr.FLIP_CASES + mr.FLIP_MANY[:7], ids=str)
def test_weight_flip_reference(case):
    G, Co, KH, KW, Ci = case
    w = mr.ramp_bf16(G * Co * KH * KW * Ci, start=9)
    other = w.view(G, Co, KH, KW, Ci).flip(2, 3).permute(0, 4, 2, 3, 1).reshape(-1)
    mr.assert_bits_equal(mr.weight_flip_ref(w, *case), other)
    if KH * KW > 1 or Co != Ci:
        assert not torch.equal(mr.bits(mr.weight_flip_ref(w, *case)), mr.bits(w))


@pytest.mark.parametrize("cs,npix", [c for c in mr.CONCAT_CASES if c[1] <= 105], ids=str)
def test_concat_reference(cs, npix):
    ins = [mr.relu_out_bf16((npix, c), 60 + k) if npix * c >= 64 else mr.rnd_bf16((npix, c), 60 + k)
           for k, c in enumerate(cs)]
    out = mr.concat_forward_ref(ins)
    mr.assert_bits_equal(out, torch.cat(ins, 1))
    g = mr.rnd_bf16(tuple(out.shape), 70)
    for mask in [(), (0,), (len(cs) - 1,), tuple(range(len(cs)))]:
        back = mr.concat_backward_ref(g, ins, mask)
        for k, (b, piece) in enumerate(zip(back, torch.split(g, cs, 1))):
            want = piece * (ins[k] > 0) if k in mask else piece
            assert torch.equal(b.float() + 0.0, want.float() + 0.0)  # (+ 0.0: the sign of a masked zero aside)
            if k in mask:
                assert int(torch.count_nonzero(mr.bits(b)[~(ins[k] > 0)])) == 0  # +0 exactly
    # the CPU executor has no one-launch concat: it declines, and writes nothing
    o = torch.full_like(out, mr.SENTINEL)
    assert ops.concat_channels(ins, o) is False and bool((o == mr.SENTINEL).all())


@pytest.mark.parametrize("rows,L,Lp", mr.PAD_ROWS, ids=str)
def test_pad_and_add_rows_reference(rows, L, Lp):
    src = mr.rnd_bf16((rows, L), 80)
    want = torch.zeros(rows, Lp, dtype=mr.BF16)
    want[:, :L] = src
    mr.assert_bits_equal(mr.pad_rows_ref(src, rows, L, Lp), want)
    g = torch.Generator().manual_seed(81)
    s32, d32 = torch.randn(rows, Lp, generator=g), torch.randn(rows, L, generator=g)
    mr.assert_bits_equal(mr.add_rows_ref(s32, d32, rows, L, Lp), d32 + s32[:, :L])


# ------------------------------------------------------------------ the CPU executor under the GPU tests' assertions
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("case", mr.CHANNEL_COPY_VECTOR + mr.CHANNEL_COPY_SCALAR, ids=str)
def test_channel_copy(case, mode):
    mr.check_channel_copy(case, mode, CPU)


@pytest.mark.parametrize("n", mr.FAN_N)
@pytest.mark.parametrize("nd", mr.FAN_ND)
def test_fanout_and_sum_into(nd, n):
    mr.check_fanout(nd, n, CPU)
    mr.check_sum_into(nd, n, CPU)
    mr.check_sum_into(nd, n, CPU, alias=True)
    if nd in (1, 2, 4, 5):
        mr.check_sum_into(nd, n, CPU, mask_relu=True)


def test_fanout_and_sum_into_large():
    mr.check_fanout(2, mr.FAN_BIG, CPU)
    mr.check_sum_into(2, mr.FAN_BIG, CPU)


def test_sum_reference_chain():
    """the chain of groups of 4 rounds where one rounding would not: the two references must differ
    somewhere for more than 4 sources, and agree up to 4"""
    srcs = [mr.rnd_bf16((840,), 20 + k) for k in range(9)]
    assert torch.equal(mr.sum_ref(srcs[:4], group=4), mr.sum_ref(srcs[:4], group=None))
    assert not torch.equal(mr.sum_ref(srcs, group=4), mr.sum_ref(srcs, group=None))
    chain = mr.sum_ref([mr.sum_ref([mr.sum_ref(srcs[:4])] + srcs[4:7])] + srcs[7:])
    mr.assert_bits_equal(mr.sum_ref(srcs, group=4), chain)


@pytest.mark.parametrize("C", mr.PAD_INTERIOR_C)
@pytest.mark.parametrize("geo", mr.PAD_INTERIOR_GEOS, ids=str)
def test_pad_interior(geo, C):
    mr.check_pad_interior(geo, C, CPU)


@pytest.mark.parametrize("case", mr.LAYOUT_CASES, ids=str)
def test_layout(case):
    mr.check_layout(case, CPU)


def test_nhwc_to_nchw_of_a_channel_slice():
    mr.check_nhwc_to_nchw_slice(CPU)


@pytest.mark.parametrize("n", mr.ELEMENTWISE_N)
def test_cast_and_add(n):
    mr.check_cast_add(n, CPU)


@pytest.mark.parametrize("n", mr.COPY_ELEMS)
def test_copy_and_zero(n):
    mr.check_copy_zero(n, CPU)


def test_cast_inputs_hold_the_edges():
    x = mr.cast_inputs(4099)[-12:]
    y = mr.bits(mr.cast_ref(x)).tolist()
    u = [v & 0xFFFF for v in y]
    assert u[:4] == [0x3F80, 0x3F82, 0xBF80, 0xBF82]        # ties to even: down, up, and negative
    assert u[4:8] == [0x0000, 0x8000, 0x7F80, 0xFF80]       # +-0, +-inf
    assert u[8:] == [0x7F80, 0x7F7F, 0x3F81, 0x3F80]        # overflow to inf, largest finite, just off a tie


# ------------------------------------------------------------------ column sums
ALL_COLSUM = (mr.COLSUM_MULTI + [(C, r, None) for C, r in mr.COLSUM_SLICE + mr.COLSUM_NOSPLIT + mr.COLSUM_DET +
                                 mr.COLSUM_SCALAR] + [(C, r, "some") for C, r in mr.COLSUM_SLICE])
ALL_COLSUM = sorted(set(ALL_COLSUM), key=str)


def test_column_sum_case_lists():
    assert len(mr.COLSUM_MANY) == 70 and any(k for _, _, k in mr.COLSUM_MANY) and len(mr.COLSUM_MULTI) <= 64
    assert {k for _, _, k in mr.COLSUM_MULTI} == {None, "some", "all", "none"}


@pytest.mark.parametrize("C,rows,kind", ALL_COLSUM, ids=str)
def test_column_sum_exact_case(C, rows, kind):
    """the exactness condition (asserted inside colsum_exact_ref), the CPU executor, and the power of
    the expected value: a dropped last row, a dropped row 0 and a mask shifted by one row change it"""
    dy, db0, mask, want = mr.colsum_case(C, rows, kind, True)
    assert float((db0.abs() + dy.float().abs().sum(0)).max()) < 2 ** 24 and bool((db0 != 0).all())
    if rows > 1 and C >= 8:  # (three columns of -8 .. 8 cannot tell 700 rows apart by sign and digit alone)
        assert torch.unique(dy.float(), dim=0).shape[0] == rows  # no two rows equal
    mr.check_bias_grad(C, rows, kind, CPU)
    mr.check_bias_grad(C, rows, kind, CPU, multi=True)
    if kind != "all":  # (with every entry masked no row counts)
        for keep in (slice(0, rows - 1), slice(1, rows)):
            assert not torch.equal(mr.colsum_exact_ref(dy[keep], db0, mask[keep] if mask is not None else None), want)
    if kind == "some":
        shifted = torch.cat([torch.zeros(1, C, dtype=torch.uint8), mask[:-1]])
        assert not torch.equal(mr.colsum_exact_ref(dy, db0, shifted), want)
        assert 0.3 < float((mask >= 128).float().mean()) < 0.5 or rows * C < 512


@pytest.mark.parametrize("C,rows,kind", [c for c in ALL_COLSUM if c[1] <= mr.COLSUM_BOUND_MAX_ROWS], ids=str)
def test_column_sum_bounded_case(C, rows, kind):
    worst = mr.check_bias_grad(C, rows, kind, CPU, exact=False)
    print("column sum C %d rows %d mask %s: max d/bound %.3g" % (C, rows, kind, worst))


@pytest.mark.parametrize("route", ["slice", "masked-slice", "odd-stride"])
@pytest.mark.parametrize("C,rows", mr.COLSUM_SLICE, ids=str)
def test_column_sum_of_a_channel_slice(C, rows, route):
    mr.check_bias_grad_slice(C, rows, route, CPU)
    mr.check_bias_grad_slice(C, rows, route, CPU, exact=False)


def test_column_sums_in_one_call():
    mr.check_bias_grad_many(mr.COLSUM_MULTI, CPU)
    mr.check_bias_grad_many(mr.COLSUM_MANY, CPU)


# ------------------------------------------------------------------ image input stage
IMAGE = mr.image_cases()


@pytest.mark.parametrize("entry", IMAGE, ids=[e[0] for e in IMAGE])
def test_image_cpu_executor(entry):
    _, mode, B, h, w, C, Cp, Wp, _ = entry
    assert B >= 2
    worst = mr.check_image(mr.image_case_of(entry), Cp, Wp, CPU, "zero")
    if mode:
        print("image %s: max d/bound %.3f" % (entry[0], worst))


def test_image_row_padded_group_counts():
    groups = {B * h * (Wp // 4) for B, h, w, Wp in mr.IMAGE_ROWPAD}
    assert 64 in groups and 65 in groups and min(groups) < 64 and any(g % 256 == 1 for g in groups)
    assert {w for _, _, w, _ in mr.IMAGE_ROWPAD} == {1, 3, 4, 5, 7, 13, 227}
    assert all(Wp % 4 == 0 and B * h * w * 3 >= 16 for B, h, w, Wp in mr.IMAGE_ROWPAD)
    B, h, w, Wp = mr.IMAGE_ROWPAD_TINY
    assert B * h * w * 3 < 16


def test_image_bound_is_valid():
    """fp32 emulations of the kernels' arithmetic, unfused and with (d - m) * ct + il rounded once,
    stay inside the bound on every case"""
    import bounds
    worst = {False: 0.0, True: 0.0}
    for entry in IMAGE:
        if entry[1] == 0:
            continue
        case, Cp = mr.image_case_of(entry), entry[6]
        ref, bound = mr.image_bound_ref(case, Cp)
        for fused in (False, True):
            worst[fused] = max(worst[fused], bounds.assert_within(mr.image_emulate(case, Cp, fused), ref, bound,
                                                                  "%s fused %d" % (entry[0], fused), axes="bhwc"))
    print("image bound, emulation: max d/bound unfused %.3f, fused %.3f" % (worst[False], worst[True]))
    assert 0.3 < worst[False] <= 1.0 and 0.3 < worst[True] <= 1.0  # (a bound nothing comes near would have no power)


MUTATIONS = {"col+1": (2, 3), "nomirror": (2,), "nocrop": (2,), "ct_next": (1, 2, 3)}


@pytest.mark.parametrize("mutate", sorted(MUTATIONS))
def test_image_bound_has_power(mutate):
    """each defect violates the bound at 10 % or more of the elements it affects, on every case of
    the modes it applies to -- a condition on the inputs (mean image uniform in [0, 255], contrasts
    0.35 apart), checked on the defective emulation against the true reference and bound"""
    import bounds
    seen = set()
    for entry in IMAGE:
        mode, B, h, w, C, Cp = entry[1:7]
        if mode not in MUTATIONS[mutate]:
            continue
        case = mr.image_case_of(entry)
        ref, bound = mr.image_bound_ref(case, Cp)
        wrong = mr.image_bound_ref(case, Cp, mutate)[0].float().to(mr.BF16)  # the defective result, stored
        affected = torch.zeros(ref.shape, dtype=torch.bool)
        affected[..., :C] = True
        if mutate == "col+1":
            if w == 1:
                continue  # (a one-column image has no column to the right)
            affected[:, :, w - 1] = False if mode == 3 else affected[:, :, w - 1]  # clamped: unchanged in mode 3
        elif mutate == "nomirror":
            affected &= (case["prm"][:, 2] != 0).view(B, 1, 1, 1)
            if w % 2:
                affected[:, :, w // 2] = False  # the middle column mirrors onto itself
            if w == 1:
                continue
        elif mutate == "nocrop":
            affected &= ((case["prm"][:, 0] != 0) | (case["prm"][:, 1] != 0)).view(B, 1, 1, 1)
        n = int(affected.sum())
        assert n > 0, entry[0]
        bad = ~((wrong.double() - ref).abs() <= bound) & affected
        assert int(bad.sum()) >= 0.1 * n, "%s %s: only %d of %d affected elements violate the bound" % (
            entry[0], mutate, int(bad.sum()), n)
        assert bounds.violations(wrong, ref, bound)[0] > 0
        seen.add(mode)
    assert seen == set(MUTATIONS[mutate])
