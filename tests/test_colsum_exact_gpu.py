"""The column-sum kernels behind every bias gradient (colsum_multi with and without the column-chunk
split, colsum_bf16 + partials_reduce in deterministic mode, colsum_scalar), exactly.

Every case runs on integer inputs (tests/move_refs.py colsum_exact_inputs) whose magnitudes stay
below 2^24 per column, so every fp32 partial sum in any order, the atomics' included, is an exact
integer and the result must EQUAL the integer sum: one dropped row -- the last of a block, a tail
row behind the 8-deep unrolled loop -- fails at any row count.  The cases of up to 1500 rows run
on random inputs as well, inside the bias-gradient bound (R + 2) 2^-23 (sum |dy| + |db0|).  db0 is
non-zero everywhere and every db is a view into a sentinel-filled buffer.

The row counts sit on the edges the launcher computes (cxn_colsum_multi): with the split on a block
of CB = min(C / 8, 64) column vectors and RG = 256 // CB row groups takes
max(98304 / (CB * 8 * (3 masked, 2 not)), 8 RG) rows, and one unrolled round is 8 RG rows."""
import pytest
import torch

import move_refs as mr
from cxxnet_amd import native, ops
from cxxnet_amd.ops import gemm

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ids(cases):
    return ["c%d-r%d%s" % (c[0], c[1], "-" + c[2] if len(c) > 2 and c[2] else "") for c in cases]


def _report(what, worst):
    print("%s: max d/bound %.3g" % (what, worst))


# ------------------------------------------------------------------ colsum_multi, split on
@pytest.mark.parametrize("C,rows,kind", mr.COLSUM_MULTI, ids=_ids(mr.COLSUM_MULTI))
def test_colsum_multi_exact(C, rows, kind):
    assert ops.nn.bias_fast_ok(torch.empty(rows, C, dtype=mr.BF16, device=DEV)) and not gemm.deterministic()
    mr.check_bias_grad(C, rows, kind, DEV)


BOUNDED = [c for c in mr.COLSUM_MULTI if c[1] <= mr.COLSUM_BOUND_MAX_ROWS]


@pytest.mark.parametrize("C,rows,kind", BOUNDED, ids=_ids(BOUNDED))
def test_colsum_multi_bounded(C, rows, kind):
    _report("colsum_multi C %d rows %d mask %s" % (C, rows, kind), mr.check_bias_grad(C, rows, kind, DEV, exact=False))


def test_colsum_multi_every_case_in_one_call():
    assert len(mr.COLSUM_MULTI) <= 64
    mr.check_bias_grad_many(mr.COLSUM_MULTI, DEV)
    _report("colsum_multi, %d bounded segments in one call" % len(BOUNDED), mr.check_bias_grad_many(BOUNDED, DEV, exact=False))


def test_colsum_multi_second_batch():
    """70 segments, masked ones among them: 64 in the first table, 6 in a second launch"""
    assert len(mr.COLSUM_MANY) == 70
    mr.check_bias_grad_many(mr.COLSUM_MANY, DEV)


# ------------------------------------------------------------------ ld > C
@pytest.mark.parametrize("route", ["slice", "masked-slice", "odd-stride"])
@pytest.mark.parametrize("C,rows", mr.COLSUM_SLICE, ids=_ids(mr.COLSUM_SLICE))
def test_colsum_of_a_channel_slice(C, rows, route):
    """slice: read in place by colsum_multi (ld = C + 16).  masked-slice: copied out by
    _rows_contiguous first.  odd-stride: a row stride that is no multiple of 8 falls to bias_grad's
    copy and colsum_bf16.  The neighbour channels hold 1e30, which must not enter a sum."""
    mr.check_bias_grad_slice(C, rows, route, DEV)
    _report("bias gradient of a channel slice (%s) C %d rows %d" % (route, C, rows),
            mr.check_bias_grad_slice(C, rows, route, DEV, exact=False))


# ------------------------------------------------------------------ split off
@pytest.mark.parametrize("C,rows", mr.COLSUM_NOSPLIT, ids=_ids(mr.COLSUM_NOSPLIT))
def test_colsum_multi_without_the_chunk_split(C, rows):
    """one block walks the column chunks and reuses its LDS partials (C = 520: the last chunk is one
    vector wide, RG = 256)"""
    k = native.kernels()
    try:
        native.check(k.cxn_set_kernel_variant(1, 0), "variant")
        mr.check_bias_grad(C, rows, None, DEV)
        mr.check_bias_grad(C, rows, "some", DEV)
        _report("colsum_multi unsplit C %d rows %d" % (C, rows), mr.check_bias_grad(C, rows, None, DEV, exact=False))
    finally:
        native.check(k.cxn_set_kernel_variant(1, 1), "variant")


# ------------------------------------------------------------------ deterministic two-pass path, scalar columns
@pytest.mark.parametrize("C,rows", mr.COLSUM_DET, ids=_ids(mr.COLSUM_DET))
def test_colsum_deterministic(C, rows):
    """colsum_bf16 (512 rows to a block) + partials_reduce: exact on integers; on random inputs two
    runs are bitwise equal and inside the bound"""
    gemm.set_deterministic(True)  # (restored by the autouse fixture)
    mr.check_bias_grad(C, rows, None, DEV)
    dy, db0, _, expected = mr.colsum_case(C, rows, None, False)
    runs = []
    for _ in range(2):
        db = mr.flat_guard(C, torch.float32, DEV, fill=db0)
        ops.bias_grad(dy.to(DEV), db.view)
        torch.cuda.synchronize()
        _report("colsum deterministic C %d rows %d" % (C, rows), mr.assert_colsum(db, expected, False, "colsum deterministic"))
        runs.append(db.view.cpu())
    mr.assert_bits_equal(runs[0], runs[1], "two deterministic runs")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("C,rows", mr.COLSUM_SCALAR, ids=_ids(mr.COLSUM_SCALAR))
def test_colsum_scalar(C, rows, det):
    gemm.set_deterministic(det)
    assert C % 8
    mr.check_bias_grad(C, rows, None, DEV)
    _report("colsum_scalar C %d rows %d" % (C, rows), mr.check_bias_grad(C, rows, None, DEV, exact=False))
