"""prelu, insanity, insanity_max_pooling (csrc/kernels/layer_kernels.hip), the activations and dropout
(csrc/kernels/act_kernels.hip) element by element against the float64 references and the derived
bounds of tests/layer_bounds.py, through the ops layer as the layers call them.  The random draws
are the package's counter hash (the generator); the operations are written out in the reference.
Every output is the head of a sentinel-filled buffer; nothing behind it may change.

Worst d / bound observed on an MI355X (`pytest -s` prints them per case):
  prelu (3, 8)      y 0.63   dx 0.87   gslope 0 (exact)
  prelu (75, 16)    y 0.95   dx 0.98   gslope 0.0071
  prelu (300, 72)   y 0.995  dx 0.99   gslope 0.00070
  insanity          y 0.98   dx 0.98        insanity_max_pooling  y, ysave exact; dx 0.98
  relu     y 0 (exact)  dx 0 (exact)        sigmoid  y 0.98  dx 0.995
  tanh     y 0.95       dx 0.99             xelu     y 0.79  dx 0.79
  dropout  y 0.97, the keep sets equal
(Just under 1 is the bf16 store itself.)  No kernel left a bound and no guard changed.
"""
import pytest
import torch

import layer_bounds as LB
import layer_cases as LC
from cxxnet_amd import ops
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(tag, **worst):
    print("\n%s: worst d/bound %s" % (tag, "  ".join("%s %.3g" % kv for kv in worst.items())))


def _counters(value, with_counter):
    """(device counter or None, its CPU twin for the reference)"""
    if not with_counter:
        return None, None
    return torch.tensor([value], dtype=torch.int32, device=DEV), torch.tensor([value], dtype=torch.int32)


# ------------------------------------------------------------------------------------ prelu
# every shape and noise with a device counter, and once without one
PRELU_RUNS = [(r, c, rnd, True) for r, c in LC.PRELU_SHAPES for rnd in LC.PRELU_RND] + [(75, 16, 0.3, False)]


@pytest.mark.parametrize("rows,C,rnd,with_counter", PRELU_RUNS)
def test_prelu(rows, C, rnd, with_counter):
    p = LC.prelu_inputs(rows, C)
    ctr, ctr_cpu = _counters(LC.PRELU_COUNTER, with_counter)
    n = rows * C
    xbuf, x = LC.guarded(p["x"], DEV)
    gbuf, gy = LC.guarded(p["gy"], DEV)
    ybuf, y = LC.guarded_empty((rows, C), torch.bfloat16, DEV)
    gsbuf, gs = LC.guarded(p["gs0"], DEV)
    slope = p["slope"].to(DEV)
    assert (p["slope"] < 0).any() and (p["slope"] > 1).any() and (p["gs0"] != 0).all()
    w = {}
    L.prelu_forward(x, y, slope, LC.PRELU_SEED, ctr, rnd)
    w["y"] = LB.assert_within(y, *LB.prelu_ref(p["x"], p["x"], p["slope"], rnd, LC.PRELU_SEED, ctr_cpu), "y", axes="rc")
    assert torch.equal(x.cpu(), p["x"])
    # weights only: x and g stay, gslope accumulates onto its non-zero start
    gs_ref = LB.prelu_gslope_ref(p["x"], p["gy"], p["gs0"])
    L.prelu_backward(x, gy, x, slope, gs, LC.PRELU_SEED, ctr, rnd, False)
    w["gslope"] = LB.assert_within(gs, *gs_ref, "gslope", axes="c")
    assert torch.equal(x.cpu(), p["x"]) and torch.equal(gy.cpu(), p["gy"])
    # dx written over x
    gs.copy_(p["gs0"])
    L.prelu_backward(x, gy, x, slope, gs, LC.PRELU_SEED, ctr, rnd, True)
    w["dx"] = LB.assert_within(x, *LB.prelu_ref(p["x"], p["gy"], p["slope"], rnd, LC.PRELU_SEED, ctr_cpu),
                               "dx in place of x", axes="rc")
    LB.assert_within(gs, *gs_ref, "gslope", axes="c")
    assert torch.equal(gy.cpu(), p["gy"])
    for what, buf, k in (("x", xbuf, n), ("g", gbuf, n), ("y", ybuf, n), ("gslope", gsbuf, C)):
        LC.assert_guard(buf, k, what)
    _report("prelu (%d, %d) rnd %g %s" % (rows, C, rnd, "counter" if with_counter else "no counter"), **w)


# ------------------------------------------------------------------------------------ insanity
@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
@pytest.mark.parametrize("n", LC.INSANITY_N)
def test_insanity(n, train):
    x0, g0 = LC.insanity_inputs(n)
    ctr, ctr_cpu = _counters(LC.INSANITY_COUNTER, True)
    args = (LC.INSANITY_LB, LC.INSANITY_UB, train, LC.INSANITY_SEED)
    xbuf, x = LC.guarded(x0, DEV)
    gbuf, gy = LC.guarded(g0, DEV)
    y2buf, y2 = LC.guarded_empty((n,), torch.bfloat16, DEV)
    L.insanity_forward(x, x, y2, *args, ctr)  # the layer's arrangement: y over x, and the output node
    w = {"y": LB.assert_within(x, *LB.insanity_ref(x0, x0, *args, ctr_cpu), "y", axes="i")}
    assert torch.equal(x, y2), "y2 must equal y bit for bit"
    y = x.cpu().clone()
    L.insanity_backward(x, gy, x, *args, ctr)  # dx over y
    w["dx"] = LB.assert_within(x, *LB.insanity_ref(y, g0, *args, ctr_cpu), "dx in place of y", axes="i")
    assert torch.equal(gy.cpu(), g0)
    for what, buf in (("x", xbuf), ("g", gbuf), ("y2", y2buf)):
        LC.assert_guard(buf, n, what)
    _report("insanity n %d %s" % (n, "train" if train else "test"), **w)


# ------------------------------------------------------------------------------------ insanity pooling
@pytest.mark.parametrize("keep", LC.INS_POOL_KEEP)
@pytest.mark.parametrize("shape", LC.INS_POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_insanity_max_pooling(shape, keep):
    N, H, W, C, K, S = shape
    x0, g0 = LC.ins_pool_inputs(*shape)
    Ho, Wo = g0.shape[1], g0.shape[2]
    ctr, ctr_cpu = _counters(LC.INS_POOL_COUNTER, True)
    xbuf, x = LC.guarded(x0, DEV)
    gbuf, gy = LC.guarded(g0, DEV)
    ybuf, y = LC.guarded_empty((N, Ho, Wo, C), torch.bfloat16, DEV)
    sbuf, ys = LC.guarded_empty((N, Ho, Wo, C), torch.bfloat16, DEV)
    dbuf, dx = LC.guarded_empty((N, H, W, C), torch.bfloat16, DEV)
    sh = LB.ins_pool_shifted(x0, keep, LC.INS_POOL_SEED, ctr_cpu)
    yref = LB.ins_pool_forward_ref(sh, K, S)
    L.ins_pool_forward(x, y, ys, K, S, keep, LC.INS_POOL_SEED, ctr)
    LB.assert_within(y, yref, torch.zeros_like(yref), "y (exact)")
    LB.assert_within(ys, yref, torch.zeros_like(yref), "ysave (exact)")
    L.ins_pool_backward(x, ys, gy, dx, K, S, keep, LC.INS_POOL_SEED, ctr)
    ref, bound = LB.ins_pool_backward_ref(sh, yref, g0, K, S)
    w = LB.assert_within(dx, ref, bound, "dx")
    assert bool((dx.cpu().double()[bound == 0] == 0).all()), "no window's max: exactly 0"
    assert torch.equal(x.cpu(), x0) and torch.equal(gy.cpu(), g0)
    for what, buf, k in (("x", xbuf, x0.numel()), ("g", gbuf, g0.numel()), ("y", ybuf, g0.numel()),
                         ("ysave", sbuf, g0.numel()), ("dx", dbuf, x0.numel())):
        LC.assert_guard(buf, k, what)
    _report("ins_pool %s keep %g" % (shape, keep), dx=w)


# ------------------------------------------------------------------------------------ activations
@pytest.mark.parametrize("n", LC.ACT_N)
@pytest.mark.parametrize("kind", LB.ACT_KINDS)
def test_activation(kind, n):
    x0, d0 = LC.act_inputs(n)
    fref, fbound = LB.act_forward_ref(kind, x0, LC.XELU_B)
    xbuf, x = LC.guarded(x0, DEV)
    ybuf, y = LC.guarded_empty((n,), torch.bfloat16, DEV)
    y2buf, y2 = LC.guarded_empty((n,), torch.bfloat16, DEV)
    ops.act_forward(kind, x, y, y2, b=LC.XELU_B)
    w = {"y": LB.assert_within(y, fref, fbound, "y", axes="i")}
    assert torch.equal(y, y2), "y2 must equal y bit for bit"
    assert torch.equal(x.cpu(), x0)
    ops.act_forward(kind, x, x, None, b=LC.XELU_B)  # in place
    assert torch.equal(x, y), "the in-place forward must give the same bits"
    ystored = y.cpu().clone()
    dbuf, dy = LC.guarded(d0, DEV)
    ops.act_backward(kind, y, dy, dy, b=LC.XELU_B)  # dx over dy
    w["dx"] = LB.assert_within(dy, *LB.act_backward_ref(kind, ystored, d0, LC.XELU_B), "dx in place of dy", axes="i")
    assert torch.equal(y.cpu(), ystored)
    assert not torch.isnan(y.float()).any() and not torch.isnan(dy.float()).any()
    for what, buf in (("x", xbuf), ("y", ybuf), ("y2", y2buf), ("dy", dbuf)):
        LC.assert_guard(buf, n, what)
    _report("%s n %d" % (kind, n), **w)


# ------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("with_counter", [True, False], ids=["counter", "nocounter"])
@pytest.mark.parametrize("pkeep", LC.DROPOUT_PKEEP)
@pytest.mark.parametrize("n", LC.DROPOUT_N)
def test_dropout(n, pkeep, with_counter):
    x0 = LC.dropout_inputs(n)
    ctr, ctr_cpu = _counters(LC.DROPOUT_COUNTER, with_counter)
    ref, bound, keep = LB.dropout_ref(x0, pkeep, LC.DROPOUT_SEED, ctr_cpu)
    xbuf, x = LC.guarded(x0, DEV)
    ybuf, y = LC.guarded_empty((n,), torch.bfloat16, DEV)
    ops.dropout_apply(x, y, LC.DROPOUT_SEED, pkeep, ctr)
    w = {"y": LB.assert_within(y, ref, bound, "y", axes="i")}
    live = x0.float() != 0
    assert torch.equal((y.cpu().float() != 0)[live], keep[live]), "the keep set must be the reference's exactly"
    assert torch.equal(x.cpu(), x0)
    ops.dropout_apply(x, x, LC.DROPOUT_SEED, pkeep, ctr)  # in place
    assert torch.equal(x, y), "the in-place call must give the same bits"
    LC.assert_guard(xbuf, n, "x")
    LC.assert_guard(ybuf, n, "y")
    _report("dropout n %d pkeep %g %s" % (n, pkeep, "counter" if with_counter else "no counter"), **w)
