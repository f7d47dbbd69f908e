"""Kernels of the layer batch_norm and of bias (csrc/kernels/layer_kernels.hip: chan_reduce, bn_mean,
bn_inv, bn_fwd, bn_bwd_coeffs, bn_bwd) element by element against the float64 references and the
derived bounds of tests/layer_bounds.py, through cxxnet_amd.ops.layer_ops as the layers call them.
The fp32 statistics are checked directly, so that a wrong statistic is not hidden under an
output's bf16 rounding.  Every output is the head of a sentinel-filled buffer; nothing behind it
may change.  The cases (tests/layer_cases.py BN_CASES) are the smallest that reach one idle row
lane, two and five row blocks with cross-block atomics, a second and a ragged last channel group,
mean / std ~ 50, and a constant channel.

Worst d / bound observed on an MI355X (`pytest -s` prints them per case):
  case    mean     inv      y      x-hat   dx     gslope   gbias       (the worse of the two eps)
  r3      0.12     0.075    0.93   0.82    0.88   0.051    0.051
  r98     0.0021   0.022    0.99   0.98    0.96   0.0022   0.0029
  c       0.0039   0.0098   0.84   0.74    0.85   0.0020   0.0035
  r257    0.00086  0.0068   0.98   0.99    0.97   0.00096  0.0012
  r1030   0.00037  0.0022   0.98   0.97    0.94   0.00027  0.00068
  const   0.0019   0.017    0.97   0.96    0.94   0.0019   0.0032
  deterministic mode: r257 inv 0.0067, gslope 0.0012; r1030 inv 0.0035, gslope 0.00050; the bf16
  outputs as above.  affine_forward: 0.995 (bias layer), 0.996 (general vectors).
The bf16 outputs sit just under 1 because the bound is the store itself there (a value just above a
power of two is moved by up to U of itself); the fp32 statistics show how much room the worst-case
summation bounds leave.  No kernel left a bound and no guard changed.
"""
import functools

import pytest
import torch

import layer_bounds as LB
import layer_cases as LC
from cxxnet_amd.ops import gemm
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
RUNS = pytest.mark.parametrize("name,eps", LC.BN_RUNS, ids=LC.BN_IDS)


@functools.lru_cache(maxsize=None)
def _refs(name, eps):
    c = LC.bn_inputs(name)
    fwd = LB.bn_forward_ref(c["x"], c["slope"], c["bias"], eps)
    bwd = LB.bn_backward_ref(c["gy"], c["x"], c["slope"], c["gs0"], c["gb0"], eps)
    return c, fwd, bwd


class Run:
    """Guarded device buffers of one case and the training forward."""

    def __init__(self, c):
        self.c = c
        R, C = c["R"], c["C"]
        self.xbuf, self.x = LC.guarded(c["x"], DEV)
        self.gbuf, self.g = LC.guarded(c["gy"], DEV)
        self.ybuf, self.y = LC.guarded_empty((R, C), torch.bfloat16, DEV)
        self.slope, self.bias = c["slope"].to(DEV), c["bias"].to(DEV)
        self.gsbuf, self.gs = LC.guarded(c["gs0"], DEV)
        self.gbbuf, self.gb = LC.guarded(c["gb0"], DEV)
        self.st = L.BNState(C, DEV)
        self.mbuf, self.st.mean = LC.guarded_empty((C,), torch.float32, DEV)
        self.ibuf, self.st.inv = LC.guarded_empty((C,), torch.float32, DEV)

    def forward(self, eps, train=True):
        if train:  # (bn_forward keeps a buffer of the input's shape)
            self.sbuf, self.st.xsave = LC.guarded_empty(tuple(self.x.shape), torch.bfloat16, DEV)
        L.bn_forward(self.x, self.y, self.slope, self.bias, eps, self.st, train)

    def guards(self):
        R, C = self.c["R"], self.c["C"]
        for what, buf, n in (("x", self.xbuf, R * C), ("g", self.gbuf, R * C), ("y", self.ybuf, R * C),
                             ("gslope", self.gsbuf, C), ("gbias", self.gbbuf, C), ("mean", self.mbuf, C),
                             ("inv", self.ibuf, C)):
            LC.assert_guard(buf, n, what)
        if getattr(self, "sbuf", None) is not None:
            LC.assert_guard(self.sbuf, R * C, "xsave")


def _report(tag, **worst):
    print("\n%s: worst d/bound %s" % (tag, "  ".join("%s %.3g" % kv for kv in worst.items())))


def _check_forward(r, fwd, tag, train=True):
    c = r.c
    w = dict(mean=LB.assert_within(r.st.mean, *fwd["mean"], "mean", axes="c"),
             inv=LB.assert_within(r.st.inv, *fwd["inv"], "inv", axes="c"),
             y=LB.assert_within(r.y, *fwd["y"], "y", axes="rc"))
    assert torch.isfinite(r.y.float()).all()
    if train:
        w["xhat"] = LB.assert_within(r.x, *fwd["xhat"], "x-hat in place of x", axes="rc")
        assert torch.equal(r.st.xsave.cpu(), c["x"]), "xsave must be the input, bit for bit"
    else:
        assert torch.equal(r.x.cpu(), c["x"]), "the test-time forward must leave the input alone"
        assert r.st.xsave is None
    r.guards()
    _report(tag, **w)


def _check_backward(r, bwd, dx, tag):
    w = dict(gslope=LB.assert_within(r.gs, *bwd["gslope"], "gslope", axes="c"),
             gbias=LB.assert_within(r.gb, *bwd["gbias"], "gbias", axes="c"))
    if dx is not None:
        w["dx"] = LB.assert_within(dx, *bwd["dx"], "dx", axes="rc")
        assert torch.isfinite(dx.float()).all()
    r.guards()
    _report(tag, **w)


@RUNS
def test_training_forward(name, eps):
    c, fwd, _ = _refs(name, eps)
    r = Run(c)
    r.forward(eps)
    _check_forward(r, fwd, "forward %s eps %g" % (name, eps))


@RUNS
def test_test_time_forward(name, eps):
    c, fwd, _ = _refs(name, eps)
    r = Run(c)
    r.forward(eps, train=False)
    _check_forward(r, fwd, "test-time forward %s eps %g" % (name, eps), train=False)


@RUNS
def test_backward_into_the_xhat_node(name, eps):
    """The layer's arrangement: dx overwrites the input node, which holds x-hat; gslope / gbias
    accumulate onto non-zero values."""
    c, _, bwd = _refs(name, eps)
    assert (c["gs0"] != 0).all() and (c["gb0"] != 0).all()
    r = Run(c)
    r.forward(eps)
    L.bn_backward(r.g, r.x, r.slope, r.gs, r.gb, r.st, True)
    _check_backward(r, bwd, r.x, "backward %s eps %g" % (name, eps))
    assert torch.equal(r.g.cpu(), c["gy"]), "the gradient must be left alone"


@RUNS
def test_backward_dx_aliasing_g(name, eps):
    c, fwd, bwd = _refs(name, eps)
    r = Run(c)
    r.forward(eps)
    L.bn_backward(r.g, r.g, r.slope, r.gs, r.gb, r.st, True)
    _check_backward(r, bwd, r.g, "backward in place %s eps %g" % (name, eps))
    LB.assert_within(r.x, *fwd["xhat"], "x-hat must survive a backward that writes elsewhere", axes="rc")


@RUNS
def test_backward_without_prop_grad(name, eps):
    c, _, bwd = _refs(name, eps)
    r = Run(c)
    r.forward(eps)
    xhat = r.x.clone()
    L.bn_backward(r.g, r.x, r.slope, r.gs, r.gb, r.st, False)
    _check_backward(r, bwd, None, "backward, weights only %s eps %g" % (name, eps))
    assert torch.equal(r.g.cpu(), c["gy"]) and torch.equal(r.x, xhat), "only the weight gradients may change"


@pytest.mark.parametrize("name", [n for n in LC.BN_CASES if n != "const"])
def test_affine_forward_as_the_bias_layer_uses_it(name):
    c = LC.bn_inputs(name)
    R, C = c["R"], c["C"]
    xbuf, x = LC.guarded(c["x"], DEV)
    ybuf, y = LC.guarded_empty((R, C), torch.bfloat16, DEV)
    zero, one = torch.zeros(C), torch.ones(C)
    L.affine_forward(x, y, zero.to(DEV), one.to(DEV), one.to(DEV), c["bias"].to(DEV))
    w = LB.assert_within(y, *LB.affine_ref(c["x"], zero, one, one, c["bias"]), "x + bias", axes="rc")
    # and with general vectors
    gen = torch.Generator().manual_seed(C)
    mean, inv, slope = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    L.affine_forward(x, y, mean.to(DEV), inv.to(DEV), slope.to(DEV), c["bias"].to(DEV))
    w2 = LB.assert_within(y, *LB.affine_ref(c["x"], mean, inv, slope, c["bias"]), "affine", axes="rc")
    assert torch.equal(x.cpu(), c["x"])
    LC.assert_guard(xbuf, R * C, "x")
    LC.assert_guard(ybuf, R * C, "y")
    _report("affine %s" % name, bias=w, general=w2)


@pytest.mark.parametrize("name", ["r257", "r1030"])
def test_deterministic_mode_is_inside_the_bounds_and_bitwise_reproducible(name):
    """cxn_deterministic: one block per channel group, no cross-block atomics."""
    eps = 1e-5
    c, fwd, bwd = _refs(name, eps)
    was = gemm._DET["on"]
    gemm.set_deterministic(True)
    try:
        runs = []
        for i in range(2):
            r = Run(c)
            r.forward(eps)
            xhat = r.x.clone()
            if i == 0:
                _check_forward(r, fwd, "deterministic forward %s" % name)
            L.bn_backward(r.g, r.x, r.slope, r.gs, r.gb, r.st, True)
            if i == 0:
                _check_backward(r, bwd, r.x, "deterministic backward %s" % name)
            runs.append([t.cpu().clone() for t in (r.y, r.st.mean, r.st.inv, xhat, r.x, r.gs, r.gb)])
        for a, b in zip(*runs):
            assert torch.equal(a, b)
    finally:
        gemm.set_deterministic(was)
