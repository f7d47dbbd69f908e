"""The per-element net audit (tests/net_audit.py) on the GPU executor: one forward + backward pass
of two tiny nets at batch 3, every fusion NeuralNet._fuse can make of them switched on and off,
each observed value within its float64 bound (d / bound <= 1 at every connection, in every
direction).  The CXXNET_FUSE=0 variants show that the audit measures the conf's meaning and not
the fused layout, and pin a defect on the fusion when only a fused variant fails.

Worst d / bound per net and variant, measured on an MI355X (informational; the assertion is <= 1):
  net             variant          worst   fwd     bwd     dW      db
  alex_mini       default          0.980   0.978   0.980   0.094   0.074
  alex_mini       dgrad_bias       0.980   0.978   0.980   0.094   0.074
  alex_mini       unfused          0.988   0.978   0.988   0.094   0.000
  alex_mini       deterministic    0.980   0.978   0.980   0.094   0.000
  inception_mini  default          0.987   0.987   0.984   0.074   0.001
  inception_mini  copying_concat   0.995   0.987   0.995   0.074   0.000
  inception_mini  no_siblings      0.993   0.987   0.993   0.074   0.000
  inception_mini  unfused          0.993   0.987   0.993   0.074   0.000
  inception_mini  deterministic    0.987   0.987   0.984   0.074   0.001
  inception_mini  folded           0.996   0.996   0.993   0.090   0.000
(fwd and bwd sit just under 1: a bf16 store lands up to half an ulp from the float64 value, which is
all of u |ref|, the bound's leading term.  db 0.000: sums of so few bf16 terms are exact in fp32.)
"""
import pytest

import net_audit as NA

pytestmark = pytest.mark.gpu

ZERO = dict(fuse_relu=0, fused_into_producer=0, bias_of=0, bias_below=0, zero_copy=0, alias=0, fused_lrn=0,
            sib_groups=0)
# alex_mini: the relus of 3 convs and 2 fullcs and both dropouts fused, max-pool 1 -> LRN one kernel,
# both max-pools give their conv's bias gradient; CXXNET_DGRAD_BIAS=1: conv3's epilogue gives conv2's
ALEX = dict(ZERO, fuse_relu=5, fused_into_producer=7, bias_of=2, fused_lrn=1)
# inception_mini: 13 conv relus, both concats zero-copy, both splits aliased, one sibling group per
# module (1x1, 3x3 reduce, 5x5 reduce; without the zero-copy concat the 1x1 stays out: still one
# group), the stem's LRN gives the stem's bias gradient
INCEPTION = dict(ZERO, fuse_relu=13, fused_into_producer=13, zero_copy=2, alias=2, sib_groups=2, bias_of=1)

VARIANTS = [
    ("alex_mini", "default", {}, (), ALEX),
    ("alex_mini", "dgrad_bias", {"CXXNET_DGRAD_BIAS": "1"}, (), dict(ALEX, bias_below=1)),
    ("alex_mini", "unfused", {"CXXNET_FUSE": "0"}, (), ZERO),
    ("alex_mini", "deterministic", {}, (("deterministic", "1"),), ALEX),
    ("inception_mini", "default", {}, (), INCEPTION),
    ("inception_mini", "copying_concat", {"CXXNET_CONCAT_ZC": "0"}, (), dict(INCEPTION, zero_copy=0)),
    ("inception_mini", "no_siblings", {"CXXNET_FUSE_SIBLINGS": "0"}, (), dict(INCEPTION, sib_groups=0)),
    ("inception_mini", "unfused", {"CXXNET_FUSE": "0"}, (), ZERO),
    ("inception_mini", "deterministic", {}, (("deterministic", "1"),), INCEPTION),
]


def _counts(tr):
    c = NA.flag_counts(tr)
    c.pop("folded")
    return c


def _audit(tr, net, what):
    rep = NA.audit(tr, NA.make_batch(net))
    print("net_audit %s %s: worst d/bound %.3f %s" % (net, what, rep.net_worst(), {
        k: round(v, 3) for k, v in sorted(rep.by_direction().items())}))
    rep.assert_clean()
    assert rep.net_worst() <= 1.0
    convs = [i for i, c in enumerate(tr.net.connections) if c.layer.type_name in ("conv", "fullc")]
    for i in convs:
        assert {d for (j, d) in rep.worst if j == i} == {"fwd", "bwd", "dW", "db"}, i
    return rep


@pytest.mark.parametrize("net,what,env,extra,flags", VARIANTS, ids=["%s-%s" % v[:2] for v in VARIANTS])
def test_audit_on_the_gpu_executor(net, what, env, extra, flags, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = NA.make_trainer(net, "gpu", extra)
    assert _counts(tr) == flags
    for conn in tr.net.connections:  # small enough for weight_grad_ref, off the kernels' tiles
        if conn.layer.type_name == "conv":
            b, c, h, w = conn.nodes_out[0].shape
            assert b * h * w <= NA.K_MAX and c % 8 == 0 and h < 24 and w < 24, conn.nodes_out[0].shape
    _audit(tr, net, what)


def test_audit_with_the_split_sum_folded(monkeypatch):
    """The split's sum folded into the sibling group's data-gradient GEMM (ConvolutionLayer.backprop,
    ops.gemm.conv_backward_data_add).  The fold needs an LDS-DMA tile for the signature; the tuner's
    pick depends on timings, so tuning is off here and the heuristic tile serves (as in
    deterministic mode).  One whole update cycle runs first, as a step's first passes are the ones
    that settle tiles and lazy buffers; the audited pass must still fold."""
    from cxxnet_amd.ops import gemm
    gemm.set_glds(True, tune=False)  # (restored by conftest's _restore_gemm_modes)
    tr = NA.make_trainer("inception_mini", "gpu")
    assert _counts(tr) == INCEPTION
    for seed in (5, 6):
        tr.update(NA.make_batch("inception_mini", seed))
    assert NA.flag_counts(tr)["folded"] >= 1
    _audit(tr, "inception_mini", "folded")
    assert NA.flag_counts(tr)["folded"] >= 1
