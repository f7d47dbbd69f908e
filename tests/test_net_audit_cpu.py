"""The per-element net audit (tests/net_audit.py) proves itself on the CPU executor: with bf16 at
the node boundaries both tiny nets pass with graph fusion forced on (CXXNET_FUSE=2) and off, each
net triggers the fusions it is meant to, and six planted defects -- one wrapped layer each -- are
caught at their own connection and direction and nowhere else."""
import pytest

import net_audit as NA
from test_bn_ma_net_gpu import _bf16_at_node_boundaries, _round

# what NeuralNet._fuse makes of each net on the CPU executor with CXXNET_FUSE=2 (no sibling groups
# and no pool -> LRN kernel there: both are GPU-only).  alex_mini: 3 conv + 2 fullc relus and the
# two dropouts fused, both max-pools give their conv's bias gradient.  inception_mini: 13 conv
# relus, both concats zero-copy, both splits aliased, the stem's LRN gives the stem's bias gradient.
CPU_FLAGS = {
    "alex_mini": dict(fuse_relu=5, fused_into_producer=7, bias_of=2, bias_below=0, zero_copy=0, alias=0,
                      fused_lrn=0, sib_groups=0),
    "inception_mini": dict(fuse_relu=13, fused_into_producer=13, bias_of=1, bias_below=0, zero_copy=2, alias=2,
                           fused_lrn=0, sib_groups=0),
}


def _trainer(net, fuse, monkeypatch, extra=()):
    monkeypatch.setenv("CXXNET_FUSE", fuse)
    tr = NA.make_trainer(net, "cpu", extra)
    _bf16_at_node_boundaries(tr)
    return tr


def _counts(tr):
    c = NA.flag_counts(tr)
    c.pop("folded")
    return c


@pytest.mark.parametrize("fuse", ["2", "0"])
@pytest.mark.parametrize("net", ["alex_mini", "inception_mini"])
def test_audit_passes_on_the_cpu_executor(net, fuse, monkeypatch):
    tr = _trainer(net, fuse, monkeypatch)
    want = CPU_FLAGS[net] if fuse == "2" else dict.fromkeys(CPU_FLAGS[net], 0)
    assert _counts(tr) == want
    rep = NA.audit(tr, NA.make_batch(net))
    print(net, "CXXNET_FUSE=" + fuse, "worst d/bound", rep.net_worst(), rep.by_direction())
    rep.assert_clean()
    # every conv / fullc was checked in all four directions, every other head in two
    convs = [i for i, c in enumerate(tr.net.connections) if c.layer.type_name in ("conv", "fullc")]
    for i in convs:
        assert {d for (j, d) in rep.worst if j == i} == {"fwd", "bwd", "dW", "db"}, i
    assert rep.net_worst() <= 1.0


def test_dgrad_bias_flag_on_the_cpu_executor(monkeypatch):
    monkeypatch.setenv("CXXNET_DGRAD_BIAS", "1")
    tr = _trainer("alex_mini", "2", monkeypatch)
    assert _counts(tr) == dict(CPU_FLAGS["alex_mini"], bias_below=1)  # conv3's epilogue for conv2
    NA.audit(tr, NA.make_batch("alex_mini")).assert_clean()


def _after(layer, which, fn):
    """Wrap layer.forward / layer.backprop (on the instance): fn(nodes_in, nodes_out) runs after it."""
    f0 = getattr(layer, which)

    def wrapped(flag, nin, nout):
        f0(flag, nin, nout)
        fn(nin, nout)
    setattr(layer, which, wrapped)


def _failed_at(rep):
    return [(f.conn, f.direction) for f in rep.failures]


def test_defect_a_fused_relu_mask_flipped(monkeypatch):
    """conv3 masks the gradient it writes into conv2's fused relu output; one dead element gets a
    value: caught at conv2's output gradient."""
    tr = _trainer("alex_mini", "2", monkeypatch)
    conv3 = NA.layer_of(tr, "conv3")
    assert conv3.grad_mask_relu
    dead = {}
    _after(conv3, "forward", lambda nin, nout: dead.update(idx=(nin[0].data == 0).nonzero()[0]))

    def flip(nin, nout):
        n, h, w, c = dead["idx"].tolist()
        nin[0].gdst[n, h, w, c] = 0.125
    _after(conv3, "backprop", flip)
    rep = NA.audit(tr, NA.make_batch("alex_mini"))
    assert _failed_at(rep) == [(NA.conn_of(tr, "conv2"), "bwd")], rep.failures
    n, h, w, c = dead["idx"].tolist()
    assert "(%d, %d, %d, %d)" % (n, h, w, c) in rep.failures[0].message


def test_defect_b_concat_input_eight_channels_off(monkeypatch):
    tr = _trainer("inception_mini", "0", monkeypatch)
    i = next(j for j, c in enumerate(tr.net.connections) if c.layer.type_name == "ch_concat")

    def shifted(nin, nout):
        nout[0].data[..., 16:32] = nin[1].data  # the 3x3 branch belongs at channels 8..24
    _after(tr.net.connections[i].layer, "forward", shifted)
    rep = NA.audit(tr, NA.make_batch("inception_mini"))
    assert _failed_at(rep) == [(i, "fwd")], rep.failures
    assert "c 16..31" in rep.failures[0].message


def test_defect_c_bias_gradient_from_the_unmasked_gradient(monkeypatch):
    tr = _trainer("alex_mini", "0", monkeypatch)
    i = NA.conn_of(tr, "conv2")
    relu, conv2 = tr.net.connections[i + 1].layer, tr.net.connections[i].layer
    assert relu.type_name == "relu"
    seen = {}
    b0 = relu.backprop

    def relu_bwd(prop_grad, nin, nout):
        seen["unmasked"] = nout[0].data.clone()
        b0(prop_grad, nin, nout)
    relu.backprop = relu_bwd

    def wrong_bias(nin, nout):
        conv2.b.g[5] = seen["unmasked"][..., 5].sum()
    _after(conv2, "backprop", wrong_bias)
    rep = NA.audit(tr, NA.make_batch("alex_mini"))
    assert _failed_at(rep) == [(i, "db")], rep.failures
    assert "(c)=(5,)" in rep.failures[0].message


def test_defect_d_split_sum_misses_a_branch_on_one_pixel(monkeypatch):
    """The first module's split leaves one branch out of its sum at one pixel: the stem LRN's output
    gradient (the split's input) is where the conf observes it."""
    tr = _trainer("inception_mini", "2", monkeypatch)
    i = next(j for j, c in enumerate(tr.net.connections) if c.layer.type_name == "split")
    assert tr.net.connections[i].layer.alias

    def short(nin, nout):
        g = nin[0].gdst
        g[2, 10, 8] -= nout[2].gdst[2, 10, 8]
        _round(g)
    _after(tr.net.connections[i].layer, "backprop", short)
    rep = NA.audit(tr, NA.make_batch("inception_mini"))
    assert _failed_at(rep) == [(i - 1, "bwd")], rep.failures
    assert tr.net.connections[i - 1].layer.type_name == "lrn"
    assert "n 2..2, h 10..10, w 8..8" in rep.failures[0].message


def test_defect_e_sibling_weight_gradient_rows_swapped(monkeypatch):
    """Two sibling 1x1 convs of one module (one stacked matrix on the GPU) exchange a row of their
    weight gradients: both members fail, each through its own arena spec."""
    tr = _trainer("inception_mini", "2", monkeypatch)
    a, b = NA.layer_of(tr, "a_1x1"), NA.layer_of(tr, "a_3x3r")

    def swap(nin, nout):  # a_1x1's backprop runs after a_3x3r's: both gradients are final
        row = a.w.g[7].clone()
        a.w.g[7] = b.w.g[0]
        b.w.g[0] = row
    _after(a, "backprop", swap)
    rep = NA.audit(tr, NA.make_batch("inception_mini"))
    assert _failed_at(rep) == [(NA.conn_of(tr, "a_1x1"), "dW"), (NA.conn_of(tr, "a_3x3r"), "dW")], rep.failures
    assert "o 7..7" in rep.failures[0].message and "o 0..0" in rep.failures[1].message


def test_defect_f_dropout_backward_mask_differs(monkeypatch):
    """The first dropout's backward drops one element the forward kept: caught at fc1's output
    gradient."""
    tr = _trainer("alex_mini", "0", monkeypatch)
    i = NA.conn_of(tr, "fc1")
    drop = tr.net.connections[i + 2].layer
    assert drop.type_name == "dropout"
    kept = {}
    _after(drop, "forward", lambda nin, nout: kept.update(fwd=nin[0].data > 0))

    def other_mask(nin, nout):
        g = nin[0].data
        live = (kept["fwd"] & (g != 0)).nonzero()
        kept["idx"] = live[0].tolist()
        g[tuple(kept["idx"])] = 0
    _after(drop, "backprop", other_mask)
    rep = NA.audit(tr, NA.make_batch("alex_mini"))
    assert _failed_at(rep) == [(i, "bwd")], rep.failures
    assert "(%d, %d, %d, %d)" % tuple(kept["idx"]) in rep.failures[0].message
