"""The `relu6` / `hsigmoid` / `hswish` layers (type ids 43 / 44 / 45) on the CPU executor:
configuration, connection checks, forward and backward against the float64 references of
tests/hact_bounds.py, checkpoints, and the MobileNet-v3 conf."""
import numpy as np
import pytest
import torch

import hact_bounds as H

IDS = {"relu6": 43, "hsigmoid": 44, "hswish": 45}

# 4 x 6 x 6 input -> conv + bn + hswish -> a residual block whose branch is conv + bn + relu6 and an SE
# module gated by hsigmoid -> add -> avg pooling -> fullc -> softmax
NET = """
netconfig=start
layer[0->c0] = conv:c0
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[c0->n0] = batch_norm_ma:bn0
layer[n0->r0] = hswish:act0
layer[r0->a_x,a_id] = split
layer[a_x->a_c1] = conv:a_c1
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[a_c1->a_n1] = batch_norm_ma:a_bn1
layer[a_n1->a_r1] = relu6:act1
layer[a_r1->a_sq,a_ex] = split
layer[a_sq->a_gp] = avg_pooling
  kernel_size = 6
  stride = 1
layer[a_gp->a_gf] = flatten
layer[a_gf->a_g1] = fullc:a_fc1
  nhidden = 8
layer[a_g1->a_g2] = relu
layer[a_g2->a_g3] = fullc:a_fc2
  nhidden = 8
layer[a_g3->a_gs] = hsigmoid:gate
layer[a_ex,a_gs->a_se] = ch_scale:a_scale
layer[a_se,a_id->a] = add:a_add
  add_relu = 0
layer[a->gap] = avg_pooling
  kernel_size = 6
  stride = 1
layer[gap->flat] = flatten
layer[flat->fc] = fullc:fc
  nhidden = 5
layer[fc->fc] = softmax
netconfig=end
input_shape = 4,6,6
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
"""
B = 4


def _trainer(conf=NET, extra=(), seed=5):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf)) + [("batch_size", str(B)), ("dev", "cpu"), ("eval_train", "0"),
                                                        ("silent", "1"), ("seed", str(seed))] + list(extra):
        tr.set_param(k, v)
    return tr


def _make(*args, **kw):
    tr = _trainer(*args, **kw)
    tr.init_model()
    return tr


def _batch(seed, n=B, shape=(4, 6, 6), classes=5):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(n, *shape, generator=g), torch.randint(0, classes, (n, 1), generator=g).float())


def _raw(tr, batch):
    return tr.forward_to([len(tr.net.nodes) - 1], batch)[0].copy()


def _layer(tr, name):
    return tr.net.connections[tr.net_cfg.layer_name_map[name]].layer


def _params(tr):
    return [tr.net.arena.w[s.offset:s.offset + s.numel].detach().clone() for _, s in tr.net.arena.specs]


def _fresh(kind):
    from cxxnet_amd.layers import LayerContext, create_layer
    return create_layer(IDS[kind], LayerContext(torch.device("cpu")))


def _nodes(*shapes):
    from cxxnet_amd.layers import Node
    out = []
    for i, s in enumerate(shapes):
        n = Node("n%d" % i)
        n.set_shape(*s)
        out.append(n)
    return out


# ------------------------------------------------------------------ configuration
@pytest.mark.parametrize("kind", H.KINDS)
def test_type_id_name_and_flags(kind):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import neural_net
    tid = IDS[kind]
    assert native.rt().get_layer_type(kind) == tid
    assert native.rt().get_layer_type("pairtest-%s-%s" % (kind, kind)) == 1024 * tid + tid
    assert tid not in neural_net._SPLIT_SAFE
    lay = _fresh(kind)
    assert type(lay).__name__ == "HardActLayer" and lay.type_name == kind and lay.type_id == tid
    assert type(lay).__dict__["replay_audited"] is False and lay.replay_safe() is False
    lay.set_param("add_relu", "1")  # another layer's key: ignored
    lay.set_param("eta", "0.1")     # a global key: ignored
    assert lay.params == []


@pytest.mark.parametrize("kind", H.KINDS)
def test_connection_checks(kind):
    from cxxnet_amd.layers import Node
    x, x2 = _nodes((2, 3, 4, 5), (2, 3, 4, 5))
    o, o2 = Node("o"), Node("o2")
    for nin, nout in [([x, x2], [o]),      # two inputs
                      ([x], [o, o2]),      # two outputs
                      ([], [o]),
                      ([x], [])]:
        with pytest.raises(ValueError, match="HardActLayer"):
            _fresh(kind).init_connection(nin, nout)
    with pytest.raises(ValueError, match="self-loop"):  # layer[+0] = hswish
        _fresh(kind).init_connection([x], [x])
    (p,) = _nodes((2, 3, 4, 5))
    p.cp = 4  # a channel-padded map
    with pytest.raises(ValueError, match="padded-channel"):
        _fresh(kind).init_connection([p], [o])
    for shape in ((2, 3, 4, 5), (2, 1, 1, 7), (2, 6, 1, 1)):  # any shape: a map, a matrix node, a (B,C,1,1) node
        (n,) = _nodes(shape)
        o = Node("o")
        _fresh(kind).init_connection([n], [o])
        assert o.shape == shape and o.cp == shape[1]


def test_a_self_loop_in_a_conf_is_rejected_with_the_layer_named():
    conf = NET.replace("layer[n0->r0] = hswish:act0", "layer[n0->n0] = hswish:act0").replace("layer[r0->a_x,a_id]",
                                                                                            "layer[n0->a_x,a_id]")
    with pytest.raises(ValueError, match="HardActLayer: hswish .*self-loop"):
        _make(conf)


# ------------------------------------------------------------------ the layer's arithmetic
@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("kind", H.KINDS)
def test_forward_and_backward_match_the_float64_references(kind, alias):
    """fp32 nodes: the only error is the formulas' fp32 arithmetic, the eps32 part of the bounds of
    hact_bounds.py plus one eps32 |ref| (0 where the table gives a constant or a copy; relu6 is exact).
    alias: dx overwrites x (the usual in-place node), else it goes to a private gradient buffer."""
    n = 2 * 3 * 4 * 5
    xb, gb = H.inputs(n)
    x, o = _nodes((2, 3, 4, 5), (0, 0, 0, 0))
    lay = _fresh(kind)
    lay.init_connection([x], [o])
    for nd in (x, o):
        nd.alloc("cpu", torch.float32)
    x.data.copy_(xb.float().view(x.data.shape))
    if not alias:
        x.grad_buf = torch.full_like(x.data, 9.0)
    ys = []
    for is_train in (True, False):
        lay.forward(is_train, [x], [o])
        ys.append(o.data.clone())
    assert torch.equal(ys[0], ys[1])
    assert torch.equal(x.data.view(-1), xb.float())  # forward only reads x

    def fp32_bound(ref, bound):
        return torch.where(bound > 0, bound - H.U_BF16 * ref.abs() + H.EPS_F32 * ref.abs(), bound)

    ref, bound = H.forward_ref(kind, xb)
    H.assert_within(ys[0].view(-1), ref, fp32_bound(ref, bound), kind + " y", axes="i")
    o.data.copy_(gb.float().view(o.data.shape))  # the output node now holds the gradient
    lay.backprop(False, [x], [o])  # prop_grad = False writes nothing
    assert torch.equal(x.data.view(-1), xb.float())
    lay.backprop(True, [x], [o])
    ref, bound = H.backward_ref(kind, xb, gb)
    H.assert_within(x.gdst.view(-1), ref, fp32_bound(ref, bound), kind + " dx", axes="i")
    assert torch.equal(o.data.view(-1), gb.float())  # g is only read
    if not alias:
        assert torch.equal(x.data.view(-1), xb.float())
    if kind == "relu6":  # the sign of a zero too
        assert torch.equal(ys[0].view(-1).view(torch.int32), ref_f32_bits(H.forward_ref(kind, xb)[0]))


def ref_f32_bits(ref):
    return ref.float().view(torch.int32)


def test_ops_reject_an_unknown_kind_and_other_sizes():
    from cxxnet_amd.ops import layer_ops as L
    x = torch.zeros(2, 3)
    with pytest.raises(ValueError, match="hact"):
        L.hact_forward("swish", x, torch.zeros_like(x))
    with pytest.raises(ValueError, match="hact"):
        L.hact_forward("hswish", x, torch.zeros(2, 4))
    with pytest.raises(ValueError, match="hact"):
        L.hact_backward("relu6", x, torch.zeros(2, 4), x)
    g = torch.ones(2, 3)
    for kind in H.KINDS:  # y = x and dx = g are refused on every path; dx = x is the in-place gradient
        with pytest.raises(ValueError, match="alias"):
            L.hact_forward(kind, x, x)
        with pytest.raises(ValueError, match="alias"):
            L.hact_backward(kind, x, g, g)
        L.hact_backward(kind, x.clone(), g, x.clone())
    assert L.HACT_KINDS == H.KINDS


# ------------------------------------------------------------------ the executor
def test_the_output_is_not_marked_non_negative():
    conf = NET.replace("layer[a_r1->a_sq,a_ex] = split", "layer[a_r1->a_m] = max_pooling\n  kernel_size = 1\n"
                       "layer[a_m->a_sq,a_ex] = split")
    tr = _make(conf)
    pool = next(c.layer for c in tr.net.connections if c.type == 11)
    assert pool.input_nonneg is False


def test_splits_in_front_of_the_layers_keep_copying(monkeypatch):
    """not in _SPLIT_SAFE: with the graph fusion on, a split one of whose outputs feeds one of the
    layers is not made zero-copy"""
    monkeypatch.setenv("CXXNET_FUSE", "2")
    conf = NET.replace("layer[a_x->a_c1] = conv:a_c1", "layer[a_x->a_h] = hswish\nlayer[a_h->a_c1] = conv:a_c1")
    tr = _make(conf)
    sp = next(c for c in tr.net.connections if c.type == 23)
    assert sp.layer.alias is False and all(o.grad_buf is None for o in sp.nodes_out)
    tr.update(_batch(1))
    assert torch.isfinite(tr.net.arena.w).all()


def test_one_step_trains_every_branch():
    tr = _make()
    before = _params(tr)
    tr.update(_batch(1))
    after = _params(tr)
    keys = [(li, s.tag) for li, s in tr.net.arena.specs]
    assert len(keys) == 2 * 2 + 2 + 2 * 2 + 2  # two bn (slope, bias), two convs, the gate's fullc pair, fc
    for k, a, b in zip(keys, before, after):
        assert torch.isfinite(b).all() and not torch.equal(a, b), k
    out = _raw(tr, _batch(3))
    assert np.isfinite(out).all() and np.allclose(out.reshape(B, -1).sum(1), 1.0, atol=1e-5)


def test_smaller_batch_gives_the_same_rows():
    from cxxnet_amd.io.data import DataBatch
    tr = _make()
    tr.update(_batch(1))
    full = _batch(4)
    part = DataBatch(full.data[:3].clone(), full.label[:3].clone())
    want = _raw(tr, full)[:3]
    assert np.array_equal(_raw(tr, part), want)
    tr.update(part)
    tr.update(full)
    assert torch.isfinite(tr.net.arena.w).all()


# ------------------------------------------------------------------ checkpoints
def test_the_layers_write_nothing_into_the_model_file():
    from cxxnet_amd.layers.base import BinWriter
    tr = _make()
    for name, tid in (("act0", 45), ("act1", 43), ("gate", 44)):
        fo = BinWriter()
        _layer(tr, name).save_model(fo)
        assert fo.getvalue() == b""
        assert not hasattr(_layer(tr, name), "bind_state")
    tr.update(_batch(1))
    data = tr.save_model()
    tr2 = _trainer(seed=77)
    tr2.load_model(data)
    probe = _batch(9)
    assert np.array_equal(_raw(tr2, probe), _raw(tr, probe))
    assert tr2.save_model() == data
    for name, tid in (("act0", 45), ("act1", 43), ("gate", 44)):
        assert tr2.net_cfg.layers[tr2.net_cfg.layer_name_map[name]].type == tid


# ------------------------------------------------------------------ MobileNet-v3
@pytest.fixture(scope="module")
def mobilenet_v3():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("mobilenet_v3", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                           ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


# kernel, expansion, out, SE, hswish, stride: table 1 of the paper
TABLE = [(3, 16, 16, 0, 0, 1), (3, 64, 24, 0, 0, 2), (3, 72, 24, 0, 0, 1), (5, 72, 40, 1, 0, 2), (5, 120, 40, 1, 0, 1),
         (5, 120, 40, 1, 0, 1), (3, 240, 80, 0, 1, 2), (3, 200, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1),
         (3, 480, 112, 1, 1, 1), (3, 672, 112, 1, 1, 1), (5, 672, 160, 1, 1, 2), (5, 960, 160, 1, 1, 1),
         (5, 960, 160, 1, 1, 1)]


def test_mobilenet_v3_conf_builds(mobilenet_v3):
    net = mobilenet_v3.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    conns = net.connections
    types = [c.type for c in conns]
    dw = [c for c in conns if c.type == 10 and c.layer.lp.num_group > 1]
    assert len(dw) == 15
    got = [(c.layer.lp.kernel_height, c.layer.lp.num_channel, c.layer.lp.stride) for c in dw]
    assert got == [(k, e, s) for k, e, _, _, _, s in TABLE]
    assert all(c.layer.lp.num_group == c.layer.lp.num_channel == c.nodes_in[0].shape[1] for c in dw)
    assert all(c.layer.lp.pad_y == c.layer.lp.kernel_height // 2 for c in dw)
    # the stem, 14 expansions (the first block has none), 15 depthwise, 15 projections, the 960 conv
    assert types.count(10) == 1 + 14 + 15 + 15 + 1 == types.count(40)
    assert all(c.layer.lp.no_bias == 1 for c in conns if c.type == 10)
    assert types.count(42) == 8 == types.count(44)                       # SE modules, each gated by an hsigmoid
    # hswish: the stem, two per HS block, the 960 conv, the 1280 fullc; relu: one in block 1, two in
    # the other five RE blocks, one in each SE module
    assert types.count(45) == 1 + 2 * 9 + 1 + 1 == 21
    assert types.count(3) == 1 + 2 * 5 + 8 == 19
    assert types.count(43) == 0
    joins = [c for c in conns if c.type == 41]
    assert len(joins) == 10 and not any(c.layer.relu for c in joins)     # stride 1 and Cin = Cout
    assert [c.nodes_out[0].shape[1:] for c in joins] == [(16, 112, 112), (24, 56, 56), (40, 28, 28), (40, 28, 28)] + \
        [(80, 14, 14)] * 3 + [(112, 14, 14)] + [(160, 7, 7)] * 2
    assert types.count(23) == 10 + 8 and types.count(8) == 1 and types.count(2) == 1
    assert types.count(13) == 9  # the eight squeezes and the classifier's pooling
    for c in conns:  # every pooling is global and unpadded
        if c.type == 13:
            assert c.nodes_out[0].shape[2:] == (1, 1) and c.layer.lp.kernel_height == c.nodes_in[0].shape[2]
            assert c.layer.lp.pad_y == 0
    gates = [c.nodes_in[1].shape[1:] for c in conns if c.type == 42]
    maps = [c.nodes_in[0].shape[1:] for c in conns if c.type == 42]
    assert gates == [(1, 1, e) for _, e, _, se, _, _ in TABLE if se]
    assert maps == [(72, 28, 28), (120, 28, 28), (120, 28, 28), (480, 14, 14), (672, 14, 14), (672, 7, 7),
                    (960, 7, 7), (960, 7, 7)]
    widths = [c.layer.lp.num_hidden for c in conns if c.type == 1]
    assert widths[:-2:2] == [24, 32, 32, 120, 168, 168, 240, 240] and widths[-2:] == [1280, 1000]
    assert widths[1:-2:2] == [e for _, e, _, se, _, _ in TABLE if se]
    # the blocks end at the table's widths and resolutions
    outs = [net.nodes[mobilenet_v3.net_cfg.node_name_map["b%d" % i]].shape[1:] for i in range(1, 16)]
    hw, want = 112, []
    for _, _, co, _, _, s in TABLE:
        hw //= s
        want.append((co, hw, hw))
    assert outs == want
    nparam = sum(s.numel for _, s in net.arena.specs)
    assert 5.4e6 < nparam < 5.6e6  # the paper's 5.4 M (5,483,032 in the usual implementations)


def test_mobilenet_v3_one_training_step(mobilenet_v3):
    tr = mobilenet_v3
    b = _batch(1, n=2, shape=(3, 224, 224), classes=1000)
    before = tr.net.arena.w.clone()
    tr.update(b)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
