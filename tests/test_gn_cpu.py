"""The `group_norm` layer (type id 46) on the CPU executor: configuration and connection checks,
forward and backward against an independent float64 group norm and against central differences,
checkpoints, independence from the batch, and the ResNet-18-GN conf."""
import struct

import numpy as np
import pytest
import torch

# 4 x 6 x 6 input -> conv -> group_norm (2 groups of 4) -> relu -> pooling -> fullc -> group_norm with
# one group (layer norm) -> fullc -> softmax
NET = """
netconfig=start
layer[0->c0] = conv:c0
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[c0->n0] = group_norm:gn0
  gn_group = 2
  init_slope = 1.5
  init_bias = 0.25
layer[n0->r0] = relu
layer[r0->p0] = max_pooling
  kernel_size = 2
  stride = 2
layer[p0->f0] = flatten
layer[f0->h1] = fullc:f1
  nhidden = 6
layer[h1->n1] = group_norm:gn1
  gn_group = 1
layer[n1->out] = fullc:f2
  nhidden = 5
layer[out->out] = softmax
netconfig=end
input_shape = 4,6,6
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
"""
B = 4


def _trainer(conf=NET, extra=(), seed=5, batch=B):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf)) + [("batch_size", str(batch)), ("dev", "cpu"), ("eval_train", "0"),
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


def _fresh(**keys):
    from cxxnet_amd.layers import LayerContext, create_layer
    lay = create_layer(46, LayerContext(torch.device("cpu")))
    for k, v in keys.items():
        lay.set_param(k, str(v))
    return lay


def _nodes(*shapes):
    from cxxnet_amd.layers import Node
    out = []
    for i, s in enumerate(shapes):
        n = Node("n%d" % i)
        n.set_shape(*s)
        out.append(n)
    return out


def _gn64(x, slope, bias, groups, eps):
    """Independent float64 group norm of an NCHW tensor."""
    return torch.nn.functional.group_norm(x.double(), groups, slope.double(), bias.double(), eps)


# ------------------------------------------------------------------ configuration
def test_type_id_name_and_flags():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("group_norm") == 46
    lay = _fresh()
    assert type(lay).__name__ == "GroupNormLayer" and lay.type_name == "group_norm" and lay.type_id == 46
    assert type(lay).__dict__["replay_audited"] is False and lay.replay_safe() is False
    assert not hasattr(lay, "state_numel") and not hasattr(lay, "bind_state")


def test_defaults_and_keys():
    from cxxnet_amd.layers import Node
    (x,) = _nodes((2, 64, 3, 3))
    lay = _fresh(ngroup=4)  # the conv key, as a global setting would hand it over: not this layer's
    lay.init_connection([x], [Node("o")])
    assert lay.groups == 32 and lay.eps == 1e-5 and lay.init_slope == 1.0 and lay.init_bias == 0.0
    assert [(p.tag, p.shape) for p in lay.params] == [("wmat", (64,)), ("bias", (64,))]
    lay = _fresh(gn_group=8, eps=1e-3, init_slope=2, init_bias=-1)
    o = Node("o")
    lay.init_connection([x], [o])
    assert lay.groups == 8 and lay.eps == 1e-3 and lay.init_slope == 2.0 and lay.init_bias == -1.0
    assert o.shape == x.shape and o.cp == 64
    (m,) = _nodes((2, 1, 1, 10))  # a matrix node: HW = 1, C = the features
    lay = _fresh(gn_group=5)
    lay.init_connection([m], [Node("o")])
    assert (lay.hw, lay.channel, lay.groups) == (1, 10, 5)


@pytest.mark.parametrize("bad", ["4", "0", "-2", "2.5", "x"])
def test_gn_group_must_be_a_positive_divisor_of_the_channels(bad):
    from cxxnet_amd.layers import Node
    (x,) = _nodes((2, 6, 3, 3))
    with pytest.raises(ValueError, match="GroupNormLayer: gn_group"):
        _fresh(gn_group=bad).init_connection([x], [Node("o")])


def test_the_default_of_32_groups_must_divide_too():
    from cxxnet_amd.layers import Node
    (x,) = _nodes((2, 48, 3, 3))
    with pytest.raises(ValueError, match="GroupNormLayer: gn_group = 32"):
        _fresh().init_connection([x], [Node("o")])


def test_connection_checks():
    from cxxnet_amd.layers import Node
    x, x2 = _nodes((2, 6, 4, 5), (2, 6, 4, 5))
    o, o2 = Node("o"), Node("o2")
    for nin, nout in [([x, x2], [o]), ([x], [o, o2]), ([], [o]), ([x], [])]:
        with pytest.raises(ValueError, match="GroupNormLayer"):
            _fresh(gn_group=3).init_connection(nin, nout)
    with pytest.raises(ValueError, match="GroupNormLayer: .*self-loop"):
        _fresh(gn_group=3).init_connection([x], [x])
    (p,) = _nodes((2, 6, 4, 5))
    p.cp = 8  # a channel-padded map
    with pytest.raises(ValueError, match="GroupNormLayer: padded-channel"):
        _fresh(gn_group=3).init_connection([p], [o])


def test_a_self_loop_in_a_conf_is_rejected_with_the_layer_named():
    conf = NET.replace("layer[h1->n1] = group_norm:gn1", "layer[h1->h1] = group_norm:gn1").replace("layer[n1->out]",
                                                                                                 "layer[h1->out]")
    with pytest.raises(ValueError, match="GroupNormLayer: .*self-loop"):
        _make(conf)


# ------------------------------------------------------------------ the layer's arithmetic
def _run_layer(x_nchw, gy_nchw, groups, slope, bias, prop_grad=True, alias=True, eps=1e-5):
    """The layer on fp32 CPU nodes -> (y, dx, gslope, gbias), NCHW."""
    Bn, C, H, W = x_nchw.shape
    x, o = _nodes((Bn, C, H, W), (0, 0, 0, 0))
    lay = _fresh(gn_group=groups, eps=eps)
    lay.init_connection([x], [o])
    for nd in (x, o):
        nd.alloc("cpu", torch.float32)
    for p, v in zip(lay.params, (slope, bias)):
        p.w, p.g = v.clone().float(), torch.zeros(C)
    x.data.copy_(x_nchw.permute(0, 2, 3, 1))
    if not alias:
        x.grad_buf = torch.full_like(x.data, 9.0)
    ys = []
    for is_train in (True, False):
        lay.forward(is_train, [x], [o])
        ys.append(o.data.clone())
    assert torch.equal(ys[0], ys[1]), "forward must not depend on is_train"
    assert torch.equal(x.data, x_nchw.permute(0, 2, 3, 1)), "forward only reads x"
    o.data.copy_(gy_nchw.permute(0, 2, 3, 1))
    lay.backprop(prop_grad, [x], [o])
    return ys[0].permute(0, 3, 1, 2), x.gdst.permute(0, 3, 1, 2).clone(), lay.params[0].g, lay.params[1].g, x


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("shape,groups", [((2, 6, 3, 3), 3), ((3, 8, 5, 4), 1), ((2, 8, 2, 2), 8), ((4, 12, 1, 1), 4)])
def test_forward_and_backward_match_float64_autograd(shape, groups, alias):
    gen = torch.Generator().manual_seed(shape[1])
    x = torch.randn(*shape, generator=gen) * 1.5 + 0.5
    gy = torch.randn(*shape, generator=gen)
    C = shape[1]
    slope, bias = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xd = x.double().requires_grad_()
    sd, bd = slope.double().requires_grad_(), bias.double().requires_grad_()
    yd = _gn64(xd, sd, bd, groups, 1e-5)
    yd.backward(gy.double())
    y, dx, gslope, gbias, _ = _run_layer(x, gy, groups, slope, bias, alias=alias)

    def close(a, b):
        return torch.allclose(a.double(), b, rtol=1e-5, atol=2e-5 * b.abs().max().item())
    assert close(y, yd.detach())
    assert close(dx, xd.grad)
    assert close(gslope, sd.grad)
    assert close(gbias, bd.grad)


def test_without_prop_grad_only_the_weight_gradients_move():
    gen = torch.Generator().manual_seed(1)
    x, gy = torch.randn(2, 6, 3, 3, generator=gen), torch.randn(2, 6, 3, 3, generator=gen)
    _, _, gslope, gbias, node = _run_layer(x, gy, 3, torch.ones(6), torch.zeros(6), prop_grad=False)
    assert torch.equal(node.data, x.permute(0, 2, 3, 1))
    assert gslope.abs().sum() > 0 and gbias.abs().sum() > 0


def test_matrix_node_is_layer_norm_over_the_features():
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(3, 1, 1, 10, generator=gen)
    n, o = _nodes((3, 1, 1, 10), (0, 0, 0, 0))
    lay = _fresh(gn_group=1)
    lay.init_connection([n], [o])
    for nd in (n, o):
        nd.alloc("cpu", torch.float32)
    lay.params[0].w, lay.params[1].w = torch.ones(10), torch.zeros(10)
    n.data.view(3, 10).copy_(x.view(3, 10))
    lay.forward(True, [n], [o])
    want = torch.nn.functional.layer_norm(x.view(3, 10).double(), (10,), eps=1e-5)
    assert torch.allclose(o.data.view(3, 10).double(), want, rtol=1e-5, atol=1e-5)


def test_central_difference_gradients():
    """dx, gslope and gbias of the layer against central differences of its own forward, in the
    loss sum(y w) on a (2, 6, 3, 3) node with gn_group = 3.  The forward is fp32, so h = 2^-6 and the
    tolerance are set for a difference quotient of fp32 values: its rounding error is about
    |y| 2^-24 sum|w| / h ~ 1e-4 and its truncation error h^2 f''' / 6 ~ 1e-4."""
    gen = torch.Generator().manual_seed(3)
    shape, groups = (2, 6, 3, 3), 3
    x = torch.randn(*shape, generator=gen)
    w = torch.randn(*shape, generator=gen)
    slope, bias = torch.rand(6, generator=gen) + 0.5, torch.randn(6, generator=gen)
    _, dx, gslope, gbias, _ = _run_layer(x, w, groups, slope, bias, alias=False, eps=1e-2)
    h = 2.0 ** -6

    def loss(xv, sv, bv):
        y = _run_layer(xv, w, groups, sv, bv, alias=False, eps=1e-2)[0]
        return (y.double() * w.double()).sum().item()

    def quotient(which, idx):
        args = [x.clone(), slope.clone(), bias.clone()]
        args[which][idx] += h
        up = loss(*args)
        args[which][idx] -= 2 * h
        return (up - loss(*args)) / (2 * h)
    tol = 2e-3
    for idx in [(0, 0, 0, 0), (0, 1, 2, 1), (1, 5, 2, 2), (1, 2, 0, 1), (0, 3, 1, 1)]:
        assert abs(quotient(0, idx) - dx[idx].item()) < tol, idx
    for c in range(6):
        assert abs(quotient(1, (c,)) - gslope[c].item()) < tol, c
        assert abs(quotient(2, (c,)) - gbias[c].item()) < tol, c


def test_ops_reject_bad_arguments():
    from cxxnet_amd.ops import layer_ops as L
    st = L.GNState(2, 3, 6, 3, "cpu")
    assert st.mean.shape == (2, 3) and st.rstd.shape == (2, 3) and st.ws is None
    x = torch.zeros(2, 3, 6)
    with pytest.raises(ValueError, match="alias"):
        L.gn_forward(x, x, torch.ones(6), torch.zeros(6), 1e-5, st)
    with pytest.raises(ValueError, match="gn_forward"):
        L.gn_forward(torch.zeros(3, 3, 6), torch.zeros(3, 3, 6), torch.ones(6), torch.zeros(6), 1e-5, st)  # B > max


# ------------------------------------------------------------------ the executor
def test_the_net_matches_float64_group_norm_at_both_layers():
    tr = _make()
    b = _batch(2)
    tr._set_batch(b)
    tr.net.forward(True)
    nm = tr.net_cfg.node_name_map
    for name, src, dst, groups in (("gn0", "c0", "n0", 2), ("gn1", "h1", "n1", 1)):
        lay = _layer(tr, name)
        xin, y = tr.net.nodes[nm[src]].data, tr.net.nodes[nm[dst]].data
        C = lay.channel
        want = _gn64(xin.reshape(B, -1, C).permute(0, 2, 1), lay.params[0].w, lay.params[1].w, groups, 1e-5)
        if name == "gn0":  # the relu behind it works in place: n0 holds relu(y) by now
            want = want.clamp_min(0)
        assert torch.allclose(y.reshape(B, -1, C).permute(0, 2, 1).double(), want, rtol=1e-5, atol=1e-5), name
    g0 = _layer(tr, "gn0")
    assert torch.equal(g0.params[0].w, torch.full((8,), 1.5)) and torch.equal(g0.params[1].w, torch.full((8,), 0.25))


def test_no_running_state():
    tr = _make()
    assert tr.net.bn_state is None
    tr.update(_batch(1))
    assert tr.net.bn_state is None and not tr.net.ctx.bn_dirty


def test_one_step_trains_every_parameter():
    tr = _make()
    specs = tr.net.arena.specs
    before = [tr.net.arena.w[s.offset:s.offset + s.numel].clone() for _, s in specs]
    tr.update(_batch(1))
    assert len(specs) == 1 + 2 + 2 + 2 + 2  # conv, gn0 (slope, bias), f1 (w, b), gn1, f2
    for (li, s), a in zip(specs, before):
        b = tr.net.arena.w[s.offset:s.offset + s.numel]
        if (li, s.tag) == (tr.net_cfg.layer_name_map["f1"], "bias"):
            continue  # a layer norm follows: the bias of f1 has a zero gradient, up to rounding
        assert torch.isfinite(b).all() and not torch.equal(a, b), (li, s.tag)


def test_pred_of_a_row_is_identical_alone_and_inside_a_batch():
    from cxxnet_amd.io.data import DataBatch
    tr = _make()
    for seed in (1, 2):
        tr.update(_batch(seed))
    a, b = _batch(5), _batch(6)
    b.data[0] = a.data[0]
    ya, yb = _raw(tr, a), _raw(tr, b)
    assert np.array_equal(ya[0], yb[0]) and not np.array_equal(ya[1], yb[1])
    assert tr.predict(a)[0] == tr.predict(b)[0]
    one = DataBatch(a.data[:1].clone(), a.label[:1].clone())
    # alone, through adjust_batch_size (torch's CPU GEMMs block a batch of 1 differently: last-bit
    # differences in the raw output come from fullc / conv, so the raw row is compared to 1e-6)
    assert tr.predict(one)[0] == tr.predict(a)[0]
    assert np.allclose(_raw(tr, one)[0], ya[0], rtol=0, atol=1e-6)
    # and in training mode: the statistics are per sample
    outs = []
    for bt in (a, b):
        tr._set_batch(bt)
        tr.net.forward(True)
        outs.append(tr.net.nodes[-1].data[0].clone())
    assert torch.equal(outs[0], outs[1])
    part = DataBatch(a.data[:3].clone(), a.label[:3].clone())
    tr.update(part)  # a smaller last batch trains with the buffers of the largest
    tr.update(a)
    assert torch.isfinite(tr.net.arena.w).all()


# ------------------------------------------------------------------ checkpoints
def _tensors(blob, pos, n):
    out = []
    for _ in range(n):
        (ln,) = struct.unpack_from("<I", blob, pos)
        out.append(np.frombuffer(blob, "<f4", ln, pos + 4).copy())
        pos += 4 + 4 * ln
    return out, pos


def test_checkpoint_round_trip_and_layout():
    tr = _make()
    for seed in (1, 2):
        tr.update(_batch(seed))
    data = tr.save_model()
    probe = _batch(9)
    want = _raw(tr, probe)
    tr2 = _trainer(seed=77)
    tr2.load_model(data)
    assert np.array_equal(_raw(tr2, probe), want)
    assert np.array_equal(tr2.predict(probe), tr.predict(probe))
    assert tr2.save_model() == data
    assert tr2.net_cfg.layers[tr2.net_cfg.layer_name_map["gn0"]].type == 46
    assert tr2.net.bn_state is None
    # the layer's blob: slope then bias, two 1-D tensors and nothing else
    from cxxnet_amd.layers.base import BinWriter
    gn = _layer(tr, "gn0")
    fo = BinWriter()
    gn.save_model(fo)
    blob = fo.getvalue()
    got, end = _tensors(blob, 0, 2)
    assert end == len(blob)
    for t, ref in zip(got, (gn.params[0].w, gn.params[1].w)):
        assert t.shape == (8,) and np.array_equal(t, ref.numpy())
    assert not np.array_equal(got[0], np.full(8, 1.5, np.float32))  # trained values, not the initial ones


# ------------------------------------------------------------------ ResNet-18-GN
def test_resnet18_gn_is_resnet18_with_group_norm():
    from cxxnet_amd.models import available, load_conf
    assert "resnet18_gn" in available()

    def layers(name):
        return [(k, v) for k, v in load_conf(name) if k.startswith("layer[")]
    ref, gn = layers("resnet18"), layers("resnet18_gn")
    assert len(ref) == len(gn)
    n = 0
    for (ka, va), (kb, vb) in zip(ref, gn):
        assert ka == kb
        if va.startswith("batch_norm_ma"):
            assert vb.startswith("group_norm")
            n += 1
        else:
            assert va == vb
    assert n == 20
    other = [(k, v) for k, v in load_conf("resnet18") if not k.startswith("layer[")]
    mine = [(k, v) for k, v in load_conf("resnet18_gn") if not k.startswith("layer[") and k != "gn_group"]
    assert other == mine
    assert [v for k, v in load_conf("resnet18_gn") if k == "gn_group"] == ["32"] * 20


def test_resnet18_gn_builds_and_takes_one_finite_step_at_batch_1():
    # 195 x 195: the smallest input whose last stage still holds the 7 x 7 window of the final pooling
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("resnet18_gn", [("batch_size", "1"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                          ("seed", "1"), ("input_shape", "3,195,195")]):
        tr.set_param(k, v)
    tr.init_model()
    types = [c.type for c in tr.net.connections]
    assert types.count(46) == 20 and types.count(40) == 0 and tr.net.bn_state is None
    assert all(c.layer.groups == 32 for c in tr.net.connections if c.type == 46)
    b = _batch(1, n=1, shape=(3, 195, 195), classes=1000)
    before = tr.net.arena.w.clone()
    tr.update(b)
    assert torch.isfinite(tr.net.arena.w).all() and not torch.equal(before, tr.net.arena.w)
    out = _raw(tr, b).reshape(1, -1)
    assert out.shape == (1, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
