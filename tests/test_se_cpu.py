"""The `ch_scale` layer (type id 42) on the CPU executor: configuration, connection checks, gradients
against torch autograd, the zero-copy split in front of it, checkpoints, and the SE-ResNet-18 conf."""
import numpy as np
import pytest
import torch

# 4 x 6 x 6 input -> conv + bn + relu -> a residual block whose branch carries a squeeze-and-excitation
# module (global avg pooling -> flatten -> fullc(8) -> relu -> fullc(8) -> sigmoid -> ch_scale) ->
# avg pooling -> fullc -> softmax
NET = """
netconfig=start
layer[0->c0] = conv:c0
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[c0->n0] = batch_norm_ma:bn0
layer[n0->r0] = relu
layer[r0->a_x,a_id] = split
layer[a_x->a_c1] = conv:a_c1
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[a_c1->a_n1] = batch_norm_ma:a_bn1
layer[a_n1->a_sq,a_ex] = split
layer[a_sq->a_gp] = avg_pooling
  kernel_size = 6
  stride = 1
layer[a_gp->a_gf] = flatten
layer[a_gf->a_g1] = fullc:a_fc1
  nhidden = 8
layer[a_g1->a_g2] = relu
layer[a_g2->a_g3] = fullc:a_fc2
  nhidden = 8
layer[a_g3->a_gs] = sigmoid
layer[a_ex,a_gs->a_se] = ch_scale:a_scale
layer[a_se,a_id->a] = add:a_add
  add_relu = 1
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


# ------------------------------------------------------------------ configuration
def test_type_id_name_and_flags():
    from cxxnet_amd import native
    from cxxnet_amd.layers import LayerContext, create_layer
    from cxxnet_amd.nnet import neural_net
    assert native.rt().get_layer_type("ch_scale") == 42
    assert neural_net.K_CH_SCALE == 42 and 42 in neural_net._SPLIT_SAFE
    lay = create_layer(42, LayerContext(torch.device("cpu")))
    assert type(lay).__name__ == "ChScaleLayer" and lay.type_name == "ch_scale"
    assert type(lay).__dict__["replay_audited"] is False and lay.replay_safe() is False
    lay.set_param("add_relu", "1")  # another layer's key: ignored
    lay.set_param("eta", "0.1")     # a global key: ignored
    assert lay.params == []


def _nodes(*shapes):
    from cxxnet_amd.layers import Node
    out = []
    for i, s in enumerate(shapes):
        n = Node("n%d" % i)
        n.set_shape(*s)
        out.append(n)
    return out


def _fresh():
    from cxxnet_amd.layers import LayerContext, create_layer
    return create_layer(42, LayerContext(torch.device("cpu")))


def test_connection_checks():
    from cxxnet_amd.layers import Node
    x, x2, s_mat, s_ch = _nodes((2, 3, 4, 5), (2, 3, 4, 5), (2, 1, 1, 3), (2, 3, 1, 1))
    o, o2 = Node("o"), Node("o2")
    for nin, nout in [([x], [o]),                    # one input
                      ([x, s_mat, s_ch], [o]),       # three inputs
                      ([x, s_mat], [o, o2]),         # two outputs
                      ([x, s_mat], []),              # no output
                      ([x, s_mat], [x]),             # the output is an input
                      ([x, s_mat], [s_mat]),
                      ([x, x], [o]),                 # x is s
                      ([x, x2], [o]),                # a gate of the map's shape
                      ([s_mat, x], [o])]:            # the inputs swapped
        with pytest.raises(ValueError, match="ChScaleLayer"):
            _fresh().init_connection(nin, nout)
    for other in [(2, 1, 1, 4), (3, 1, 1, 3), (2, 4, 1, 1), (2, 1, 3, 1), (1, 1, 1, 6), (2, 3, 1, 2)]:
        (m,) = _nodes(other)
        with pytest.raises(ValueError, match="ChScaleLayer"):
            _fresh().init_connection([x, m], [o])
    (p,) = _nodes((2, 3, 4, 5))
    p.cp = 4  # a channel-padded map
    with pytest.raises(ValueError, match="ChScaleLayer"):
        _fresh().init_connection([p, s_mat], [o])
    (q,) = _nodes((2, 3, 1, 1))
    q.cp = 8  # a channel-padded gate
    with pytest.raises(ValueError, match="ChScaleLayer"):
        _fresh().init_connection([x, q], [o])
    for s in (s_mat, s_ch):
        o = Node("o")
        _fresh().init_connection([x, s], [o])
        assert o.shape == (2, 3, 4, 5) and o.cp == 3
    (one,) = _nodes((2, 3, 1, 1))  # a 1 x 1 map with a gate of its own shape
    (g1,) = _nodes((2, 3, 1, 1))
    _fresh().init_connection([one, g1], [Node("o")])


def test_an_unknown_scale_layer_name_is_still_an_error():
    from cxxnet_amd import native
    with pytest.raises(Exception, match="unknown layer type"):
        native.rt().get_layer_type("scale")


# ------------------------------------------------------------------ the layer's arithmetic
@pytest.mark.parametrize("gate", ["mat", "ch"])
@pytest.mark.parametrize("alias", [False, True])
def test_gradients_match_autograd(gate, alias):
    """y = x s and its two gradients against torch autograd; alias: the gradients overwrite the inputs
    (the usual in-place nodes), else x's goes to a private buffer as behind a zero-copy split."""
    Bn, C, H, W = 3, 5, 4, 2
    x, s, o = _nodes((Bn, C, H, W), (Bn, 1, 1, C) if gate == "mat" else (Bn, C, 1, 1), (0, 0, 0, 0))
    lay = _fresh()
    lay.init_connection([x, s], [o])
    for n in (x, s, o):
        n.alloc("cpu", torch.float32)
    gen = torch.Generator().manual_seed(3)
    xv = torch.randn(x.data.shape, generator=gen)
    sv = torch.rand(Bn, C, generator=gen)
    gv = torch.randn(x.data.shape, generator=gen)
    x.data.copy_(xv)
    s.data.copy_(sv.reshape(s.data.shape))
    if not alias:
        x.grad_buf = torch.full_like(x.data, 9.0)
    ys = []
    for is_train in (True, False):
        lay.forward(is_train, [x, s], [o])
        ys.append(o.data.clone())
    assert torch.equal(ys[0], ys[1])
    xa, sa = xv.clone().requires_grad_(), sv.clone().requires_grad_()
    ya = xa * sa[:, None, None, :]
    assert torch.equal(ys[0], ya.detach())
    ya.backward(gv)
    o.data.copy_(gv)  # the output node now holds the gradient
    lay.backprop(False, [x, s], [o])  # prop_grad = False writes nothing
    assert torch.equal(x.data, xv) and torch.equal(s.data.reshape(Bn, C), sv)
    lay.backprop(True, [x, s], [o])
    assert torch.allclose(x.gdst, xa.grad, rtol=1e-6, atol=1e-6)
    assert torch.allclose(s.data.reshape(Bn, C), sa.grad, rtol=1e-5, atol=1e-5)
    if not alias:
        assert torch.equal(x.data, xv)  # only read


def test_ops_reject_a_gate_of_another_size():
    from cxxnet_amd.ops import layer_ops as L
    x = torch.zeros(2, 3, 3, 4)
    with pytest.raises(ValueError, match="ch_scale"):
        L.ch_scale_forward(x, torch.zeros(2, 5), torch.zeros_like(x))


# ------------------------------------------------------------------ the executor
def _splits(tr):
    return [c for c in tr.net.connections if c.type == 23]


def test_fused_split_aliases_the_map_and_the_step_is_unchanged(monkeypatch):
    res = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("CXXNET_FUSE", mode)
        tr = _make()
        sc = tr.net.connections[tr.net_cfg.layer_name_map["a_scale"]]
        assert sc.type == 42 and _splits(tr)[1].nodes_out[1] is sc.nodes_in[0]
        for sp in _splits(tr):
            assert sp.layer.alias is (mode == "2"), mode
            for o in sp.nodes_out:
                assert (o.data.data_ptr() == sp.nodes_in[0].data.data_ptr()) is (mode == "2")
                assert (o.grad_buf is not None) is (mode == "2")
        probe = _batch(7)
        tr.update(_batch(1))
        tr.update(_batch(2))
        res[mode] = (_params(tr), _raw(tr, probe), tr.net.bn_state.clone())
    for a, b in zip(res["0"][0], res["2"][0]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert np.allclose(res["0"][1], res["2"][1], rtol=1e-5, atol=1e-6)
    assert torch.allclose(res["0"][2], res["2"][2], rtol=1e-5, atol=1e-6)


# the gate itself comes out of a split: that split must keep copying
GATE_SPLIT = NET.replace("layer[a_g3->a_gs] = sigmoid", "layer[a_g3->a_g4] = sigmoid\nlayer[a_g4->a_gs,a_gt] = split") \
    .replace("layer[a->gap] = avg_pooling", "layer[a_gt->a_gu] = fullc:a_fc3\n  nhidden = 3\nlayer[a->gap] = avg_pooling")


def test_a_split_feeding_the_gate_keeps_copying(monkeypatch):
    monkeypatch.setenv("CXXNET_FUSE", "2")
    tr = _make(GATE_SPLIT)
    sc = tr.net.connections[tr.net_cfg.layer_name_map["a_scale"]]
    sp = next(c for c in _splits(tr) if sc.nodes_in[1] in c.nodes_out)
    assert sp.layer.alias is False and all(o.grad_buf is None for o in sp.nodes_out)
    tr.update(_batch(1))
    assert torch.isfinite(tr.net.arena.w).all()


def test_the_output_is_not_marked_non_negative():
    conf = NET.replace("layer[a_se,a_id->a] = add:a_add\n  add_relu = 1", "layer[a_se->a] = max_pooling\n  kernel_size = 1")
    conf = conf.replace("layer[r0->a_x,a_id] = split", "layer[r0->a_x] = relu")
    tr = _make(conf)
    pool = next(c.layer for c in tr.net.connections if c.type == 11)
    assert pool.input_nonneg is False


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
def test_the_layer_writes_nothing_into_the_model_file():
    from cxxnet_amd.layers.base import BinWriter
    tr = _make()
    fo = BinWriter()
    _layer(tr, "a_scale").save_model(fo)
    assert fo.getvalue() == b""
    assert not hasattr(_layer(tr, "a_scale"), "bind_state")
    tr.update(_batch(1))
    data = tr.save_model()
    tr2 = _trainer(seed=77)
    tr2.load_model(data)
    probe = _batch(9)
    assert np.array_equal(_raw(tr2, probe), _raw(tr, probe))
    assert tr2.save_model() == data
    assert tr2.net_cfg.layers[tr2.net_cfg.layer_name_map["a_scale"]].type == 42


# ------------------------------------------------------------------ SE-ResNet-18
@pytest.fixture(scope="module")
def se_resnet18():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("se_resnet18", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                          ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def test_se_resnet18_conf_builds(se_resnet18):
    net = se_resnet18.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    types = [c.type for c in net.connections]
    assert types.count(42) == 8 and types.count(41) == 8 and types.count(23) == 16
    assert types.count(10) == 20 and types.count(40) == 20 and types.count(4) == 8 and types.count(1) == 17
    assert types.count(13) == 9  # the eight squeezes and the classifier's pooling
    # the four stages end at 56^2 x 64, 28^2 x 128, 14^2 x 256, 7^2 x 512
    tails = [c.nodes_out[0].shape[1:] for c in net.connections if c.type == 41][1::2]
    assert tails == [(64, 56, 56), (128, 28, 28), (256, 14, 14), (512, 7, 7)]
    gates = [c.nodes_in[1].shape[1:] for c in net.connections if c.type == 42]
    assert gates == [(1, 1, 64)] * 2 + [(1, 1, 128)] * 2 + [(1, 1, 256)] * 2 + [(1, 1, 512)] * 2
    widths = [c.layer.lp.num_hidden for c in net.connections if c.type == 1][:-1:2]
    assert widths == [8, 8, 8, 8, 16, 16, 32, 32]  # r = max(C / 16, 8)
    # every squeeze pools its whole map
    for c in net.connections:
        if c.type == 13:
            assert c.nodes_out[0].shape[2:] == (1, 1) and c.layer.lp.kernel_height == c.nodes_in[0].shape[2]
    # ResNet-18's 11,689,512 + 2 (2 C r + r + C) per stage
    nparam = sum(s.numel for _, s in net.arena.specs)
    assert nparam == 11689512 + 2 * (1096 + 2184 + 8464 + 33312) == 11779624


def test_se_resnet18_one_training_step(se_resnet18):
    tr = se_resnet18
    b = _batch(1, n=2, shape=(3, 224, 224), classes=1000)
    before = tr.net.arena.w.clone()
    tr.update(b)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
