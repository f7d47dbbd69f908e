"""The `add` layer (type id 41) on the CPU executor: configuration, connection checks, gradients,
the zero-copy split in front of it, checkpoints through the CLI, and the ResNet-18 conf."""
import os

import numpy as np
import pytest
import torch

# 4 x 6 x 6 input -> conv + bn + relu -> one residual block (identity shortcut, add_relu = 1)
# -> a block with a stride-2 projection shortcut (plain add) -> avg pooling -> fullc -> softmax
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
layer[a_n1->a_r1] = relu
layer[a_r1->a_c2] = conv:a_c2
  kernel_size = 3
  pad = 1
  nchannel = 8
  no_bias = 1
layer[a_c2->a_n2] = batch_norm_ma:a_bn2
layer[a_n2,a_id->a] = add:a_add
  add_relu = 1
layer[a->b_x,b_id] = split
layer[b_x->b_c1] = conv:b_c1
  kernel_size = 3
  pad = 1
  stride = 2
  nchannel = 16
  no_bias = 1
layer[b_c1->b_n1] = batch_norm_ma:b_bn1
layer[b_id->b_cp] = conv:b_proj
  kernel_size = 1
  stride = 2
  nchannel = 16
  no_bias = 1
layer[b_cp->b_np] = batch_norm_ma:b_bnp
layer[b_n1,b_np->b] = add:b_add
layer[b->gap] = avg_pooling
  kernel_size = 3
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


# ------------------------------------------------------------------ configuration
def test_type_id_name_and_flags():
    from cxxnet_amd import native
    from cxxnet_amd.layers import LayerContext, create_layer
    from cxxnet_amd.nnet import neural_net
    assert native.rt().get_layer_type("add") == 41
    assert neural_net.K_ADD == 41
    lay = create_layer(41, LayerContext(torch.device("cpu")))
    assert type(lay).__name__ == "AddLayer" and lay.type_name == "add"
    assert type(lay).__dict__["replay_audited"] is False and lay.replay_safe() is False
    assert lay.relu is False  # the default
    lay.set_param("add_relu", "1")
    assert lay.relu is True
    lay.set_param("add_relu", "0")
    assert lay.relu is False
    lay.set_param("relu", "1")  # another layer's key: ignored
    lay.set_param("eta", "0.1")  # a global key: ignored
    assert lay.relu is False
    with pytest.raises(ValueError, match="AddLayer"):
        lay.set_param("add_relu", "2")


def test_the_conf_sets_add_relu_per_layer():
    tr = _make()
    assert tr.net_cfg.layers[tr.net_cfg.layer_name_map["a_add"]].type == 41
    assert _layer(tr, "a_add").relu is True and _layer(tr, "b_add").relu is False
    assert _layer(tr, "a_add").params == [] and tr.net.nodes[-1].shape == (B, 1, 1, 5)


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
    return create_layer(41, LayerContext(torch.device("cpu")))


def test_rejected_connections():
    from cxxnet_amd.layers import Node
    s = (2, 3, 4, 4)
    a, b, c, d, e = _nodes(s, s, s, s, s)
    o, o2 = Node("o"), Node("o2")
    for nin, nout in [([a], [o]),                    # one input
                      ([a, b, c, d, e], [o]),        # five inputs
                      ([a, b], [o, o2]),             # two outputs
                      ([a, b], []),                  # no output
                      ([a, b], [a]),                 # the output is an input
                      ([a, b, c], [c]),
                      ([a, a], [o]),                 # the same node twice
                      ([a, b, a], [o])]:
        with pytest.raises(ValueError, match="AddLayer"):
            _fresh().init_connection(nin, nout)
    for other in [(2, 3, 4, 5), (2, 4, 4, 4), (2, 1, 1, 48)]:  # another shape, also with the same size
        (m,) = _nodes(other)
        with pytest.raises(ValueError, match="AddLayer"):
            _fresh().init_connection([a, m], [o])
    (p,) = _nodes(s)
    p.cp = 4  # a channel-padded node
    with pytest.raises(ValueError, match="AddLayer"):
        _fresh().init_connection([a, p], [o])
    lay = _fresh()
    lay.init_connection([a, b, c, d], [o])
    assert o.shape == s and o.cp == 3


def test_an_unknown_sum_layer_name_is_still_an_error():
    from cxxnet_amd import native
    with pytest.raises(Exception, match="unknown layer type"):
        native.rt().get_layer_type("sum")


# ------------------------------------------------------------------ the layer's arithmetic
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", [2, 4])
def test_finite_difference_gradient(N, relu):
    """The loss sum(w y) is piecewise linear in the inputs, so a central difference is exact up to
    fp32 rounding wherever no kink lies inside the step; sums within 0.05 of 0 are moved away."""
    shape = (2, 3, 2, 2)
    gen = torch.Generator().manual_seed(10 * N + relu)
    nodes = _nodes(*([shape] * (N + 1)))
    ins, out = nodes[:N], nodes[N]
    lay = _fresh()
    lay.set_param("add_relu", str(relu))
    lay.init_connection(ins, [out])
    for n in nodes:
        n.alloc("cpu", torch.float32)
    xs = [torch.randn(n.data.shape, generator=gen) for n in ins]
    tot = sum(xs[1:], xs[0])
    xs[0] += torch.where(tot.abs() < 0.05, torch.full_like(tot, 0.2), torch.zeros_like(tot)) * torch.sign(tot + 1e-9)
    w = torch.randn(out.data.shape, generator=gen)

    def loss(vals):
        for n, v in zip(ins, vals):
            n.data.copy_(v)
        lay.forward(True, ins, [out])
        return (out.data.double() * w.double()).sum().item()

    loss(xs)
    y = out.data.clone()
    if relu:
        assert (y == 0).any() and (y > 0).any()
    out.data.copy_(w)  # the output node now holds the gradient
    lay.backprop(True, ins, [out])
    want = torch.where(y > 0, w, torch.zeros_like(w)) if relu else w
    h = 1e-2
    grads = [n.data.clone() for n in ins]  # (loss() below overwrites the nodes)
    for k in range(N):
        assert torch.equal(grads[k], want)  # the same gradient for every input, exactly 0 where masked
        fd = torch.zeros_like(w).reshape(-1)
        for i in range(fd.numel()):
            plus, minus = [x.clone() for x in xs], [x.clone() for x in xs]
            plus[k].view(-1)[i] += h
            minus[k].view(-1)[i] -= h
            fd[i] = (loss(plus) - loss(minus)) / (2 * h)
        assert torch.allclose(fd.view_as(w), want, rtol=1e-3, atol=1e-3), k
    # prop_grad = False writes nothing
    for n in ins:
        n.data.fill_(7.0)
    lay.backprop(False, ins, [out])
    assert all((n.data == 7.0).all() for n in ins)


def test_forward_order_rounding_and_inference():
    """fp32 accumulation in input order; the inference forward keeps no mask and gives the same y."""
    from cxxnet_amd.ops import layer_ops as L
    x0, x1, x2 = torch.tensor([2.0 ** 24, -1.0]), torch.tensor([1.0, -1.0]), torch.tensor([1.0, 3.0])
    y = torch.empty(2)
    L.add_forward([x0, x1, x2], y, False)
    assert y.tolist() == [2.0 ** 24, 1.0]  # (2^24 + 1) + 1 in fp32, left to right
    st = L.AddState(2, "cpu", False)
    L.add_forward([x1, x2], y, True, st)
    assert y.tolist() == [2.0, 2.0] and st.mask.dtype == torch.bool and st.mask.tolist() == [True, True]
    L.add_forward([x0, x1], y, True, st)
    assert y.tolist() == [2.0 ** 24 + 1 - 1, 0.0] and st.mask.tolist() == [True, False]
    d0, d1 = torch.full((2,), 9.0), torch.full((2,), 9.0)
    L.add_backward(torch.tensor([5.0, 6.0]), [d0, d1], st)
    assert d0.tolist() == d1.tolist() == [5.0, 0.0]
    with pytest.raises(ValueError):
        L.add_forward([x0], y, False)


def test_backprop_before_a_training_forward_is_an_error():
    a, b, o = _nodes((1, 2, 1, 1), (1, 2, 1, 1), (0, 0, 0, 0))
    lay = _fresh()
    lay.set_param("add_relu", "1")
    lay.init_connection([a, b], [o])
    for n in (a, b, o):
        n.alloc("cpu", torch.float32)
    lay.forward(False, [a, b], [o])  # inference: no mask is allocated
    assert lay._st is None
    with pytest.raises(ValueError, match="AddLayer"):
        lay.backprop(True, [a, b], [o])


# ------------------------------------------------------------------ the executor
def _splits(tr):
    return [c for c in tr.net.connections if c.type == 23]


def _params(tr):
    return [tr.net.arena.w[s.offset:s.offset + s.numel].detach().clone() for _, s in tr.net.arena.specs]


def test_fused_split_aliases_the_shortcut_and_the_step_is_unchanged(monkeypatch):
    res = {}
    for mode in ("0", "2"):
        monkeypatch.setenv("CXXNET_FUSE", mode)
        tr = _make()
        add = tr.net.connections[tr.net_cfg.layer_name_map["a_add"]]
        assert any(o in add.nodes_in for o in _splits(tr)[0].nodes_out)  # the identity shortcut
        assert len(_splits(tr)) == 2
        for sp in _splits(tr):
            assert sp.layer.alias is (mode == "2"), mode
            src = sp.nodes_in[0]
            for o in sp.nodes_out:
                same = o.data.data_ptr() == src.data.data_ptr()
                assert same is (mode == "2")
                assert (o.grad_buf is not None) is (mode == "2")
        probe = _batch(7)
        tr.update(_batch(1))
        tr.update(_batch(2))
        res[mode] = (_params(tr), _raw(tr, probe), tr.net.bn_state.clone())
    for a, b in zip(res["0"][0], res["2"][0]):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
    assert np.allclose(res["0"][1], res["2"][1], rtol=1e-5, atol=1e-6)
    assert torch.allclose(res["0"][2], res["2"][2], rtol=1e-5, atol=1e-6)


def test_nonneg_marking_follows_add_relu():
    """A max pooling behind an add takes the non-negative path only with add_relu = 1."""
    for relu, want in (("1", True), ("0", False)):
        conf = NET.replace("layer[b->gap] = avg_pooling", "layer[b->gap] = max_pooling").replace(
            "layer[b_n1,b_np->b] = add:b_add", "layer[b_n1,b_np->b] = add:b_add\n  add_relu = " + relu)
        tr = _make(conf)
        pool = next(c.layer for c in tr.net.connections if c.type == 11)
        assert pool.input_nonneg is want


def test_one_step_trains_every_branch():
    tr = _make()
    before = _params(tr)
    tr.update(_batch(1))
    after = _params(tr)
    keys = [(li, s.tag) for li, s in tr.net.arena.specs]
    for k, a, b in zip(keys, before, after):
        assert torch.isfinite(b).all() and not torch.equal(a, b), k
    out = _raw(tr, _batch(3))
    assert np.isfinite(out).all() and np.allclose(out.reshape(B, -1).sum(1), 1.0, atol=1e-5)


def test_smaller_batch_gives_the_same_rows():
    tr = _make()
    tr.update(_batch(1))
    full = _batch(4)
    from cxxnet_amd.io.data import DataBatch
    part = DataBatch(full.data[:3].clone(), full.label[:3].clone())
    want = _raw(tr, full)[:3]
    assert np.array_equal(_raw(tr, part), want)
    tr.update(part)  # a training step on the smaller batch: the mask covers any batch up to the largest
    tr.update(full)


# ------------------------------------------------------------------ checkpoints
def test_the_layer_writes_nothing_into_the_model_file():
    from cxxnet_amd.layers.base import BinWriter
    tr = _make()
    fo = BinWriter()
    _layer(tr, "a_add").save_model(fo)
    assert fo.getvalue() == b""
    assert not hasattr(_layer(tr, "a_add"), "bind_state")
    tr.update(_batch(1))
    data = tr.save_model()
    tr2 = _trainer(seed=77)
    tr2.load_model(data)
    probe = _batch(9)
    assert np.array_equal(_raw(tr2, probe), _raw(tr, probe))
    assert tr2.save_model() == data
    assert tr2.net_cfg.layers[tr2.net_cfg.layer_name_map["b_add"]].type == 41
    assert _layer(tr2, "a_add").relu is True  # layer keys travel in the NetConfig


CLI_CONF = """
data = train
iter = synthetic
  num_class = 5
  num_batch = 3
  synthetic_device = cpu
iter = end
%s
batch_size = 4
dev = cpu
save_model = 1
max_round = 2
num_round = 2
metric = error
model_dir = %s
silent = 1
"""


def test_cli_save_load_continue(tmp_path):
    from cxxnet_amd import native
    from cxxnet_amd.cli import LearnTask
    mdir = tmp_path / "models"
    path = tmp_path / "res.conf"
    path.write_text(CLI_CONF % (NET, mdir))
    t = LearnTask()
    assert t.run([str(path)]) == 0
    assert sorted(os.listdir(mdir)) == ["0000.model", "0001.model", "0002.model"]
    raw = open(mdir / "0002.model", "rb").read()

    def load(name):
        t2 = LearnTask()
        for k, v in native.rt().parse_config(path.read_text()):
            t2.set_param(k, v)
        t2.name_model_in = str(mdir / name)
        t2.task = "pred"
        t2.load_model()
        return t2
    t2 = load("0002.model")
    assert b"\x00\x00\x00\x00" + t2.trainer.save_model() == raw
    assert torch.equal(t2.trainer.net.arena.w, t.trainer.net.arena.w)
    assert torch.equal(t2.trainer.net.bn_state, t.trainer.net.bn_state)
    probe = _batch(9)
    assert np.array_equal(_raw(t2.trainer, probe), _raw(t.trainer, probe))
    # continue = 1 picks 0002.model up and trains one more round
    assert LearnTask().run([str(path), "continue=1", "num_round=3", "max_round=3"]) == 0
    assert "0003.model" in os.listdir(mdir)
    t3 = load("0003.model")
    assert not torch.equal(t3.trainer.net.arena.w, t.trainer.net.arena.w)
    assert torch.isfinite(t3.trainer.net.arena.w).all()


# ------------------------------------------------------------------ ResNet-18
@pytest.fixture(scope="module")
def resnet18():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("resnet18", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                       ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def test_resnet18_conf_builds(resnet18):
    net = resnet18.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    types = [c.type for c in net.connections]
    assert types.count(41) == 8 and types.count(23) == 8 and types.count(10) == 20 and types.count(40) == 20
    assert all(c.layer.relu for c in net.connections if c.type == 41)
    assert all(c.layer.lp.no_bias == 1 for c in net.connections if c.type == 10)
    # the four stages end at 56^2 x 64, 28^2 x 128, 14^2 x 256, 7^2 x 512
    tails = [c.nodes_out[0].shape[1:] for c in net.connections if c.type == 41][1::2]
    assert tails == [(64, 56, 56), (128, 28, 28), (256, 14, 14), (512, 7, 7)]
    # conv weights + bn slope and bias + the classifier: the paper's 11.7 M parameters
    nparam = sum(s.numel for _, s in net.arena.specs)
    assert nparam == 11689512


def test_resnet18_one_training_step(resnet18):
    tr = resnet18
    b = _batch(1, n=2, shape=(3, 224, 224), classes=1000)
    before = tr.net.arena.w.clone()
    tr.update(b)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
