"""`layer_norm` (type id 49) and `gelu` (type id 50) on the CPU executor against plain torch, a
checkpoint round trip of a net holding both, and gemm.dwlk_served without a device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

# 8 x 9 x 9 input -> depthwise 7 x 7 -> layer_norm -> 1 x 1 conv -> gelu -> pooling -> fullc -> softmax
NET = """
netconfig=start
layer[0->d0] = conv:dw
  kernel_size = 7
  pad = 3
  nchannel = 8
  ngroup = 8
layer[d0->n0] = layer_norm:ln0
  init_slope = 1.5
  init_bias = 0.25
layer[n0->c1] = conv:pw
  kernel_size = 1
  nchannel = 16
layer[c1->a1] = gelu
layer[a1->p0] = avg_pooling
  kernel_size = 9
  stride = 9
layer[p0->f0] = flatten
layer[f0->out] = fullc:fc
  nhidden = 5
layer[out->out] = softmax
netconfig=end
input_shape = 8,9,9
random_type = xavier
eta = 0.05
momentum = 0.9
"""


def _trainer(seed=5):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(NET)) + [("batch_size", "4"), ("dev", "cpu"), ("eval_train", "0"),
                                                       ("silent", "1"), ("seed", str(seed))]:
        tr.set_param(k, v)
    return tr


def _batch(seed):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(4, 8, 9, 9, generator=g), torch.randint(0, 5, (4, 1), generator=g).float())


def _layer(kind, shape, **keys):
    """(layer, x node, y node) of a fresh CPU layer on an NCHW-shaped node, initialised"""
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    lay = create_layer(kind, LayerContext(torch.device("cpu")))
    for k, v in keys.items():
        lay.set_param(k, str(v))
    x, y = Node("x"), Node("y")
    x.set_shape(*shape)
    lay.init_connection([x], [y])
    return lay, x, y


def test_type_ids():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("layer_norm") == 49 and native.rt().get_layer_type("gelu") == 50


@pytest.mark.parametrize("C", [8, 20])
def test_layer_norm_ops_match_torch(C):
    from cxxnet_amd.ops import layer_ops as L
    gen = torch.Generator().manual_seed(C)
    x, g = torch.randn(7, C, generator=gen), torch.randn(7, C, generator=gen)
    slope, bias = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xr = x.double().requires_grad_()
    sr, br = slope.double().requires_grad_(), bias.double().requires_grad_()
    ref = F.layer_norm(xr, (C,), sr, br, 1e-6)
    ref.backward(g.double())
    st = L.LNState(7, C, "cpu")
    y, dx = torch.empty_like(x), torch.full_like(x, -3.0)
    gs, gb = torch.ones(C), torch.ones(C)
    L.ln_forward(x, y, slope, bias, 1e-6, st)
    L.ln_backward(g, x, dx, slope, gs, gb, st, False)
    assert bool((dx == -3.0).all())
    L.ln_backward(g, x, dx, slope, gs, gb, st, True)
    assert torch.allclose(y.double(), ref.detach(), atol=1e-5)
    assert torch.allclose(dx.double(), xr.grad, atol=1e-4)
    assert torch.allclose(gs.double(), 1 + 2 * sr.grad, atol=1e-4) and torch.allclose(gb.double(), 1 + 2 * br.grad, atol=1e-4)


def test_gelu_ops_match_torch():
    from cxxnet_amd.ops import layer_ops as L
    x = torch.cat([torch.linspace(-40, 40, 801), torch.tensor([0.0, -0.0, 3e38, -3e38])])
    g = torch.randn(x.numel(), generator=torch.Generator().manual_seed(1))
    xr = x.double().requires_grad_()
    ref = F.gelu(xr)
    ref.backward(g.double())
    y, dx = torch.empty_like(x), torch.empty_like(x)
    L.gelu_forward(x, y)
    L.gelu_backward(x, g, dx)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert torch.allclose(y.double(), ref.detach(), rtol=1e-6, atol=1e-6)
    assert torch.allclose(dx.double(), xr.grad, rtol=1e-6, atol=1e-6)


def test_layer_norm_layer_shapes_and_params():
    lay, x, y = _layer(49, (2, 24, 5, 5), init_slope=2, init_bias=-1)
    assert y.shape == x.shape and lay.eps == 1e-6 and lay.channel == 24 and lay.max_rows == 50
    assert [(p.tag, p.shape) for p in lay.params] == [("wmat", (24,)), ("bias", (24,))]
    lay, x, y = _layer(49, (3, 1, 1, 10))  # a matrix node: rows = B
    assert lay.channel == 10 and lay.max_rows == 3
    assert _layer(49, (2, 2048, 1, 1))[0].channel == 2048 and _layer(40, (2, 2056, 1, 1))[0].channel == 2056
    for C in (2056, 1028):  # beyond a register row: vectorised, scalar (batch_norm_ma above has no such limit)
        with pytest.raises(Exception, match="LayerNormLayer: %d channels" % C):
            _layer(49, (2, C, 1, 1))


def test_net_trains_and_checkpoint_round_trips():
    tr = _trainer()
    tr.init_model()
    probe = _batch(9)
    before = tr.forward_to([len(tr.net.nodes) - 1], probe)[0].copy()
    for seed in (1, 2):
        tr.update(_batch(seed))
    want = tr.forward_to([len(tr.net.nodes) - 1], probe)[0].copy()
    assert np.isfinite(want).all() and not np.array_equal(before, want)
    data = tr.save_model()
    tr2 = _trainer(seed=77)
    tr2.load_model(data)
    assert np.array_equal(tr2.forward_to([len(tr2.net.nodes) - 1], probe)[0], want)
    assert tr2.save_model() == data
    ln = tr2.net.connections[tr2.net_cfg.layer_name_map["ln0"]].layer
    assert tr2.net_cfg.layers[tr2.net_cfg.layer_name_map["ln0"]].type == 49
    assert not np.array_equal(ln.params[0].w.numpy(), np.full(8, 1.5, np.float32))  # trained, not initial


# (N, C, Cout, H, K, stride, pad, groups) -> served
@pytest.mark.parametrize("geo,want", [
    ((2, 96, 96, 56, 7, 1, 3, 96), True), ((2, 8, 8, 12, 11, 1, 0, 8), True), ((2, 8, 8, 9, 9, 1, 8, 8), True),
    ((2, 8, 8, 9, 7, 2, 3, 8), False), ((2, 12, 12, 9, 7, 1, 3, 12), False), ((2, 8, 8, 9, 5, 1, 2, 8), False),
    ((2, 8, 16, 9, 7, 1, 3, 8), False), ((2, 8, 8, 9, 7, 1, 7, 8), False), ((2, 16, 16, 9, 7, 1, 3, 2), False),
])
def test_dwlk_served(geo, want):
    N, C, Cout, H, K, S, pad, groups = geo
    Ho, _ = gemm.conv_out_size(H, H, K, K, S, pad, pad)
    g = ConvGeom(N, H, H, C, Ho, Ho, Cout, K, K, S, pad, pad, groups)
    assert gemm.dwlk_served(g) is want
    assert not gemm.dwconv_served(g) or K == 5


def test_convnext_tiny_conf_shapes_and_parameter_count():
    """models/confs/convnext_tiny.conf on the CPU executor: the stage maps and widths, 18 blocks, and
    the parameter count of ConvNeXt-T without its 18 layer-scale vectors, computed from the widths."""
    from cxxnet_amd.models import available, load_conf
    from cxxnet_amd.nnet import NetTrainer
    assert "convnext_tiny" in available()
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("convnext_tiny", []) if not k.startswith("metric")] + [
            ("batch_size", "2"), ("dev", "cpu"), ("silent", "1"), ("eval_train", "0")]:
        tr.set_param(k, v)
    tr.init_model()
    depths, widths, maps = (3, 3, 9, 3), (96, 192, 384, 768), (56, 28, 14, 7)
    shape = {n.name: n.shape for n in tr.net.nodes}
    for s, (d, C, m) in enumerate(zip(depths, widths, maps), 1):
        assert shape["s%d_in" % s] == (2, C, m, m) and shape["s%db%d" % (s, d)] == (2, C, m, m)
        assert shape["s%db1_e" % s] == (2, 4 * C, m, m) and "s%db%d" % (s, d + 1) not in shape
    assert shape["gap_n"] == (2, 768, 1, 1) and tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    block = lambda C: (49 * C + C) + 2 * C + (4 * C * C + 4 * C) + (4 * C * C + C)
    want = (48 * 96 + 96) + 2 * 96 + sum(d * block(C) for d, C in zip(depths, widths))
    want += sum(2 * a + (4 * a * b + b) for a, b in zip(widths, widths[1:])) + 2 * 768 + (768 * 1000 + 1000)
    assert want == 28589128 - sum(d * C for d, C in zip(depths, widths))  # the paper's count less layer scale
    assert sum(s.numel for _, s in tr.net.arena.specs) == want
