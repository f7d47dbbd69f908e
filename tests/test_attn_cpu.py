"""`attention` (type id 51) on the CPU executor: the layer's torch path against
scaled_dot_product_attention in float64 with autograd, what init_connection rejects, and
cpvt_small.conf on dev = cpu."""
import pytest
import torch
import torch.nn.functional as F


def _layer(shape, out=None, **keys):
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    lay = create_layer(51, LayerContext(torch.device("cpu")))
    for k, v in keys.items():
        lay.set_param(k, str(v))
    x = Node("x")
    y = x if out == "self" else Node("y")
    x.set_shape(*shape)
    lay.init_connection([x], [y])
    return lay, x, y


def test_type_id():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("attention") == 51


def test_layer_matches_sdpa():
    B, C, NH, H = 2, 64, 2, 3
    lay, x, y = _layer((B, 3 * C, H, H), nhead=NH)
    assert y.shape == (B, C, H, H) and lay.tokens == 9 and not lay.params
    x.alloc("cpu", torch.float32)
    y.alloc("cpu", torch.float32)
    gen = torch.Generator().manual_seed(4)
    x.data.copy_(torch.randn(x.data.shape, generator=gen))
    g = torch.randn(y.data.shape, generator=gen)
    xr = x.data.double().requires_grad_()
    v = xr.view(B, H * H, 3, NH, C // NH).permute(2, 0, 3, 1, 4)
    ref = F.scaled_dot_product_attention(v[0], v[1], v[2]).permute(0, 2, 1, 3).reshape(B, H, H, C)
    ref.backward(g.double())
    lay.forward(True, [x], [y])
    assert torch.allclose(y.data.double(), ref.detach(), atol=1e-5)
    y.data.copy_(g)
    keep = x.data.clone()
    lay.backprop(False, [x], [y])
    assert torch.equal(x.data, keep)
    lay.backprop(True, [x], [y])  # x.gdst is x.data
    assert torch.allclose(x.data.double(), xr.grad, atol=1e-5)


@pytest.mark.parametrize("shape,keys,msg", [
    ((2, 3 * 96, 3, 3), dict(nhead=2), "head width 48"),
    ((2, 3 * 64, 3, 3), dict(), "must set nhead"),
    ((2, 3 * 64, 33, 32), dict(nhead=2), "1056 positions"),
    ((2, 3 * 64, 3, 3), dict(nhead=2, out="self"), "no self-loop"),
])
def test_init_connection_rejects(shape, keys, msg):
    with pytest.raises(Exception, match=msg):
        _layer(shape, **keys)


def test_cpvt_small_builds_on_cpu():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("cpvt_small", []) if not k.startswith("metric")] + [
            ("batch_size", "2"), ("dev", "cpu"), ("silent", "1")]:
        tr.set_param(k, v)
    tr.init_model()
    att = [c.layer for c in tr.net.connections if c.type == 51]
    assert len(att) == 12 and all((l.nhead, l.channel, l.tokens) == (6, 384, 196) for l in att)
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
