"""`kv_attention` (type id 53) on the CPU executor: the layer's torch path in float64 against
softmax(Q K^T / sqrt(d)) V written with autograd, what init_connection rejects, and the shape
inference of models/confs/pvt_v2_b1.conf."""
import pytest
import torch

B, NHEAD = 2, 3


def _layer(qshape, kvshape, nhead=NHEAD, same=None):
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    lay = create_layer(53, LayerContext(torch.device("cpu")))
    lay.set_param("nhead", str(nhead))
    q, kv, y = Node("q"), Node("kv"), Node("y")
    q.set_shape(*qshape)
    kv.set_shape(*kvshape)
    nodes = dict(q=q, kv=kv, y=y)
    if same:
        nodes[same[0]] = nodes[same[1]]
    lay.init_connection([nodes["q"], nodes["kv"]], [nodes["y"]])
    return lay, q, kv, y


def test_type_id():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("kv_attention") == 53


@pytest.mark.parametrize("d", [32, 64])
def test_layer_matches_autograd(d):
    C, (H, W), (Hk, Wk) = NHEAD * d, (3, 5), (2, 3)
    lay, q, kv, y = _layer((B, C, H, W), (B, 2 * C, Hk, Wk))
    assert y.shape == (B, C, H, W) and not lay.params
    for n in (q, kv, y):
        n.alloc("cpu", torch.float64)
    gen = torch.Generator().manual_seed(d)
    q.data.copy_(torch.randn(q.data.shape, generator=gen, dtype=torch.float64))
    kv.data.copy_(torch.randn(kv.data.shape, generator=gen, dtype=torch.float64))
    g = torch.randn(y.data.shape, generator=gen, dtype=torch.float64)
    qr, kvr = q.data.clone().requires_grad_(), kv.data.clone().requires_grad_()
    qh = qr.reshape(B, H * W, NHEAD, d).permute(0, 2, 1, 3)
    k, v = kvr.reshape(B, Hk * Wk, 2, NHEAD, d).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(qh @ k.transpose(-1, -2) / d ** 0.5, -1) @ v).permute(0, 2, 1, 3).reshape(y.data.shape)
    ref.backward(g)

    def close(got, want):
        return float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    lay.forward(True, [q, kv], [y])
    assert close(y.data, ref.detach())
    y.data.copy_(g)
    keep = q.data.clone(), kv.data.clone()
    lay.backprop(False, [q, kv], [y])
    assert torch.equal(q.data, keep[0]) and torch.equal(kv.data, keep[1])
    lay.backprop(True, [q, kv], [y])  # each gdst is the node's data
    assert close(q.data, qr.grad) and close(kv.data, kvr.grad)


@pytest.mark.parametrize("qshape,kvshape,keys,msg", [
    ((2, 48, 8, 8), (2, 96, 2, 2), dict(), "head width 16"),
    ((2, 96, 12, 12), (2, 192, 9, 9), dict(), "81 key positions"),
    ((2, 96, 129, 128), (2, 192, 2, 2), dict(), "16512 query positions"),
    ((2, 96, 8, 8), (2, 192, 2, 2), dict(same=("y", "q")), "three distinct nodes"),
    ((2, 96, 8, 8), (2, 192, 2, 2), dict(same=("y", "kv")), "three distinct nodes"),
    ((2, 96, 8, 8), (2, 96, 2, 2), dict(), "2 x its 96 channels"),
])
def test_init_connection_rejects(qshape, kvshape, keys, msg):
    with pytest.raises(Exception, match=msg):
        _layer(qshape, kvshape, **keys)


def test_pvt_v2_b1_shapes():
    from cxxnet_amd.models import available, load_conf
    from cxxnet_amd.nnet import NetTrainer
    assert "pvt_v2_b1" in available()
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("pvt_v2_b1", []) if not k.startswith("metric")] + [
            ("batch_size", "2"), ("dev", "cpu"), ("silent", "1")]:
        tr.set_param(k, v)
    tr.init_model()
    att = [c.layer for c in tr.net.connections if c.type == 53]
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000) and len(att) == 8
    assert [(l.tq, l.tk, l.nhead) for l in att[::2]] == [(3136, 49, 1), (784, 49, 2), (196, 49, 5), (49, 49, 8)]
