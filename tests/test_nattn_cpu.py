"""`neighborhood_attention` (type id 54) on the CPU executor: the layer's torch path (an index
gather) in float64 against an independent formulation with autograd -- per query an explicit list
of key positions built from the clamped definition, one softmax per query --, what init_connection
rejects, the checkpoint round trip of the bias table, and nat_mini.conf."""
import pytest
import torch

B, NHEAD, D = 2, 2, 32
C = NHEAD * D
CASES = [(7, 7, 7), (9, 10, 7), (22, 17, 7), (12, 11, 5), (8, 8, 3)]  # (H, W, k)


def _layer(shape, out=None, **keys):
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    lay = create_layer(54, LayerContext(torch.device("cpu")))
    for k, v in keys.items():
        lay.set_param(k, str(v))
    x = Node("x")
    y = x if out == "self" else Node("y")
    x.set_shape(*shape)
    lay.init_connection([x], [y])
    return lay, x, y


def neighbourhood(H, W, k):
    """per query y W + x: the map positions of its k k keys and their bias indices, by the definition"""
    keys, rel = [], []
    for y in range(H):
        for x in range(W):
            sy, sx = min(max(y - k // 2, 0), H - k), min(max(x - k // 2, 0), W - k)
            pairs = [(yy, xx) for yy in range(sy, sy + k) for xx in range(sx, sx + k)]
            keys.append([yy * W + xx for yy, xx in pairs])
            rel.append([(yy - y + k - 1) * (2 * k - 1) + xx - x + k - 1 for yy, xx in pairs])
    return torch.tensor(keys), torch.tensor(rel)


def nat_dense(x, bias, H, W, k, nhead):
    """x [B, H W, 3 C], bias [nhead, (2 k - 1)^2] -> q, k, v [B, nhead, H W, d] and the dense logits
    [B, nhead, H W, H W] with -inf outside every query's neighbourhood"""
    d = x.shape[-1] // 3 // nhead
    q, kk, v = x.view(x.shape[0], H * W, 3, nhead, d).permute(2, 0, 3, 1, 4)
    keys, rel = neighbourhood(H, W, k)
    add = torch.full((nhead, H * W, H * W), float("-inf"), dtype=x.dtype)
    add = add.scatter(2, keys.expand(nhead, -1, -1), bias[:, rel])
    return q, kk, v, q @ kk.transpose(-1, -2) / d ** 0.5 + add


def test_type_id():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("neighborhood_attention") == 54


@pytest.mark.parametrize("H,W,k", CASES)
def test_layer_matches_the_definition(H, W, k):
    lay, x, y = _layer((B, 3 * C, H, W), nhead=NHEAD, kernel=k)
    assert y.shape == (B, C, H, W) and lay.params[0].shape == (NHEAD, (2 * k - 1) ** 2) and lay.params[0].tag == "wmat"
    x.alloc("cpu", torch.float64)
    y.alloc("cpu", torch.float64)
    gen = torch.Generator().manual_seed(H * 100 + W)
    x.data.copy_(torch.randn(x.data.shape, generator=gen, dtype=torch.float64))
    g = torch.randn(y.data.shape, generator=gen, dtype=torch.float64)
    p = lay.params[0]
    p.w = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    p.g = torch.zeros_like(p.w)
    xr, br = x.data.clone().requires_grad_(), p.w.clone().requires_grad_()
    _, _, v, s = nat_dense(xr.view(B, H * W, 3 * C), br, H, W, k, NHEAD)
    ref = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(y.data.shape)
    ref.backward(g)

    def close(got, want):
        return float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    lay.forward(True, [x], [y])
    assert close(y.data, ref.detach())
    y.data.copy_(g)
    keep = x.data.clone()
    lay.backprop(False, [x], [y])
    assert torch.equal(x.data, keep) and close(p.g, br.grad)
    p.g.zero_()
    lay.backprop(True, [x], [y])  # x.gdst is x.data
    assert close(x.data, xr.grad) and close(p.g, br.grad)


@pytest.mark.parametrize("shape,keys,msg", [
    ((2, 3 * 128, 8, 8), dict(nhead=2, kernel=3), "head width 64"),
    ((2, 3 * 64, 8, 8), dict(nhead=2, kernel=4), "kernel = 4"),
    ((2, 3 * 64, 9, 9), dict(nhead=2, kernel=9), "kernel = 9"),
    ((2, 3 * 64, 6, 8), dict(nhead=2, kernel=7), "does not fit"),
    ((2, 3 * 64, 8, 8), dict(nhead=2, kernel=3, out="self"), "no self-loop"),
    ((2, 1, 1, 3 * 64), dict(nhead=2, kernel=3), "not a matrix node"),
])
def test_init_connection_rejects(shape, keys, msg):
    with pytest.raises(Exception, match=msg):
        _layer(shape, **keys)


def test_checkpoint_round_trip():
    from cxxnet_amd.layers.base import BinReader, BinWriter
    lay, _, _ = _layer((B, 3 * C, 8, 8), nhead=NHEAD, kernel=5)
    p = lay.params[0]
    p.w = torch.randn(p.shape, generator=torch.Generator().manual_seed(3))
    fo = BinWriter()
    lay.save_model(fo)
    other, _, _ = _layer((B, 3 * C, 8, 8), nhead=NHEAD, kernel=5)
    other.load_model(BinReader(fo.getvalue()))
    (got,) = other.loaded_values()
    assert got.dtype == torch.float32 and torch.equal(got.reshape(p.shape), p.w)


def test_nat_mini_builds():
    """the documented parameter count (docs/deviations.md) and the attention sites"""
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in [(k, v) for k, v in load_conf("nat_mini", []) if not k.startswith("metric")] + [
            ("batch_size", "2"), ("dev", "cpu"), ("silent", "1"), ("eval_train", "0")]:
        tr.set_param(k, v)
    tr.init_model()
    att = [c.layer for c in tr.net.connections if c.type == 54]
    assert [(l.hw, l.nhead) for l in att] == [((56, 56), 2)] * 3 + [((28, 28), 4)] * 4 + [((14, 14), 8)] * 6 + \
        [((7, 7), 16)] * 5 and all(l.kernel == 7 for l in att)
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    assert sum(s.numel for _, s in tr.net.arena.specs) == 19984174
