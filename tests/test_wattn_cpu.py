"""`window_attention` (type id 52) on the CPU executor: the layer's torch path (index arithmetic
on the map) in float64 against Swin's own formulation -- roll, reshape into windows, an additive
-inf mask from region labels, the bias gathered through an index table -- with autograd, and what
init_connection rejects."""
import pytest
import torch

B, NHEAD, D = 2, 3, 32
CASES = [(14, 21, 7, 3), (8, 16, 8, 4), (8, 12, 4, 0), (6, 4, 2, 1)]


def _layer(shape, out=None, **keys):
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    lay = create_layer(52, LayerContext(torch.device("cpu")))
    for k, v in keys.items():
        lay.set_param(k, str(v))
    x = Node("x")
    y = x if out == "self" else Node("y")
    x.set_shape(*shape)
    lay.init_connection([x], [y])
    return lay, x, y


def windows(t, H, W, ws, shift):
    """[B', H, W, c] -> [B', nwin, ws ws, c]: Swin's roll(-shift) and window partition"""
    t = torch.roll(t, (-shift, -shift), (1, 2)).view(t.shape[0], H // ws, ws, W // ws, ws, -1)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(t.shape[0], -1, ws * ws, t.shape[-1])


def unwindows(t, H, W, ws, shift):
    """the inverse: [B', nwin, ws ws, c] -> [B', H, W, c]"""
    t = t.view(t.shape[0], H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5)
    return torch.roll(t.reshape(t.shape[0], H, W, -1), (shift, shift), (1, 2))


def swin_logits(x, bias, H, W, ws, shift, nhead):
    """x [B, H, W, 3 C], bias [nhead, (2 ws - 1)^2] -> q, k, v [B, nwin, nhead, n, d], the logits
    [B, nwin, nhead, n, n] with -inf where Swin's region labels differ, and the bias index table"""
    n, d = ws * ws, x.shape[-1] // 3 // nhead
    xw = windows(x, H, W, ws, shift).view(x.shape[0], -1, n, 3, nhead, d).permute(3, 0, 1, 4, 2, 5)
    region = torch.zeros(1, H, W, 1, dtype=x.dtype)
    if shift:
        for a, ys in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
            for b, xs in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                region[:, ys, xs] = 3 * a + b
    lab = windows(region, H, W, ws, 0)[0, :, :, 0]  # (the labels are laid out in the rolled frame)
    mask = torch.zeros(lab.shape[0], n, n, dtype=x.dtype).masked_fill(lab[:, :, None] != lab[:, None, :], float("-inf"))
    cy, cx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    table = (cy[:, None] - cy[None] + ws - 1) * (2 * ws - 1) + cx[:, None] - cx[None] + ws - 1
    return xw[0], xw[1], xw[2], xw[0] @ xw[1].transpose(-1, -2) / d ** 0.5 + bias[:, table] + mask[:, None], table


def heads_to_map(t, H, W, ws, shift):
    """[B, nwin, nhead, n, c] -> [B, H, W, nhead c]"""
    return unwindows(t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], t.shape[3], -1), H, W, ws, shift)


def test_type_id():
    from cxxnet_amd import native
    assert native.rt().get_layer_type("window_attention") == 52


@pytest.mark.parametrize("H,W,ws,shift", CASES)
def test_layer_matches_swin_formulation(H, W, ws, shift):
    C = NHEAD * D
    lay, x, y = _layer((B, 3 * C, H, W), nhead=NHEAD, window=ws, shift=shift)
    assert y.shape == (B, C, H, W) and lay.params[0].shape == (NHEAD, (2 * ws - 1) ** 2) and lay.params[0].tag == "wmat"
    x.alloc("cpu", torch.float64)
    y.alloc("cpu", torch.float64)
    gen = torch.Generator().manual_seed(H * 100 + W)
    x.data.copy_(torch.randn(x.data.shape, generator=gen, dtype=torch.float64))
    g = torch.randn(y.data.shape, generator=gen, dtype=torch.float64)
    p = lay.params[0]
    p.w = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    p.g = torch.zeros_like(p.w)
    xr, br = x.data.clone().requires_grad_(), p.w.clone().requires_grad_()
    _, _, v, s, _ = swin_logits(xr, br, H, W, ws, shift, NHEAD)
    ref = heads_to_map(torch.softmax(s, -1) @ v, H, W, ws, shift)
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
    ((2, 3 * 128, 8, 8), dict(nhead=2, window=4), "head width 64"),
    ((2, 3 * 64, 9, 9), dict(nhead=2, window=9), "window = 9"),
    ((2, 3 * 64, 8, 6), dict(nhead=2, window=4), "does not divide"),
    ((2, 3 * 64, 8, 8), dict(nhead=2, window=4, shift=4), "shift = 4"),
    ((2, 3 * 64, 8, 8), dict(nhead=2, window=4, out="self"), "no self-loop"),
])
def test_init_connection_rejects(shape, keys, msg):
    with pytest.raises(Exception, match=msg):
        _layer(shape, **keys)
