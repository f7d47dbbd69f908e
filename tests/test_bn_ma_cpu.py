"""batch_norm_ma on the CPU executor: formulas, running statistics, row-independent inference,
checkpoint layout and round trip, finetune copies, reset_to, layer flags."""
import struct

import numpy as np
import pytest
import torch

CONF = """
netconfig=start
layer[0->1] = batch_norm_ma:bn1
  bn_momentum = 0.75
  init_slope = 1.5
  init_bias = 0.25
layer[1->2] = relu
layer[2->3] = flatten
layer[3->4] = fullc:f1
  nhidden = 6
layer[4->4] = batch_norm_ma:bn2
  bn_momentum = 0.75
layer[4->5] = fullc:f2
  nhidden = 4
layer[5->5] = softmax
netconfig=end
input_shape = 3,2,2
random_type = xavier
eta = 0.1
momentum = 0.9
wd = 0.0001
"""
C1, B = 3, 6


def _trainer(extra=(), seed=5):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(CONF)) + [("batch_size", str(B)), ("dev", "cpu"), ("eval_train", "0"),
                                                        ("silent", "1"), ("seed", str(seed))] + list(extra):
        tr.set_param(k, v)
    return tr


def _make(extra=(), seed=5):
    tr = _trainer(extra, seed)
    tr.init_model()
    return tr


def _batch(seed, n=B):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(n, C1, 2, 2, generator=g) * 2 + 1, torch.randint(0, 4, (n, 1), generator=g).float())


def _raw(tr, batch):
    return tr.forward_to([len(tr.net.nodes) - 1], batch)[0].copy()  # (on the CPU the array may view the node)


def _bn(tr, name="bn1"):
    return tr.net.connections[tr.net_cfg.layer_name_map[name]].layer


@pytest.mark.parametrize("R,C", [(6, 5), (12, 3)])
def test_forward_backward_formulas(R, C):
    from cxxnet_amd.ops import layer_ops as L
    gen = torch.Generator().manual_seed(R)
    x = torch.randn(R, C, generator=gen) * 1.5 + 0.5
    gy = torch.randn(R, C, generator=gen)
    slope, bias = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    gslope, gbias = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    gs0, gb0 = gslope.clone(), gbias.clone()
    eps = 1e-5
    xd = x.double().requires_grad_()
    sd, bd = slope.double().requires_grad_(), bias.double().requires_grad_()
    mean = xd.sum(0) / R
    var = ((xd - mean) ** 2).sum(0) / R
    yd = (xd - mean) / torch.sqrt(var + eps) * sd + bd
    yd.backward(gy.double())

    st = L.BNMAState(C, R, "cpu", torch.float32, False)
    rmean, rvar = torch.zeros(C), torch.ones(C)
    y, xin = torch.empty(R, C), x.clone()
    L.bn_ma_forward(xin, y, slope, bias, eps, 0.9, st, rmean, rvar, True)
    assert torch.equal(xin, x), "the input node must not be overwritten"
    dx = xin  # backward overwrites x with dx
    L.bn_ma_backward(gy, xin, dx, slope, gslope, gbias, st, True)

    def close(a, b):
        return torch.allclose(a.double(), b, rtol=1e-5, atol=1e-5 * b.abs().max().item())
    assert close(y, yd.detach())
    assert close(dx, xd.grad)
    assert close(gslope, gs0.double() + sd.grad)
    assert close(gbias, gb0.double() + bd.grad)
    assert (gs0 != 0).all() and (gb0 != 0).all()
    # prop_grad = False leaves dx alone and still accumulates
    keep = torch.full((R, C), 7.0)
    L.bn_ma_backward(gy, x, keep, slope, gslope, gbias, st, False)
    assert (keep == 7.0).all()
    assert close(gslope, gs0.double() + 2 * sd.grad)


def test_running_statistics_recurrence():
    tr = _make()
    bn = _bn(tr)
    assert torch.equal(bn.rmean, torch.zeros(C1)) and torch.equal(bn.rvar, torch.ones(C1))
    m = 0.75
    rm, rv = torch.zeros(C1, dtype=torch.float64), torch.ones(C1, dtype=torch.float64)
    for seed in (1, 2):
        b = _batch(seed)
        tr._set_batch(b)
        tr.net.forward(True)
        x = b.data.double().permute(0, 2, 3, 1).reshape(-1, C1)
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)  # biased
        rm = m * rm + (1 - m) * mean
        rv = m * rv + (1 - m) * var
    assert torch.allclose(bn.rmean.double(), rm, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bn.rvar.double(), rv, rtol=1e-5, atol=1e-6)
    # views into the net's one flat buffer; not parameters
    assert tr.net.bn_state.numel() == 2 * C1 + 2 * 6
    assert bn.rmean.data_ptr() == tr.net.bn_state.data_ptr()
    lo, hi = tr.net.arena.w.data_ptr(), tr.net.arena.w.data_ptr() + 4 * tr.net.arena.w.numel()
    assert not lo <= tr.net.bn_state.data_ptr() < hi
    assert [s.tag for s in bn.params] == ["wmat", "bias"]


def test_running_statistics_move_every_micro_batch():
    tr = _make([("update_period", "2")])
    before = tr.net.bn_state.clone()
    tr.update(_batch(1))
    mid = tr.net.bn_state.clone()
    tr.update(_batch(2))
    assert not torch.equal(before, mid) and not torch.equal(mid, tr.net.bn_state)


def test_inference_is_row_independent():
    tr = _make()
    for seed in (1, 2):
        tr.update(_batch(seed))
    a, b = _batch(3), _batch(4)
    b.data[0] = a.data[0]
    ya, yb = _raw(tr, a), _raw(tr, b)
    assert np.array_equal(ya[0], yb[0])
    assert not np.array_equal(ya[1], yb[1])
    state = tr.net.bn_state.clone()
    _raw(tr, a)
    assert torch.equal(state, tr.net.bn_state), "inference must not move the running statistics"


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
    assert torch.equal(tr2.net.bn_state, tr.net.bn_state)
    # the model file stores the type id and the layer's blob is slope, bias, running_mean, running_var
    assert tr2.net_cfg.layers[0].type == 40
    from cxxnet_amd.layers.base import BinWriter
    fo = BinWriter()
    tr.net.save_model(fo)
    blob = fo.getvalue()
    assert data.endswith(blob)
    bn = _bn(tr)
    got, _ = _tensors(blob, 0, 4)  # bn1 is layer 0: its blob comes first
    for t, ref in zip(got, (bn.params[0].w, bn.params[1].w, bn.rmean, bn.rvar)):
        assert t.shape == (C1,) and np.array_equal(t, ref.numpy())
    assert not np.array_equal(got[2], np.zeros(C1)) and not np.array_equal(got[3], np.ones(C1))


def test_finetune_copies_running_statistics_by_name():
    src = _make()
    for seed in (1, 2):
        src.update(_batch(seed))
    data = src.save_model()
    for how in ("bytes", "trainer"):
        dst = _make(seed=123)
        assert not torch.equal(dst.net.bn_state, src.net.bn_state)
        if how == "bytes":
            dst.copy_model_from_bytes(data)
        else:
            dst.copy_model_from(src)
        assert torch.equal(dst.net.bn_state, src.net.bn_state), how
        assert torch.equal(_bn(dst, "bn2").rvar, _bn(src, "bn2").rvar)
        assert torch.equal(_bn(dst).params[0].w, _bn(src).params[0].w)
        probe = _batch(9)
        assert np.array_equal(_raw(dst, probe), _raw(src, probe))


def test_reset_to_restores_running_statistics():
    src = _make()
    for seed in (1, 2):
        src.update(_batch(seed))
    tr = _trainer(seed=3)
    tr.load_model(src.save_model())  # post-init values that are not 0 / 1
    w0, s0 = tr.net.arena.w.clone(), tr.net.bn_state.clone()
    ptr = tr.net.bn_state.data_ptr()
    first = []
    for rnd in range(2):
        for seed in (4, 5):
            tr.update(_batch(seed))
        first.append(tr.net.bn_state.clone())
        assert not torch.equal(tr.net.bn_state, s0)
        tr.reset_to(w0)
        assert torch.equal(tr.net.bn_state, s0) and tr.net.bn_state.data_ptr() == ptr
    assert torch.equal(first[0], first[1])


def test_layer_flags_and_type_ids():
    from cxxnet_amd import native
    from cxxnet_amd.layers import LayerContext, create_layer
    lay = create_layer(40, LayerContext(torch.device("cpu")))
    assert type(lay).__name__ == "BatchNormMALayer" and lay.replay_safe() is False
    assert type(lay).__dict__["replay_audited"] is False
    rt = native.rt()
    assert rt.get_layer_type("batch_norm_ma") == 40
    assert rt.get_layer_type("batch_norm") == 30
    with pytest.raises(Exception):
        lay.set_param("bn_momentum", "1.0")


def test_nets_without_the_layer_have_no_state():
    from test_dp_gloo import _make as make_plain
    tr = make_plain(4)
    assert tr.net.bn_state is None


def test_pairtest_rejects_the_layer():
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    conf = CONF.replace("layer[4->4] = batch_norm_ma:bn2", "layer[4->4] = pairtest-batch_norm_ma-batch_norm_ma:bn2")
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf)) + [("batch_size", str(B)), ("dev", "cpu"), ("silent", "1")]:
        tr.set_param(k, v)
    with pytest.raises(ValueError, match="pairtest"):
        tr.init_model()
