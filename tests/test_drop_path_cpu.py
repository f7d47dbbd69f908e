"""The `drop_path` layer (type id 48) and ops.layer_ops.drop_path_apply on the CPU executor: the torch path
against an independent numpy evaluation of the counter hash, the +0 of a dropped sample, eval and
drop_prob = 0, the connection checks, and the kept fraction of the mirror.  CPU only."""
import numpy as np
import pytest
import torch

from cxxnet_amd.ops import layer_ops as L
from cxxnet_amd.ops.nn import dropout_mask_ref, effective_seed

SEEDS = (1, 12345, 2 ** 31 - 2)


# ------------------------------------------------------------------ an independent numpy mirror
def _np_hash(idx, seed):
    """hash_u32 of csrc/kernels/common.h in uint32 arithmetic (numpy wraps as the device does)"""
    with np.errstate(over="ignore"):
        x = np.asarray(idx, dtype=np.uint32) ^ (np.uint32(seed) * np.uint32(0x9E3779B9))
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def _np_keep(B, seed, counter, pkeep):
    s = int(_np_hash(np.array([counter]), seed)[0]) if counter is not None else seed
    t = min(int(float(np.float32(pkeep)) * 4294967296.0), 0xFFFFFFFF)   # dropout_thresh of the fp32 pkeep
    return _np_hash(np.arange(B), s) < np.uint32(t)


def _np_drop_path(x_bf16, seed, counter, pkeep):
    """bf16 tensor [B][...] -> the expected bf16 tensor: one fp32 product, one rounding; a selection"""
    B = x_bf16.shape[0]
    keep = _np_keep(B, seed, counter, pkeep)
    scale = np.float32(1.0) / np.float32(pkeep)
    v = torch.from_numpy(x_bf16.float().numpy().reshape(B, -1) * scale).to(torch.bfloat16)
    out = torch.where(torch.from_numpy(keep).view(B, 1), v, torch.zeros_like(v))
    return out.view(x_bf16.shape), keep


def _bits(t):
    return t.contiguous().view(torch.int16)


def _fresh(seed=0):
    from cxxnet_amd.layers import LayerContext, create_layer
    return create_layer(48, LayerContext(torch.device("cpu"), seed))


def _node(shape):
    from cxxnet_amd.layers import Node
    n = Node("a")
    n.set_shape(*shape)
    return n


@pytest.mark.parametrize("counter", [None, 0, 7])
@pytest.mark.parametrize("B,n,pkeep", [(8, 8, 0.5), (8, 7, 0.8), (3, 9, 0.5), (64, 5, 0.95), (1, 33, 0.5)])
def test_the_torch_path_is_the_numpy_mirror(B, n, pkeep, counter):
    for seed in SEEDS:
        g = torch.Generator().manual_seed(B * 100 + n)
        x = (4.0 * torch.randn(B, n, generator=g)).to(torch.bfloat16)
        want, keep = _np_drop_path(x, seed, counter, pkeep)
        got = x.clone()
        ctr = torch.tensor([counter], dtype=torch.int32) if counter is not None else None
        L.drop_path_apply(got, seed, pkeep, ctr)
        assert torch.equal(_bits(got), _bits(want))
        # the draw is dropout's mask at element b (ops/nn.py), here with the threshold of the fp32 pkeep
        m = dropout_mask_ref(B, effective_seed(seed, ctr), pkeep) > 0
        assert np.array_equal(m.numpy(), keep)
        assert np.array_equal(L.drop_path_keep_ref(B, effective_seed(seed, ctr), pkeep).numpy(), keep)


def test_a_dropped_sample_holding_inf_and_nan_becomes_plus_zero():
    B, n, pkeep, seed = 16, 12, 0.5, 12345
    keep = _np_keep(B, seed, 3, pkeep)
    assert keep.any() and not keep.all()
    x = torch.full((B, n), -2.0, dtype=torch.bfloat16)
    x[:, 0], x[:, 1], x[:, 2] = float("inf"), float("nan"), -0.0
    got = x.clone()
    L.drop_path_apply(got, seed, pkeep, torch.tensor([3], dtype=torch.int32))
    for b in range(B):
        if keep[b]:
            assert got[b, 0] == float("inf") and torch.isnan(got[b, 1]) and _bits(got)[b, 2] == -32768
            assert (got[b, 3:] == -4.0).all()
        else:
            assert (_bits(got)[b] == 0).all()  # +0, not -0 and not NaN: a selection, not x * 0


def test_eval_and_drop_prob_0_leave_the_bits_alone():
    x0 = torch.randn(4, 3, 2, 2).to(torch.bfloat16)
    x0[0, 0, 0, 0] = float("nan")
    for prob, train in ((0.5, False), (0.0, True), (0.0, False)):
        lay = _fresh()
        lay.set_param("drop_prob", str(prob))
        a = _node((4, 3, 2, 2))
        lay.init_connection([a], [a])
        a.alloc("cpu", torch.bfloat16)
        a.data.copy_(x0.view(a.data.shape))
        lay.forward(train, [a], [a])
        assert torch.equal(_bits(a.data), _bits(x0.view(a.data.shape)))
        lay.backprop(True, [a], [a])
        assert torch.equal(_bits(a.data), _bits(x0.view(a.data.shape)))


def test_the_layer_applies_one_mask_forward_and_backward_and_a_new_one_per_step():
    lay = _fresh(seed=3)
    lay.set_param("drop_prob", "0.5")
    lay.set_param("threshold", "0.9")  # dropout's key: not this layer's
    assert lay.drop_prob == 0.5
    a = _node((16, 3, 2, 2))
    lay.init_connection([a], [a])
    a.alloc("cpu", torch.float32)
    masks = []
    for step in (0, 1):
        lay.ctx.step_counter = torch.tensor([step], dtype=torch.int32)
        keep = _np_keep(16, lay.seed, step, 0.5)
        a.data.fill_(1.5)
        lay.forward(True, [a], [a])
        want = torch.where(torch.from_numpy(keep).view(16, 1, 1, 1), torch.tensor(3.0), torch.tensor(0.0))
        assert torch.equal(a.data, want.expand_as(a.data))
        a.data.fill_(-0.25)  # the gradient the node now holds
        lay.backprop(True, [a], [a])
        assert torch.equal(a.data, (want / -6.0).expand_as(a.data) + 0.0)
        masks.append(keep)
    assert not np.array_equal(masks[0], masks[1])


def test_connection_and_key_checks():
    a, b = _node((2, 3, 4, 5)), _node((2, 3, 4, 5))
    with pytest.raises(ValueError, match="DropPathLayer is a self-loop Layer"):
        _fresh().init_connection([a], [b])
    with pytest.raises(ValueError, match="DropPathLayer"):
        _fresh().init_connection([a, b], [a])
    for bad in ("1", "1.0", "-0.1", "1.5"):
        lay = _fresh()
        lay.set_param("drop_prob", bad)
        with pytest.raises(ValueError, match="drop_prob"):
            lay.init_connection([a], [a])
    p = _node((2, 3, 4, 5))
    p.cp = 4
    with pytest.raises(ValueError, match="padded-channel"):
        _fresh().init_connection([p], [p])
    lay = _fresh()
    lay.set_param("drop_prob", "0.999")
    lay.init_connection([a], [a])
    with pytest.raises(ValueError, match="pkeep"):
        L.drop_path_apply(torch.zeros(2, 2), 1, 0.0)
    with pytest.raises(ValueError, match="drop_path"):
        L.drop_path_apply(torch.zeros(4, 4)[:, :2], 1, 0.5)


def test_the_kept_fraction_of_the_mirror():
    """B = 4096 samples of one element at pkeep = 0.8: the kept count of a fair draw is binomial with mean
    3276.8 and standard deviation sqrt(4096 0.8 0.2) = 25.6; the mirror alone and the layer's torch path stay
    within 5 of them, +-128 of 3277, for each fixed seed and a few counter values."""
    B, pkeep = 4096, 0.8
    for seed in SEEDS:
        for counter in (None, 0, 1, 1000):
            keep = _np_keep(B, seed, counter, pkeep)
            assert abs(int(keep.sum()) - 3277) <= 128, (seed, counter, int(keep.sum()))
            x = torch.ones(B, 1)
            L.drop_path_apply(x, seed, pkeep, torch.tensor([counter], dtype=torch.int32) if counter is not None else None)
            assert int((x != 0).sum()) == int(keep.sum())
            assert ((x == 0) | (x == float(np.float32(1.0) / np.float32(0.8)))).all()
