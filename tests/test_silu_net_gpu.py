"""The `silu` and `drop_path` layers in a net on the GPU: a tiny EfficientNet-style net against the CPU
executor, determinism, HIP-graph replay, a batch-size change, the torch path under precision = fp32,
launch hygiene, and one step of EfficientNet-B0."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr
from test_drop_path_cpu import _np_keep

pytestmark = pytest.mark.gpu


def _cba(src, p, tag, act, k, C, stride=1, groups=1):
    """conv k x k (no bias) -> batch_norm_ma [-> act] from node src to node <p>_<tag>a (<p>_<tag>n without act)"""
    s = "layer[%s->%s_%s] = conv:%s_%s\n  kernel_size = %d\n  pad = %d\n  stride = %d\n  nchannel = %d\n  no_bias = 1\n" % (
        src, p, tag, p, tag, k, k // 2, stride, C)
    if groups > 1:
        s += "  ngroup = %d\n" % groups
    s += "layer[%s_%s->%s_%sn] = batch_norm_ma:%s_%s_bn\n" % (p, tag, p, tag, p, tag)
    if act:
        s += "layer[%s_%sn->%s_%sa] = %s\n" % (p, tag, p, tag, act)
    return s


# stem conv -> bn -> silu; an MBConv block at 12 x 12: 1x1 to 32 -> bn -> silu -> 5x5 depthwise -> bn ->
# silu -> SE (squeeze of 144 pixels: the global pooling kernel; silu in the squeeze; gate: sigmoid) -> 1x1
# to 16 -> bn -> drop_path 0.5 -> add with the block input; a stride-2 block: 1x1 to 32 -> bn -> silu ->
# 3x3 / 2 depthwise -> bn -> silu -> 1x1 to 24 -> bn; global average pooling, fullc, softmax
NET = "netconfig=start\n" + _cba("0", "s", "c", "silu", 3, 16) + \
    "layer[s_ca->a_x,a_id] = split\n" + _cba("a_x", "a", "e", "silu", 1, 32) + \
    _cba("a_ea", "a", "d", "silu", 5, 32, groups=32) + """layer[a_da->a_sq,a_ex] = split
layer[a_sq->a_gp] = avg_pooling
  kernel_size = 12
  stride = 1
layer[a_gp->a_gf] = flatten
layer[a_gf->a_g1] = fullc:a_fc1
  nhidden = 8
layer[a_g1->a_g2] = silu
layer[a_g2->a_g3] = fullc:a_fc2
  nhidden = 32
layer[a_g3->a_gs] = sigmoid
layer[a_ex,a_gs->a_se] = ch_scale:a_scale
""" + _cba("a_se", "a", "p", None, 1, 16) + """layer[a_pn->a_pn] = drop_path:a_dp
  drop_prob = 0.5
layer[a_pn,a_id->a] = add:a_add
  add_relu = 0
""" + _cba("a", "b", "e", "silu", 1, 32) + _cba("b_ea", "b", "d", "silu", 3, 32, stride=2, groups=32) + \
    _cba("b_da", "b", "p", None, 1, 24) + """layer[b_pn->gap] = avg_pooling
  kernel_size = 6
  stride = 1
layer[gap->flat] = flatten
layer[flat->fc] = fullc:fc
  nhidden = 10
layer[fc->fc] = softmax
netconfig=end
input_shape = 8,12,12
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
bn_momentum = 0.75
"""
BATCH = 8
DET = [("deterministic", "1")]
NEW_KERNELS = ("silu_fwd", "silu_bwd", "drop_path_apply")


def _trainer(dev="gpu", conf=NET, extra=()):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf)) + [
            ("batch_size", str(BATCH)), ("dev", dev), ("eval_train", "0"), ("silent", "1"), ("seed", "3"),
            ("cuda_graph", "0"), ("launch_replay", "0")] + list(extra):
        tr.set_param(k, v)
    return tr


def _make(*args, **kw):
    tr = _trainer(*args, **kw)
    tr.init_model()
    return tr


def _batch(seed, n=BATCH):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(n, 8, 12, 12, generator=g), torch.randint(0, 10, (n, 1), generator=g).float())


def _params(tr):
    return [tr.net.arena.w[s.offset:s.offset + s.numel].detach().cpu().clone() for _, s in tr.net.arena.specs]


def _raw(tr, batch):
    return tr.forward_to([len(tr.net.nodes) - 1], batch)[0].copy()


def _drop_path(tr):
    return next(c.layer for c in tr.net.connections if c.type == 48)


def test_the_net_has_every_new_layer_and_a_mixed_mask():
    tr = _make()
    types = [c.type for c in tr.net.connections]
    assert types.count(47) == 6 and types.count(48) == 1 and types.count(4) == 1
    assert types.count(41) == 1 and types.count(42) == 1 and types.count(10) == 7
    assert tr.net.nodes[-1].shape == (BATCH, 1, 1, 10)
    dp = _drop_path(tr)
    assert dp.drop_prob == 0.5 and dp.seed == _drop_path(_make("cpu")).seed
    masks = [_np_keep(BATCH, dp.seed, step, 0.5) for step in (1, 2, 3)]  # the counter of training steps 1, 2, 3
    for m in masks:
        assert m.any() and not m.all(), "the seed must keep some samples and drop some"
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    assert _np_keep(5, dp.seed, 2, 0.5).any() and not _np_keep(5, dp.seed, 2, 0.5).all()  # and at batch 5


def test_one_step_matches_the_cpu_executor():
    """One training step from one seed on the GPU (bf16 HIP kernels) and on the CPU executor that
    keeps bf16 at node boundaries (tests/test_bn_ma_net_gpu.py), both dropping the same samples of the
    residual branch: every parameter tensor and the output of a forward pass after the step agree
    within relerr 2e-2, each on its own scale, the project's threshold for these nets.  The
    per-tensor values are printed."""
    gpu, ora = _make("gpu"), _make("cpu")
    _bf16_at_node_boundaries(ora)
    for a, b in zip(_params(gpu), _params(ora)):
        assert relerr(a, b) < 1e-5  # the same seed starts both alike
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = [(gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    assert len(keys) == 7 + 2 * 7 + 2 * 2 + 2  # seven convs, seven batch norms, the gate's two fullc, the classifier
    errs = {k: round(relerr(a, b), 5) for k, a, b in zip(keys, _params(gpu), _params(ora))}
    probe = _batch(2)
    errs["output"] = round(relerr(torch.from_numpy(_raw(gpu, probe)), torch.from_numpy(_raw(ora, probe))), 5)
    serr = round(relerr(gpu.net.bn_state, ora.net.bn_state), 5)
    print("per tensor vs the bf16-node CPU executor", errs, "running statistics", serr)
    print("worst", max(errs.items(), key=lambda kv: kv[1]))
    assert max(errs.values()) < 2e-2, errs
    assert serr < 2e-2


def _two_steps(tr):
    tr.update(_batch(1))
    tr.update(_batch(2))
    torch.cuda.synchronize()
    return _params(tr), _raw(tr, _batch(5)), tr.net.bn_state.cpu().clone()


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0]))
    assert np.array_equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_two_deterministic_runs_are_bitwise_equal():
    _same(_two_steps(_make(extra=DET)), _two_steps(_make(extra=DET)))


def test_graph_replay_equals_eager_steps():
    """three steps, the last two replayed from the captured graph: drop_path reads the step counter on the
    device, so each replay draws the mask the eager step drew (the masks of steps 2 and 3 differ:
    test_the_net_has_every_new_layer_and_a_mixed_mask)"""
    res = []
    for graph in (0, 1):
        tr = _make(extra=[("cuda_graph", str(graph))] + DET)
        for seed in (1, 2, 3):  # eager, capture + replay, replay
            tr.update(_batch(seed))
        torch.cuda.synchronize()
        if graph:
            assert tr._graphs, "the step was not captured"
        assert int(tr.net.ctx.step_counter.item()) == 3
        res.append((_params(tr), _raw(tr, _batch(5)), tr.net.bn_state.cpu().clone()))
    _same(*res)


def _foreign_kernels(tr, b):
    """tests/test_launch_hygiene_gpu.py's check: the names of the at::native kernels of one
    forward + backward, and all kernel names."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(2):  # tile tuning and lazy buffers happen in the first steps
        tr.update(b)
    tr._set_batch(b)
    net = tr.net
    net.forward(True)
    net.backprop(False, first=True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        net.forward(True)
        net.backprop(False, first=True)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}
    return sorted(n for n in names if "at::native" in n), names


def test_forward_backward_launch_only_library_kernels():
    foreign, names = _foreign_kernels(_make(), _batch(1))
    assert not foreign, foreign
    for k in NEW_KERNELS + ("se_pool_fwd", "se_scale_fwd"):
        assert any(k in n for n in names), (k, sorted(names))


def test_a_batch_size_change_8_5_8():
    from cxxnet_amd.io.data import DataBatch
    tr = _make(extra=DET)
    tr.update(_batch(1))
    full = _batch(4)
    want = _raw(tr, full)[:5]
    part = DataBatch(full.data[:5].clone(), full.label[:5].clone())
    got = _raw(tr, part)
    assert tr.net.cur_batch == 5
    assert np.array_equal(got, want)
    tr.update(part)  # a training step at 5 rows (drop_path on 5 samples), then at 8 again
    tr.update(full)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()
    assert np.isfinite(_raw(tr, full)).all()


def test_fp32_mode_runs_the_torch_formulas_on_the_device():
    """precision = fp32: the layers' torch path on device tensors, drop_path's mirror hash included; one
    step agrees with the CPU executor to fp32 round-off."""
    from cxxnet_amd.ops.mode import set_reference_precision
    try:
        gpu = _make(extra=[("precision", "fp32")] + DET)
        assert not gpu.net.ctx.is_gpu and gpu.net.nodes[0].data.is_cuda
        gpu.update(_batch(1))
        out = _raw(gpu, _batch(2))
        pg = _params(gpu)
    finally:
        set_reference_precision(False)
    cpu = _make("cpu")
    cpu.update(_batch(1))
    for a, b in zip(pg, _params(cpu)):
        assert relerr(a, b) < 1e-3
    assert relerr(torch.from_numpy(out), torch.from_numpy(_raw(cpu, _batch(2)))) < 1e-3


def test_efficientnet_b0_one_step():
    """One deterministic training step of models/confs/efficientnet_b0.conf at batch 2: the layer counts,
    finite softmax rows that sum to 1, weights that moved, library kernels only -- the new ones and the
    global pooling kernel among them.  No numeric comparison with the CPU executor, as for the other zoo
    nets; the tiny net above carries the numerics."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("efficientnet_b0", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:  # (deterministic: no tile timing)
        tr.set_param(k, v)
    tr.init_model()
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    types = [c.type for c in tr.net.connections]
    assert types.count(47) == 49 and types.count(48) == 9 and types.count(42) == 16 and types.count(41) == 9
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = tr.net.arena.w.clone()
    foreign, names = _foreign_kernels(tr, b)
    assert not foreign, foreign
    for k in NEW_KERNELS + ("se_pool_fwd", "se_scale_fwd", "se_scale_bwd"):
        assert any(k in n for n in names), (k, sorted(names))
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and (np.abs(out.sum(1) - 1.0) <= 2.0 ** -8).all()  # (u = 2^-8 of a bf16 row)
