"""The `add` layer in a net on the GPU: a tiny residual net against the CPU executor, the zero-copy
split in front of the add, HIP-graph replay, launch hygiene, a batch-size change, the non-negative
marking of its output, one step of ResNet-18, and the torch path under precision = fp32."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr

pytestmark = pytest.mark.gpu

# conv -> bn -> relu, a block with the identity shortcut, [a max pooling,] a block that halves the
# resolution with a 1x1 stride-2 projection shortcut, average pooling, fullc, softmax
NET = """
netconfig=start
layer[0->c0] = conv:c0
  kernel_size = 3
  pad = 1
  nchannel = 16
  no_bias = 1
layer[c0->n0] = batch_norm_ma:bn0
layer[n0->r0] = relu
layer[r0->a_x,a_id] = split
layer[a_x->a_c1] = conv:a_c1
  kernel_size = 3
  pad = 1
  nchannel = 16
  no_bias = 1
layer[a_c1->a_n1] = batch_norm_ma:a_bn1
layer[a_n1->a_r1] = relu
layer[a_r1->a_c2] = conv:a_c2
  kernel_size = 3
  pad = 1
  nchannel = 16
  no_bias = 1
layer[a_c2->a_n2] = batch_norm_ma:a_bn2
layer[a_n2,a_id->a] = add:a_add
  add_relu = 1
%(pool)s
layer[%(a)s->b_x,b_id] = split
layer[b_x->b_c1] = conv:b_c1
  kernel_size = 3
  pad = 1
  stride = 2
  nchannel = 32
  no_bias = 1
layer[b_c1->b_n1] = batch_norm_ma:b_bn1
layer[b_n1->b_r1] = relu
layer[b_r1->b_c2] = conv:b_c2
  kernel_size = 3
  pad = 1
  nchannel = 32
  no_bias = 1
layer[b_c2->b_n2] = batch_norm_ma:b_bn2
layer[b_id->b_cp] = conv:b_proj
  kernel_size = 1
  stride = 2
  nchannel = 32
  no_bias = 1
layer[b_cp->b_np] = batch_norm_ma:b_bnp
layer[b_n2,b_np->b] = add:b_add
  add_relu = 1
layer[b->gap] = avg_pooling
  kernel_size = %(gap)d
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
PLAIN = NET % {"pool": "", "a": "a", "gap": 6}
POOLED = NET % {"pool": "layer[a->ap] = max_pooling\n  kernel_size = 2\n  stride = 2", "a": "ap", "gap": 3}
BATCH = 8
DET = [("deterministic", "1")]


def _trainer(dev="gpu", conf=PLAIN, extra=()):
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


def _splits(tr):
    return [c for c in tr.net.connections if c.type == 23]


def test_one_step_matches_the_cpu_executor():
    """One training step from one seed on the GPU (bf16 HIP kernels) and on the CPU executor that
    keeps bf16 at node boundaries (tests/test_bn_ma_net_gpu.py): every parameter tensor and the
    output of a forward pass after the step agree within relerr 2e-2, each on its own scale.
    Measured on an MI355X: the worst tensor is the first batch norm's bias at 2.85e-3, then the
    other batch norms' biases (1.74e-3, 1.05e-3, 5.9e-4), the output at 9.1e-4, the conv weights at
    6e-5 and below; everything else, the running statistics included, below 1e-5."""
    gpu, ora = _make("gpu"), _make("cpu")
    _bf16_at_node_boundaries(ora)
    for a, b in zip(_params(gpu), _params(ora)):
        assert relerr(a, b) < 1e-5  # the same seed starts both alike
    assert all(sp.layer.alias for sp in _splits(gpu)) and not any(sp.layer.alias for sp in _splits(ora))
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = [(gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    assert len(keys) == 6 + 2 * 6 + 2  # six convs, six batch norms, the classifier
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


def test_aliased_split_equals_the_copying_split(monkeypatch):
    fused = _make(extra=DET)
    assert len(_splits(fused)) == 2
    for sp in _splits(fused):
        assert sp.layer.alias
        assert all(o.data.data_ptr() == sp.nodes_in[0].data.data_ptr() and o.grad_buf is not None for o in sp.nodes_out)
    monkeypatch.setenv("CXXNET_FUSE", "0")
    plain = _make(extra=DET)
    for sp in _splits(plain):
        assert not sp.layer.alias
        assert all(o.data.data_ptr() != sp.nodes_in[0].data.data_ptr() and o.grad_buf is None for o in sp.nodes_out)
    _same(_two_steps(fused), _two_steps(plain))


def test_graph_replay_equals_eager_steps():
    res = []
    for graph in (0, 1):
        tr = _make(extra=[("cuda_graph", str(graph))] + DET)
        for seed in (1, 2, 3):  # eager, capture + replay, replay
            tr.update(_batch(seed))
        torch.cuda.synchronize()
        if graph:
            assert tr._graphs, "the step was not captured"
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
    assert any("add_fwd" in n for n in names) and any("add_bwd" in n for n in names), sorted(names)


def test_a_smaller_batch_gives_the_same_rows():
    from cxxnet_amd.io.data import DataBatch
    tr = _make(extra=DET)
    tr.update(_batch(1))
    full = _batch(4)
    want = _raw(tr, full)[:5]
    part = DataBatch(full.data[:5].clone(), full.label[:5].clone())
    got = _raw(tr, part)
    assert tr.net.cur_batch == 5
    assert np.array_equal(got, want)
    tr.update(part)  # a training step at 5 rows, then at 8 again: the mask covers every size
    tr.update(full)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()


def test_max_pooling_behind_the_add_takes_the_nonneg_path(monkeypatch):
    def pool_of(tr):
        return next(c.layer for c in tr.net.connections if c.type == 11)
    marked = _make(conf=POOLED, extra=DET)
    assert pool_of(marked).input_nonneg is True
    general = _make(conf=POOLED, extra=DET)
    pool_of(general).input_nonneg = False  # the same net through the general max-pooling kernels
    monkeypatch.setenv("CXXNET_FUSE", "0")
    unfused = _make(conf=POOLED, extra=DET)
    assert not any(sp.layer.alias for sp in _splits(unfused))
    a, b, c = _two_steps(marked), _two_steps(general), _two_steps(unfused)
    _same(a, b)
    _same(a, c)
    # without add_relu the output is not marked
    tr = _make(conf=POOLED.replace("layer[a_n2,a_id->a] = add:a_add\n  add_relu = 1", "layer[a_n2,a_id->a] = add:a_add"))
    assert pool_of(tr).input_nonneg is False


def test_resnet18_one_step():
    """One training step of models/confs/resnet18.conf at batch 2: finite softmax rows that sum
    to 1, weights that moved, library kernels only.  No numeric comparison with the CPU executor:
    twenty batch norms at batch 2 amplify storage rounding beyond any derived tolerance; the tiny
    net above carries the numerics."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("resnet18", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:  # (deterministic: no tile timing)
        tr.set_param(k, v)
    tr.init_model()
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    assert all(sp.layer.alias for sp in _splits(tr)) and len(_splits(tr)) == 8
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = tr.net.arena.w.clone()
    foreign, names = _foreign_kernels(tr, b)
    assert not foreign, foreign
    assert any("add_fwd" in n for n in names) and any("add_bwd" in n for n in names)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)  # (u = 2^-8 of a bf16 row)


def test_fp32_mode_runs_the_torch_formulas_on_the_device():
    """precision = fp32: the layer's torch path (bool mask) on device tensors; one step agrees
    with the CPU executor to fp32 round-off."""
    from cxxnet_amd.ops.mode import set_reference_precision
    try:
        gpu = _make(extra=[("precision", "fp32")] + DET)
        add = next(c.layer for c in gpu.net.connections if c.type == 41)
        assert not gpu.net.ctx.is_gpu and gpu.net.nodes[0].data.is_cuda
        gpu.update(_batch(1))
        assert add._st is not None and add._st.mask.dtype == torch.bool and add._st.mask.is_cuda
        out = _raw(gpu, _batch(2))
        pg = _params(gpu)
    finally:
        set_reference_precision(False)
    cpu = _make("cpu")
    cpu.update(_batch(1))
    for a, b in zip(pg, _params(cpu)):
        assert relerr(a, b) < 1e-3
    assert relerr(torch.from_numpy(out), torch.from_numpy(_raw(cpu, _batch(2)))) < 1e-3
