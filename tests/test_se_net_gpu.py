"""The `ch_scale` layer and the global pooling kernel in a net on the GPU: a tiny squeeze-and-excitation
residual net against the CPU executor, the zero-copy splits in front of the SE modules, HIP-graph
replay, determinism, a batch-size change, launch hygiene, the torch path under precision = fp32, and
one step of SE-ResNet-18."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr

pytestmark = pytest.mark.gpu


def _se(p, hw, C, r=8):
    """the SE module on node <p>_n2: squeeze -> fullc(r) -> relu -> fullc(C) -> sigmoid -> ch_scale -> <p>_se"""
    return """layer[%(p)s_n2->%(p)s_sq,%(p)s_ex] = split
layer[%(p)s_sq->%(p)s_gp] = avg_pooling
  kernel_size = %(hw)d
  stride = 1
layer[%(p)s_gp->%(p)s_gf] = flatten
layer[%(p)s_gf->%(p)s_g1] = fullc:%(p)s_fc1
  nhidden = %(r)d
layer[%(p)s_g1->%(p)s_g2] = relu
layer[%(p)s_g2->%(p)s_g3] = fullc:%(p)s_fc2
  nhidden = %(C)d
layer[%(p)s_g3->%(p)s_gs] = sigmoid
layer[%(p)s_ex,%(p)s_gs->%(p)s_se] = ch_scale:%(p)s_scale""" % {"p": p, "hw": hw, "C": C, "r": r}


# conv -> bn -> relu, a 16-channel block with the identity shortcut whose squeeze pools 12 x 12 (144
# elements: the global pooling kernel), a 32-channel block that halves the resolution with a 1x1
# stride-2 projection shortcut whose squeeze pools 6 x 6 (the generic kernel), average pooling, fullc
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
%(se_a)s
layer[a_se,a_id->a] = add:a_add
  add_relu = 1
layer[a->b_x,b_id] = split
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
%(se_b)s
layer[b_id->b_cp] = conv:b_proj
  kernel_size = 1
  stride = 2
  nchannel = 32
  no_bias = 1
layer[b_cp->b_np] = batch_norm_ma:b_bnp
layer[b_se,b_np->b] = add:b_add
  add_relu = 1
layer[b->gap] = avg_pooling
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
""" % {"se_a": _se("a", 12, 16), "se_b": _se("b", 6, 32)}
# the first module's gate also feeds a side branch: it comes out of a split, which must keep copying
GATE_SPLIT = NET.replace("layer[a_g3->a_gs] = sigmoid", "layer[a_g3->a_g4] = sigmoid\nlayer[a_g4->a_gs,a_gt] = split") \
    .replace("layer[a->b_x,b_id] = split", "layer[a_gt->a_gu] = fullc:a_fc3\n  nhidden = 8\nlayer[a->b_x,b_id] = split")
BATCH = 8
DET = [("deterministic", "1")]


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


def _splits(tr):
    return [c for c in tr.net.connections if c.type == 23]


def test_one_step_matches_the_cpu_executor():
    """One training step from one seed on the GPU (bf16 HIP kernels) and on the CPU executor that
    keeps bf16 at node boundaries (tests/test_bn_ma_net_gpu.py): every parameter tensor and the
    output of a forward pass after the step agree within relerr 2e-2, each on its own scale.
    Measured on an MI355X: the worst is the output at 1.19e-3, then the first two batch norms'
    biases (2.1e-4, 2.5e-4) and the second gate's first fullc bias (1.3e-4); everything else, the
    running statistics included, at 1e-5 or below."""
    gpu, ora = _make("gpu"), _make("cpu")
    _bf16_at_node_boundaries(ora)
    for a, b in zip(_params(gpu), _params(ora)):
        assert relerr(a, b) < 1e-5  # the same seed starts both alike
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = [(gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    assert len(keys) == 6 + 2 * 6 + 2 * 4 + 2  # six convs, six batch norms, two gates of two fullc, the classifier
    errs = {k: round(relerr(a, b), 5) for k, a, b in zip(keys, _params(gpu), _params(ora))}
    probe = _batch(2)
    errs["output"] = round(relerr(torch.from_numpy(_raw(gpu, probe)), torch.from_numpy(_raw(ora, probe))), 5)
    serr = round(relerr(gpu.net.bn_state, ora.net.bn_state), 5)
    print("per tensor vs the bf16-node CPU executor", errs, "running statistics", serr)
    print("worst", max(errs.items(), key=lambda kv: kv[1]))
    assert max(errs.values()) < 2e-2, errs
    assert serr < 2e-2


def test_the_splits_in_front_of_the_se_modules_are_zero_copy():
    tr = _make()
    assert len(_splits(tr)) == 4
    for sp in _splits(tr):
        assert sp.layer.alias
        assert all(o.data.data_ptr() == sp.nodes_in[0].data.data_ptr() and o.grad_buf is not None for o in sp.nodes_out)
    for name in ("a_scale", "b_scale"):
        sc = tr.net.connections[tr.net_cfg.layer_name_map[name]]
        assert sc.type == 42 and sc.nodes_in[0].grad_buf is not None and sc.nodes_in[1].grad_buf is None
    # a split whose output is a gate keeps copying; the map's split next to it stays zero-copy
    tr = _make(conf=GATE_SPLIT)
    sc = tr.net.connections[tr.net_cfg.layer_name_map["a_scale"]]
    for sp in _splits(tr):
        is_gate = sc.nodes_in[1] in sp.nodes_out
        assert sp.layer.alias is (not is_gate)
        assert all((o.grad_buf is None) is is_gate for o in sp.nodes_out)
    tr.update(_batch(1))
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()


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
    assert all(sp.layer.alias for sp in _splits(fused))
    monkeypatch.setenv("CXXNET_FUSE", "0")
    plain = _make(extra=DET)
    assert not any(sp.layer.alias for sp in _splits(plain))
    _same(_two_steps(fused), _two_steps(plain))


def test_two_deterministic_runs_are_bitwise_equal():
    _same(_two_steps(_make(extra=DET)), _two_steps(_make(extra=DET)))


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
    for k in ("se_scale_fwd", "se_scale_bwd", "se_pool_fwd", "pool_fwd_rows"):  # 12 x 12 new, 6 x 6 generic
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
    tr.update(part)  # a training step at 5 rows, then at 8 again
    tr.update(full)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()
    assert np.isfinite(_raw(tr, full)).all()


def test_se_resnet18_one_step():
    """One training step of models/confs/se_resnet18.conf at batch 2: finite softmax rows that sum
    to 1, weights that moved, library kernels only.  No numeric comparison with the CPU executor,
    as for ResNet-18 (tests/test_add_net_gpu.py); the tiny net above carries the numerics."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("se_resnet18", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:  # (deterministic: no tile timing)
        tr.set_param(k, v)
    tr.init_model()
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    assert all(sp.layer.alias for sp in _splits(tr)) and len(_splits(tr)) == 16
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = tr.net.arena.w.clone()
    foreign, names = _foreign_kernels(tr, b)
    assert not foreign, foreign
    for k in ("se_scale_fwd", "se_scale_bwd", "se_pool_fwd", "se_merge"):
        assert any(k in n for n in names), (k, sorted(names))
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)  # (u = 2^-8 of a bf16 row)


def test_fp32_mode_runs_the_torch_formulas_on_the_device():
    """precision = fp32: the layer's torch path on device tensors (no workspace); one step agrees
    with the CPU executor to fp32 round-off."""
    from cxxnet_amd.ops.mode import set_reference_precision
    try:
        gpu = _make(extra=[("precision", "fp32")] + DET)
        sc = next(c.layer for c in gpu.net.connections if c.type == 42)
        assert not gpu.net.ctx.is_gpu and gpu.net.nodes[0].data.is_cuda
        gpu.update(_batch(1))
        assert sc._st is not None and sc._st.ws is None
        out = _raw(gpu, _batch(2))
        pg = _params(gpu)
    finally:
        set_reference_precision(False)
    cpu = _make("cpu")
    cpu.update(_batch(1))
    for a, b in zip(pg, _params(cpu)):
        assert relerr(a, b) < 1e-3
    assert relerr(torch.from_numpy(out), torch.from_numpy(_raw(cpu, _batch(2)))) < 1e-3
