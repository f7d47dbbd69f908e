"""Depthwise convolutions in a net on the GPU: a tiny separable net against the CPU executor,
deterministic mode, HIP-graph and launch-list replay, launch hygiene, a batch-size change, a
checkpoint round trip of the depthwise weights, and one step of MobileNet-v1."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr

pytestmark = pytest.mark.gpu

BATCH = 8
DET = [("deterministic", "1")]
TAIL = """input_shape = 8,12,12
random_type = xavier
eta = 0.05
momentum = 0.9
wd = 0.0005
bn_momentum = 0.75
"""


def _net(bn=True):
    """conv 3x3 -> bn -> relu; a stride-1 and a stride-2 depthwise-separable block (depthwise 3x3 ->
    bn -> relu -> conv 1x1 -> bn -> relu); a depthwise 5x5 and a depthwise 3x3, each with a bias
    and directly followed by relu -- the first gets the fused-relu forward and feeds the second,
    whose data gradient is therefore relu'-masked; max pooling, average pooling, fullc, softmax.
    bn = False leaves the batch norms out (their convs then keep their biases)."""
    out = ["netconfig=start"]
    nb = "  no_bias = 1" if bn else None

    def conv(src, name, ch, k, stride=1, group=1, bias=False):
        out.extend(l for l in ["layer[%s->%s] = conv:%s" % (src, name, name), "  kernel_size = %d" % k,
                               "  pad = %d" % (k // 2), "  stride = %d" % stride, "  nchannel = %d" % ch,
                               "  ngroup = %d" % group, None if bias else nb] if l)
        return name

    def norm_relu(src, tag):
        if bn:
            out.append("layer[%s->%s_n] = batch_norm_ma:%s_bn" % (src, tag, tag))
            src = tag + "_n"
        out.append("layer[%s->%s_r] = relu" % (src, tag))
        return tag + "_r"
    x = norm_relu(conv("0", "c0", 16, 3), "c0")
    x = norm_relu(conv(x, "a_dw", 16, 3, group=16), "a_dw")
    x = norm_relu(conv(x, "a_pw", 32, 1), "a_pw")
    x = norm_relu(conv(x, "b_dw", 32, 3, stride=2, group=32), "b_dw")
    x = norm_relu(conv(x, "b_pw", 32, 1), "b_pw")
    x = conv(x, "d5", 32, 5, group=32, bias=True)
    out.append("layer[d5->d5_r] = relu")
    x = conv("d5_r", "d3", 32, 3, group=32, bias=True)
    out.append("layer[d3->d3_r] = relu")
    out.extend(["layer[d3_r->mp] = max_pooling", "  kernel_size = 2", "  stride = 2",
                "layer[mp->gap] = avg_pooling", "  kernel_size = 3", "  stride = 1",
                "layer[gap->flat] = flatten", "layer[flat->fc] = fullc:fc", "  nhidden = 10",
                "layer[fc->fc] = softmax", "netconfig=end"])
    return "\n".join(out) + "\n" + TAIL


NET, NET_NOBN = _net(True), _net(False)
DW_NAMES = ("a_dw", "b_dw", "d5", "d3")


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


def _convs(tr):
    return [c.layer for c in tr.net.connections if c.type == 10]


def _depthwise(tr):
    return [l for l in _convs(tr) if l.geo.groups > 1]


def test_one_step_matches_the_cpu_executor():
    """One training step from one seed on the GPU (bf16 HIP kernels) and on the CPU executor that
    keeps bf16 at node boundaries (tests/test_bn_ma_net_gpu.py): every parameter tensor and the
    output of a forward pass after the step agree within relerr 2e-2, each on its own scale.
    The four depthwise layers are on the direct kernels, the 5 x 5 one with the fused relu, the
    3 x 3 one behind it with the masked data gradient.
    Measured on an MI355X: the worst tensors are the batch norms' biases, 3.8e-4 (the stride-1
    block's depthwise bn), 2.7e-4 (the first bn), 1.5e-4 and 6e-5 (the next two); the first conv's
    weights 1e-5; everything else -- the depthwise weights and biases, the output, the running
    statistics -- below 5e-6."""
    from cxxnet_amd.ops import gemm
    gpu, ora = _make("gpu"), _make("cpu")
    _bf16_at_node_boundaries(ora)
    for a, b in zip(_params(gpu), _params(ora)):
        assert relerr(a, b) < 1e-5  # the same seed starts both alike
    dw = _depthwise(gpu)
    assert len(dw) == 4 and all(gemm.is_depthwise(l.geo) and gemm.dwconv_served(l.geo) for l in dw)
    assert [(l.geo.KH, l.geo.stride, l.b is not None) for l in dw] == [(3, 1, False), (3, 2, False), (5, 1, True),
                                                                      (3, 1, True)]
    assert dw[2].fuse_relu and dw[3].fuse_relu and dw[3].grad_mask_relu
    assert dw[0].w.shape == (16, 3, 3, 1)
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = [(gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    assert len(keys) == 7 + 2 + 2 * 5 + 2  # seven convs, two of them with a bias, five batch norms, the classifier
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


def test_deterministic_runs_are_bitwise_equal():
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


def test_launch_list_replay_equals_eager_steps():
    """batch_norm_ma is not audited for launch-list replay (its class keeps replay_audited off), so
    the net with batch norms stays eager under launch_replay = 1; the same net without them is
    recorded and replayed, the depthwise launches with it."""
    assert not _make(extra=[("launch_replay", "1")])._list_eligible()
    res = []
    for replay in (0, 1):
        tr = _make(conf=NET_NOBN, extra=[("launch_replay", str(replay))] + DET)
        assert len(_depthwise(tr)) == 4
        for seed in (1, 2, 3):  # eager, record, replay
            tr.update(_batch(seed))
        torch.cuda.synchronize()
        if replay:
            assert tr._lists, "the step was not recorded"
        res.append((_params(tr), _raw(tr, _batch(5))))
    assert all(torch.equal(x, y) for x, y in zip(res[0][0], res[1][0]))
    assert np.array_equal(res[0][1], res[1][1])


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


DW_KERNELS = ("dwconv_fwd", "dwconv_bwd_data", "dwconv_wgrad_partial", "dwconv_wgrad_merge")


def test_forward_backward_launch_only_library_kernels():
    foreign, names = _foreign_kernels(_make(), _batch(1))
    assert not foreign, foreign
    assert all(any(k in n for n in names) for k in DW_KERNELS), sorted(names)


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
    tr.update(part)  # a training step at 5 rows, then at 8 again
    tr.update(full)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()


def test_save_load_keeps_the_depthwise_weights():
    """The model file holds a depthwise weight as the reference's (G, Cout / G, Cg KH KW) =
    (C, 1, K K) tensor; loading it into a trainer with another seed restores the same weights and
    the same outputs."""
    tr = _make()
    tr.update(_batch(1))
    data = tr.save_model()
    probe = _batch(9)
    want = _raw(tr, probe)
    tr2 = _trainer(extra=[("seed", "99")])
    tr2.load_model(data)
    for a, b in zip(_depthwise(tr), _depthwise(tr2)):
        wa, wb = a.w.w.view(a.w.shape), b.w.w.view(b.w.shape)
        assert torch.equal(wa, wb) and wa.abs().sum() > 0
        C, K = a.geo.C, a.geo.KH
        logical = a.to_logical(wa)
        assert tuple(logical.shape) == (C, 1, K * K)
        assert torch.equal(logical.reshape(C, K, K), wa.float().cpu().reshape(C, K, K))
    assert np.array_equal(_raw(tr2, probe), want)


def test_mobilenet_v1_one_step():
    """One training step of models/confs/mobilenet_v1.conf at batch 2: finite softmax rows that
    sum to 1, every parameter tensor changed, library kernels only.  No numeric comparison with the
    CPU executor: 27 batch norms at batch 2 (the last at 7 x 7) amplify storage rounding beyond
    any derived tolerance; the tiny net above carries the numerics."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("mobilenet_v1", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:  # (deterministic: no tile timing)
        tr.set_param(k, v)
    tr.init_model()
    assert tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    assert len(_depthwise(tr)) == 13
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = _params(tr)
    foreign, names = _foreign_kernels(tr, b)
    assert not foreign, foreign
    assert all(any(k in n for n in names) for k in DW_KERNELS), sorted(names)
    after = _params(tr)
    assert all(torch.isfinite(a).all() for a in after)
    unchanged = [i for i, (a, c) in enumerate(zip(before, after)) if torch.equal(a, c)]
    assert not unchanged, unchanged
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)  # (u = 2^-8 of a bf16 row)
