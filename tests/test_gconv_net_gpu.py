"""Narrow-group convolutions in a net on the GPU: a tiny ResNeXt-style net against the CPU executor
(with the same net at ngroup = 1, served by the GEMM kernels, as the noise level), HIP-graph and
launch-list replay, a batch-size change, and one step of ResNeXt-50 32x4d."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr
from test_dwconv_net_gpu import DET, TAIL, _batch, _make, _params, _raw  # (the same input shape and solver settings)

pytestmark = pytest.mark.gpu


def _net(group=4, res=True):
    """16-channel stem; bottleneck a (1x1, grouped 3x3, 1x1, each with bn) + identity; bottleneck b
    without norms (1x1 32 -> relu -> grouped 3x3 stride 2 -> relu -> 1x1) + 1x1 stride-2 projection:
    b_c2 runs the fused-relu forward and its data gradient is relu'-masked.  Pooling, fullc, softmax.
    res = False drops the norms and the shortcuts (a chain whose layer classes all replay from launch lists)."""
    out = ["netconfig=start"]

    def conv(src, name, ch, k, stride=1, grp=1, bias=False):
        out.extend(l for l in ["layer[%s->%s] = conv:%s" % (src, name, name), "  kernel_size = %d" % k,
                               "  pad = %d" % (k // 2), "  stride = %d" % stride, "  nchannel = %d" % ch,
                               "  ngroup = %d" % grp, None if bias or not res else "  no_bias = 1"] if l)
        return name

    def norm(src, tag, relu=True):
        if res:
            out.append("layer[%s->%s_n] = batch_norm_ma:%s_bn" % (src, tag, tag))
            src = tag + "_n"
        if relu:
            out.append("layer[%s->%s_r] = relu" % (src, tag))
            src = tag + "_r"
        return src
    x = norm(conv("0", "c0", 16, 3), "c0")
    if res:
        out.append("layer[%s->a_x,a_id] = split" % x)
        x = "a_x"
    x = norm(conv(x, "a_c1", 16, 1), "a_c1")
    x = norm(conv(x, "a_c2", 16, 3, grp=group), "a_c2")
    x = norm(conv(x, "a_c3", 16, 1), "a_c3", relu=False)
    if res:
        out.extend(["layer[%s,a_id->a] = add:a_add" % x, "  add_relu = 1", "layer[a->b_x,b_id] = split"])
        x = "b_x"
    else:
        out.append("layer[%s->a] = relu" % x)
        x = "a"
    out.append("layer[%s->b_r1] = relu" % conv(x, "b_c1", 32, 1, bias=True))
    out.append("layer[%s->b_r2] = relu" % conv("b_r1", "b_c2", 32, 3, stride=2, grp=group, bias=True))
    x = conv("b_r2", "b_c3", 32, 1, bias=True)
    if res:
        conv("b_id", "b_cp", 32, 1, stride=2, bias=True)
        out.extend(["layer[b_c3,b_cp->b] = add:b_add", "  add_relu = 1"])
    else:
        out.append("layer[b_c3->b] = relu")
    out.extend(["layer[b->mp] = max_pooling", "  kernel_size = 2", "  stride = 2",
                "layer[mp->gap] = avg_pooling", "  kernel_size = 3", "  stride = 1",
                "layer[gap->flat] = flatten", "layer[flat->fc] = fullc:fc", "  nhidden = 10",
                "layer[fc->fc] = softmax", "netconfig=end"])
    return "\n".join(out) + "\n" + TAIL


def _grouped(tr):
    return [c.layer for c in tr.net.connections if c.type == 10 and c.layer.geo.groups > 1]


def _step_errors(conf):
    """relerr of every parameter tensor and of the output after one training step, GPU against the
    CPU executor that keeps bf16 at node boundaries."""
    gpu, ora = _make("gpu", conf=conf), _make("cpu", conf=conf)
    _bf16_at_node_boundaries(ora)
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = ["%s%d.%s" % (gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    errs = {k: relerr(a, b) for k, a, b in zip(keys, _params(gpu), _params(ora))}
    probe = _batch(2)
    errs["output"] = relerr(torch.from_numpy(_raw(gpu, probe)), torch.from_numpy(_raw(ora, probe)))
    return gpu, errs


def test_one_step_matches_the_cpu_executor():
    """The grouped net against the CPU executor, tensor by tensor, within twice the worst relerr of
    the same net at ngroup = 1 (served entirely by the kernels the narrow-group path leaves alone):
    that net's errors are the bf16 noise of this architecture, the factor 2 allows for the other
    reduction order and the smaller fan-in.
    Measured on an MI355X: grouped worst 7.7e-6 (the first bottleneck's bn bias; the stem conv 5e-6,
    everything else below 5e-7); at ngroup = 1 worst 2.8e-3 (b_c2's bias; the output 2.4e-3, the
    batch norms' biases 3e-4 .. 2.2e-3)."""
    from cxxnet_amd.ops import gemm
    gpu, errs = _step_errors(_net(4))
    gc = _grouped(gpu)
    assert [(l.geo.C, l.geo.groups, l.geo.stride) for l in gc] == [(16, 4, 1), (32, 4, 2)]
    assert all(gemm.gconv_served(l.geo) for l in gc)
    assert gc[1].fuse_relu and gc[1].grad_mask_relu and not gc[0].fuse_relu
    _, noise = _step_errors(_net(1))
    worst, level = max(errs.items(), key=lambda kv: kv[1]), max(noise.items(), key=lambda kv: kv[1])
    print("grouped", {k: round(v, 6) for k, v in errs.items()})
    print("ngroup = 1", {k: round(v, 6) for k, v in noise.items()})
    print("worst grouped", worst, "worst at ngroup = 1", level)
    assert worst[1] <= 2 * level[1], (worst, level)


def _three_steps(extra, conf=None):
    tr = _make(conf=conf or _net(), extra=list(extra) + DET)
    for seed in (1, 2, 3):  # eager, capture / record + replay, replay
        tr.update(_batch(seed))
    torch.cuda.synchronize()
    return tr, _params(tr), _raw(tr, _batch(5))


@pytest.mark.parametrize("key,attr,res", [("cuda_graph", "_graphs", True), ("launch_replay", "_lists", False)])
def test_replay_equals_eager_steps(key, attr, res):
    """HIP-graph replay of the residual net; launch-list replay of the chain without add and
    batch_norm_ma (not audited for launch lists), the narrow-group launches recorded with it."""
    conf = _net(4, res=res)
    _, p0, o0 = _three_steps([(key, "0")], conf)
    tr, p1, o1 = _three_steps([(key, "1")], conf)
    assert len(_grouped(tr)) == 2 and getattr(tr, attr), "the step was not captured / recorded"
    assert all(torch.equal(x, y) for x, y in zip(p0, p1)) and np.array_equal(o0, o1)


def test_a_smaller_batch_gives_the_same_rows():
    from cxxnet_amd.io.data import DataBatch
    tr = _make(conf=_net(), extra=DET)
    tr.update(_batch(1))
    full = _batch(4)
    want = _raw(tr, full)[:5]
    part = DataBatch(full.data[:5].clone(), full.label[:5].clone())
    assert np.array_equal(_raw(tr, part), want) and tr.net.cur_batch == 5
    tr.update(part)  # a training step at 5 rows, then at 8 again
    tr.update(full)
    torch.cuda.synchronize()
    assert torch.isfinite(tr.net.arena.w).all()


def _foreign_kernels(tr, b):
    """tests/test_launch_hygiene_gpu.py's check: (at::native kernel names, all kernel names) of one step."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(2):  # lazy buffers happen in the first steps
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


def test_resnext50_one_step():
    """One deterministic training step of models/confs/resnext50_32x4d.conf at batch 2: finite
    softmax rows that sum to 1, every grouped layer's weights changed, library kernels only."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("resnext50_32x4d", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:  # (deterministic: no tile timing)
        tr.set_param(k, v)
    tr.init_model()
    gc = _grouped(tr)
    assert len(gc) == 16 and tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = [l.w.w.detach().cpu().clone() for l in gc]
    foreign, names = _foreign_kernels(tr, b)
    assert not foreign, foreign
    assert all(any(k in n for n in names) for k in ("gconv_mm", "gconv_wgrad_partial", "gconv_wgrad_merge")), sorted(names)
    after = [l.w.w.detach().cpu() for l in gc]
    assert all(torch.isfinite(a).all() and not torch.equal(a, c) for a, c in zip(after, before))
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)  # (u = 2^-8 of a bf16 row)
