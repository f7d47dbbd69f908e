"""Large-kernel depthwise conv, layer_norm and gelu in a net on the GPU: a tiny ConvNeXt-style net
against the CPU executor (with the same net at 5 x 5 depthwise kernels, which dwconv_kernels.hip
serves, as the noise level), HIP-graph replay, and one step of convnext_tiny.conf."""
import numpy as np
import pytest
import torch

from test_bn_ma_net_gpu import _bf16_at_node_boundaries, relerr
from test_dwconv_net_gpu import DET, _params, _raw

pytestmark = pytest.mark.gpu
BATCH = 4


def _net(k=7):
    """8 x 16 x 16 input; 4x4 / 4 stem to 8 channels + layer_norm; a block at width 8 on 4 x 4; layer_norm
    + 2x2 / 2 conv to 16; a block at width 16 on 2 x 2; pooling, layer_norm, fullc, softmax.  A block:
    split -> depthwise k x k -> layer_norm -> 1x1 to 4C -> gelu -> 1x1 to C -> drop_path (0) -> add."""
    out = ["netconfig=start", "layer[0->stem] = conv:stem", "  kernel_size = 4", "  stride = 4", "  nchannel = 8",
           "layer[stem->s1] = layer_norm:stem_ln"]
    cur = "s1"
    for t, C in (("a", 8), ("b", 16)):
        if t == "b":
            out += ["layer[%s->ds_n] = layer_norm:ds_ln" % cur, "layer[ds_n->s2] = conv:ds", "  kernel_size = 2",
                    "  stride = 2", "  nchannel = 16"]
            cur = "s2"
        out += ["layer[%s->%s_x,%s_id] = split" % (cur, t, t),
                "layer[%s_x->%s_d] = conv:%s_dw" % (t, t, t), "  kernel_size = %d" % k, "  pad = %d" % (k // 2),
                "  nchannel = %d" % C, "  ngroup = %d" % C,
                "layer[%s_d->%s_n] = layer_norm:%s_ln" % (t, t, t),
                "layer[%s_n->%s_e] = conv:%s_pw1" % (t, t, t), "  kernel_size = 1", "  nchannel = %d" % (4 * C),
                "layer[%s_e->%s_g] = gelu" % (t, t),
                "layer[%s_g->%s_p] = conv:%s_pw2" % (t, t, t), "  kernel_size = 1", "  nchannel = %d" % C,
                "layer[%s_p->%s_p] = drop_path" % (t, t), "  drop_prob = 0",
                "layer[%s_p,%s_id->%s] = add:%s_add" % (t, t, t, t)]
        cur = t
    out += ["layer[b->gap] = avg_pooling", "  kernel_size = 2", "  stride = 1", "layer[gap->gap_n] = layer_norm:head_ln",
            "layer[gap_n->flat] = flatten", "layer[flat->fc] = fullc:fc", "  nhidden = 10", "layer[fc->fc] = softmax",
            "netconfig=end", "input_shape = 8,16,16", "random_type = xavier", "eta = 0.05", "momentum = 0.9", "wd = 0.0005"]
    return "\n".join(out) + "\n"


def _make(dev="gpu", conf=None, extra=()):
    from cxxnet_amd import native
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf or _net())) + [
            ("batch_size", str(BATCH)), ("dev", dev), ("eval_train", "0"), ("silent", "1"), ("seed", "3"),
            ("cuda_graph", "0"), ("launch_replay", "0")] + list(extra):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def _batch(seed):
    from cxxnet_amd.io.data import DataBatch
    g = torch.Generator().manual_seed(seed)
    return DataBatch(torch.randn(BATCH, 8, 16, 16, generator=g), torch.randint(0, 10, (BATCH, 1), generator=g).float())


def _depthwise(tr):
    return [c.layer for c in tr.net.connections if c.type == 10 and c.layer.geo.groups > 1]


def _step_errors(conf):
    """relerr of every parameter tensor and of the output after one training step, GPU against the
    CPU executor that keeps bf16 at node boundaries.  Intermediate nodes and raw gradients are not
    compared one by one, as in the project's other tiny-net tests: every layer's gradient enters its
    parameters through the momentum step, and every node feeds the probe batch's output."""
    gpu, ora = _make("gpu", conf), _make("cpu", conf)
    _bf16_at_node_boundaries(ora)
    gpu.update(_batch(1))
    ora.update(_batch(1))
    keys = ["%s%d.%s" % (gpu.net.connections[li].layer.type_name, li, s.tag) for li, s in gpu.net.arena.specs]
    errs = {k: relerr(a, b) for k, a, b in zip(keys, _params(gpu), _params(ora))}
    probe = _batch(2)
    errs["output"] = relerr(torch.from_numpy(_raw(gpu, probe)), torch.from_numpy(_raw(ora, probe)))
    return gpu, errs


def test_one_step_matches_the_cpu_executor():
    """The 7 x 7 net against the CPU executor, tensor by tensor, within twice the worst relerr of the
    same net with 5 x 5 pad-2 depthwise layers (served by dwconv_kernels.hip): that net's errors
    are the bf16 noise of this architecture.
    Measured on an MI355X: 7 x 7 worst 1.24e-7 (the output; the stem's weights 9.2e-8, a_dw's 1.1e-7);
    5 x 5 worst 9.44e-8 (the stem's weights; the output 6.8e-8).  Both are fp32 noise of the master
    weights: the two executors round the same bf16 values at every node."""
    from cxxnet_amd.ops import gemm
    gpu, errs = _step_errors(_net(7))
    dw = _depthwise(gpu)
    assert [(l.geo.C, l.geo.KH, l.geo.H) for l in dw] == [(8, 7, 4), (16, 7, 2)]
    assert all(gemm.dwlk_served(l.geo) and not gemm.dwconv_served(l.geo) for l in dw)
    _, noise = _step_errors(_net(5))
    worst, level = max(errs.items(), key=lambda kv: kv[1]), max(noise.items(), key=lambda kv: kv[1])
    print("7x7", {k: float("%.3g" % v) for k, v in errs.items()})
    print("5x5", {k: float("%.3g" % v) for k, v in noise.items()})
    print("worst 7x7", worst, "worst 5x5", level)
    assert worst[1] <= 2 * level[1], (worst, level)


def _three_steps(extra):
    tr = _make(extra=list(extra) + DET)
    for seed in (1, 2, 3):  # eager, capture + replay, replay
        tr.update(_batch(seed))
    torch.cuda.synchronize()
    return tr, _params(tr), _raw(tr, _batch(5))


def test_graph_replay_equals_eager_steps():
    _, p0, o0 = _three_steps([("cuda_graph", "0")])
    tr, p1, o1 = _three_steps([("cuda_graph", "1")])
    assert tr._graphs, "the step was not captured"
    assert all(torch.equal(x, y) for x, y in zip(p0, p1)) and np.array_equal(o0, o1)


def test_convnext_tiny_one_step():
    """One training step of models/confs/convnext_tiny.conf at batch 2 on synthetic data: every
    parameter finite, every depthwise layer's weights changed, softmax rows that sum to 1."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("convnext_tiny", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "2"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:
        tr.set_param(k, v)
    tr.init_model()
    dw = _depthwise(tr)
    assert len(dw) == 18 and tr.net.nodes[-1].shape == (2, 1, 1, 1000)
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = [l.w.w.detach().cpu().clone() for l in dw]
    tr.update(b)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.net.arena.w).all())
    assert all(not torch.equal(l.w.w.detach().cpu(), c) for l, c in zip(dw, before))
    out = _raw(tr, b).reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)  # (u = 2^-8 of a bf16 row)
