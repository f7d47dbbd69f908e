"""neighborhood_attention in a net on the GPU: a tiny NAT-style net against the CPU executor (with the
same net holding a 1x1 conv from 3C to C in place of each attention as the noise level), HIP-graph
replay, and one step of nat_mini.conf.  Method and helpers: test_attn_net_gpu.py, test_wattn_net_gpu.py."""
import numpy as np
import pytest
import torch

from test_attn_net_gpu import _errors, _worst
from test_bn_ma_net_gpu import _bf16_at_node_boundaries
from test_convnext_net_gpu import _batch, _make
from test_dwconv_net_gpu import DET, _params, _raw

pytestmark = pytest.mark.gpu


def _net(attention=True):
    """8 x 16 x 16 input; 2x2 / 2 stem to 64 channels on 8 x 8; two NAT blocks at nhead = 2 (d = 32),
    kernel 7 then 3, the bias tables drawn at sigma 0.5; layer_norm + 2x2 / 2 merge to 128 channels on
    4 x 4; layer_norm, pooling, fullc, softmax.  attention False: a 1x1 conv 192 -> 64 in
    place of each neighborhood_attention."""
    out = ["netconfig=start", "layer[0->tok] = conv:stem", "  kernel_size = 2", "  stride = 2", "  nchannel = 64"]
    cur = "tok"
    for t, k in (("a", 7), ("b", 3)):
        mix = (["layer[%s_qkv->%s_att] = neighborhood_attention:%s_nattn" % (t, t, t), "  nhead = 2",
                "  kernel = %d" % k, "  init_sigma = 0.5"] if attention else
               ["layer[%s_qkv->%s_att] = conv:%s_mix" % (t, t, t), "  kernel_size = 1", "  nchannel = 64"])
        out += ["layer[%s->%s_ax,%s_aid] = split" % (cur, t, t), "layer[%s_ax->%s_an] = layer_norm:%s_ln1" % (t, t, t),
                "layer[%s_an->%s_qkv] = conv:%s_qkv" % (t, t, t), "  kernel_size = 1", "  nchannel = 192"] + mix + [
                "layer[%s_att->%s_ap] = conv:%s_proj" % (t, t, t), "  kernel_size = 1", "  nchannel = 64",
                "layer[%s_ap->%s_ap] = drop_path" % (t, t), "  drop_prob = 0",
                "layer[%s_ap,%s_aid->%s_a] = add:%s_add1" % (t, t, t, t),
                "layer[%s_a->%s_mx,%s_mid] = split" % (t, t, t), "layer[%s_mx->%s_mn] = layer_norm:%s_ln2" % (t, t, t),
                "layer[%s_mn->%s_me] = conv:%s_fc1" % (t, t, t), "  kernel_size = 1", "  nchannel = 192",
                "layer[%s_me->%s_mg] = gelu" % (t, t),
                "layer[%s_mg->%s_mp] = conv:%s_fc2" % (t, t, t), "  kernel_size = 1", "  nchannel = 64",
                "layer[%s_mp->%s_mp] = drop_path" % (t, t), "  drop_prob = 0",
                "layer[%s_mp,%s_mid->%s] = add:%s_add2" % (t, t, t, t)]
        cur = t
    out += ["layer[b->ds_n] = layer_norm:ds_ln", "layer[ds_n->ds] = conv:ds", "  kernel_size = 2", "  stride = 2",
            "  nchannel = 128", "layer[ds->head_n] = layer_norm:head_ln", "layer[head_n->gap] = avg_pooling",
            "  kernel_size = 4", "  stride = 1", "layer[gap->flat] = flatten", "layer[flat->fc] = fullc:fc",
            "  nhidden = 10", "layer[fc->fc] = softmax", "netconfig=end", "input_shape = 8,16,16",
            "random_type = xavier", "eta = 0.05", "momentum = 0.9", "wd = 0.0005"]
    return "\n".join(out) + "\n"


def _one_step(conf, dev, bf16_products=False):
    """test_attn_net_gpu._one_step with the measuring switch on the neighborhood_attention layers"""
    tr = _make(dev, conf)
    if dev == "cpu":
        _bf16_at_node_boundaries(tr)
        for c in tr.net.connections:
            if c.type == 54:
                c.layer.bf16_products = bf16_products
    tr.update(_batch(1))
    return tr, list(_params(tr)) + [torch.from_numpy(_raw(tr, _batch(2)))]


def test_one_step_matches_the_cpu_executor():
    """As test_attn_net_gpu: the net is held to twice the control net's worst relerr plus what the
    bf16 roundings of P and dS alone add on the CPU executor (NeighborhoodAttentionLayer.bf16_products).
    Measured on an MI355X: neighborhood_attention worst 4.79e-3 (a_ln2's bias; output 1.5e-3), control
    worst 2.86e-3 (the output), the roundings alone 4.34e-3 (the stem's bias): the limit is 1.01e-2."""
    gpu, got = _one_step(_net(True), "gpu")
    att = [c.layer for c in gpu.net.connections if c.type == 54]
    assert len(att) == 2 and all(float(l.params[0].w.abs().max()) > 0.5 for l in att)
    _, want = _one_step(_net(True), "cpu")
    _, rounded = _one_step(_net(True), "cpu", bf16_products=True)
    cg, cgot = _one_step(_net(False), "gpu")
    _, cwant = _one_step(_net(False), "cpu")
    errs, noise, share = _errors(gpu, got, want), _errors(cg, cgot, cwant), _errors(gpu, rounded, want)
    for name, e in (("neighborhood_attention", errs), ("control", noise), ("roundings", share)):
        print(name, {k: float("%.3g" % v) for k, v in e.items()})
    worst, level, extra = _worst(errs), _worst(noise), _worst(share)
    print("worst neighborhood_attention", worst, "worst control", level, "worst roundings alone", extra)
    assert worst[1] <= 2 * level[1] + extra[1], (worst, level, extra)


def _three_steps(extra):
    tr = _make(conf=_net(), extra=list(extra) + DET)
    for seed in (1, 2, 3):  # eager, capture + replay, replay
        tr.update(_batch(seed))
    torch.cuda.synchronize()
    return tr, _params(tr), _raw(tr, _batch(5))


def test_graph_replay_equals_eager_steps():
    _, p0, o0 = _three_steps([("cuda_graph", "0")])
    tr, p1, o1 = _three_steps([("cuda_graph", "1")])
    assert tr._graphs, "the step was not captured"
    assert all(torch.equal(x, y) for x, y in zip(p0, p1)) and np.array_equal(o0, o1)


def test_nat_mini_one_step():
    """One training step of models/confs/nat_mini.conf at batch 4 on synthetic data: a finite loss
    (softmax rows that sum to 1), every parameter finite and moved."""
    from cxxnet_amd.io.data import DataBatch
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    base = [(k, v) for k, v in load_conf("nat_mini", []) if not k.startswith("metric")]
    for k, v in base + [("batch_size", "4"), ("dev", "gpu"), ("eval_train", "0"), ("silent", "1"), ("seed", "1"),
                        ("cuda_graph", "0"), ("launch_replay", "0")] + DET:
        tr.set_param(k, v)
    tr.init_model()
    assert sum(c.type == 54 for c in tr.net.connections) == 18 and tr.net.nodes[-1].shape == (4, 1, 1, 1000)
    g = torch.Generator().manual_seed(0)
    b = DataBatch(torch.randn(4, 3, 224, 224, generator=g), torch.randint(0, 1000, (4, 1), generator=g).float())
    specs = [s for _, s in tr.net.arena.specs]
    before = [s.w.detach().cpu().clone() for s in specs]
    tr.update(b)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.net.arena.w).all())
    assert all(not torch.equal(s.w.detach().cpu(), c) for s, c in zip(specs, before))
    out = _raw(tr, b).reshape(4, -1)
    assert out.shape == (4, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=2.0 ** -8)
