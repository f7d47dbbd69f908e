"""Depthwise convolution without a GPU: models/confs/mobilenet_v1.conf on the CPU executor, the
dispatch predicates of ops/gemm.py as pure functions of the geometry, and the Python mirror of the
weight-gradient launcher's partial-count / workspace formula."""
import numpy as np
import pytest
import torch

from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

# (output channels of the pointwise conv, stride of the depthwise conv) of the 13 blocks
BLOCKS = [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1),
          (512, 1), (1024, 2), (1024, 1)]


@pytest.fixture(scope="module")
def mobilenet():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("mobilenet_v1", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1"),
                                           ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def test_mobilenet_v1_conf_builds(mobilenet):
    net = mobilenet.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    convs = [c for c in net.connections if c.type == 10]
    assert len(convs) == 27 and all(c.layer.lp.no_bias == 1 for c in convs)
    assert sum(1 for c in net.connections if c.type == 40) == 27  # a batch_norm_ma behind every conv
    assert convs[0].nodes_out[0].shape[1:] == (32, 112, 112)
    # the layer list: what every block's two convs must look like, and the parameter count
    nparam = 3 * 9 * 32 + 2 * 32
    cin, res = 32, 112
    for i, (cout, stride) in enumerate(BLOCKS):
        dw, pw = convs[1 + 2 * i], convs[2 + 2 * i]
        res //= stride
        g = dw.layer.geo
        assert (g.groups, g.C, g.Cout, g.KH, g.KW, g.stride, g.pad_y, g.pad_x) == (cin, cin, cin, 3, 3, stride, 1, 1)
        assert gemm.is_depthwise(g) and gemm.dwconv_served(g)
        assert dw.nodes_out[0].shape[1:] == (cin, res, res)
        assert dw.layer.w.shape == (cin, 3, 3, 1)
        p = pw.layer.geo
        assert (p.groups, p.KH, p.stride, p.C) == (1, 1, 1, cin) and not gemm.is_depthwise(p)
        assert pw.nodes_out[0].shape[1:] == (cout, res, res)
        nparam += 9 * cin + 2 * cin + cin * cout + 2 * cout
        cin = cout
    assert (cin, res) == (1024, 7)
    nparam += 1024 * 1000 + 1000
    assert nparam == 4231976
    assert sum(s.numel for _, s in net.arena.specs) == nparam


def test_mobilenet_v1_one_training_step(mobilenet):
    from cxxnet_amd.io.data import DataBatch
    tr = mobilenet
    g = torch.Generator().manual_seed(1)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = tr.net.arena.w.clone()
    tr.update(b)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = tr.forward_to([len(tr.net.nodes) - 1], b)[0].reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)


def _g(C, Cout, K, stride, pad_y, pad_x, groups, N=2, H=9, W=9):
    Ho, Wo = gemm.conv_out_size(H, W, K, K, stride, pad_y, pad_x)
    return ConvGeom(N, H, W, C, Ho, Wo, Cout, K, K, stride, pad_y, pad_x, groups)


@pytest.mark.parametrize("C", [8, 24, 136, 1024])
@pytest.mark.parametrize("K,stride,pad_y,pad_x", [(3, 1, 1, 1), (3, 2, 1, 1), (3, 2, 0, 0), (3, 1, 1, 0), (5, 1, 2, 2),
                                                  (5, 2, 2, 2), (5, 2, 4, 0), (3, 1, 2, 2)])
def test_served_geometries(C, K, stride, pad_y, pad_x):
    g = _g(C, C, K, stride, pad_y, pad_x, C)
    assert gemm.is_depthwise(g) and gemm.dwconv_served(g)


@pytest.mark.parametrize("name,g", [
    ("channel multiplier 2", _g(8, 16, 3, 1, 1, 1, 8)),
    ("C = 12", _g(12, 12, 3, 1, 1, 1, 12)),
    ("7 x 7", _g(8, 8, 7, 1, 3, 3, 8)),
    ("stride 3", _g(8, 8, 3, 3, 1, 1, 8)),
    ("pad = K", _g(8, 8, 3, 1, 3, 1, 8)),
    ("map + pads smaller than the kernel", _g(8, 8, 5, 1, 1, 1, 8, H=2, W=2)),
])
def test_unserved_depthwise_geometries(name, g):
    """Depthwise (they never reach a GEMM), but declined: the ops layer raises for them."""
    assert gemm.is_depthwise(g) and not gemm.dwconv_served(g), name


def test_unserved_geometry_raises_before_any_launch():
    # (on CPU tensors the torch branch runs; the depthwise check itself needs no device)
    g = _g(12, 12, 3, 1, 1, 1, 12)
    x = torch.zeros(2, 9, 9, 12, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"C % 8 == 0"):
        gemm.dwconv_forward(x, torch.zeros(12, 3, 3, 1, dtype=torch.bfloat16), None, torch.zeros_like(x), g)


@pytest.mark.parametrize("name,g", [
    ("AlexNet conv2 (ngroup = 2)", ConvGeom(256, 27, 27, 96, 27, 27, 256, 5, 5, 1, 2, 2, 2)),
    ("AlexNet conv4 (ngroup = 2)", ConvGeom(256, 13, 13, 384, 13, 13, 384, 3, 3, 1, 1, 1, 2)),
    ("AlexNet conv5 (ngroup = 2)", ConvGeom(256, 13, 13, 384, 13, 13, 256, 3, 3, 1, 1, 1, 2)),
    ("plain 3 x 3", _g(32, 32, 3, 1, 1, 1, 1)),
    ("one channel, one group", _g(1, 1, 3, 1, 1, 1, 1)),
    ("grouped, 8 channels per group", _g(64, 64, 3, 1, 1, 1, 8)),
    ("two channels per group", _g(16, 16, 3, 1, 1, 1, 8)),
])
def test_other_geometries_are_not_depthwise(name, g):
    assert not gemm.is_depthwise(g) and not gemm.dwconv_served(g), name


def test_alexnet_conf_has_no_depthwise_layer():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("alexnet", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"), ("silent", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    geos = [c.layer.geo for c in tr.net.connections if c.type == 10]
    assert sorted(g.groups for g in geos) == [1, 1, 2, 2, 2]
    assert not any(gemm.is_depthwise(g) for g in geos)


# (N, C, Ho, Wo, K) -> (P, workspace floats), worked by hand from the launcher's rule: G = C / 8
# vectors, GX = min(G, 256), RL = 256 // GX item lanes, ny = ceil(G / GX), items R = N Ho ceil(Wo / 2),
# ipb = max(ceil(R / (512 // ny)), 4 RL), P = ceil(R / ipb), floats = P C (K K + 1)
WGRAD_TABLE = [
    ((3, 24, 5, 7, 3), (1, 1 * 24 * 10)),             # RL 85, R 60, ipb 340
    ((3, 136, 19, 20, 3), (10, 10 * 136 * 10)),       # RL 15, R 570, ipb 60: nine of 60, one of 30
    ((3, 136, 19, 20, 5), (10, 10 * 136 * 26)),       # the same items at 5 x 5
    ((64, 32, 112, 112, 3), (512, 512 * 32 * 10)),    # RL 64, R 401408, ipb max(784, 256) = 784
    ((64, 1024, 7, 7, 3), (224, 224 * 1024 * 10)),    # RL 2, R 1792, ipb max(4, 8) = 8
    ((2, 4096, 7, 7, 3), (14, 14 * 4096 * 10)),       # G 512: GX 256, ny 2, RL 1; R 56, ipb max(1, 4) = 4
    ((1, 8, 1, 1, 5), (1, 1 * 8 * 26)),
]


@pytest.mark.parametrize("shape,want", WGRAD_TABLE)
def test_wgrad_partial_formula(shape, want):
    N, C, Ho, Wo, K = shape
    g = ConvGeom(N, Ho, Wo, C, Ho, Wo, C, K, K, 1, K // 2, K // 2, C)
    assert gemm.dwconv_wgrad_partials(g) == want


def test_depthwise_layer_rejects_a_channel_padded_input():
    """A depthwise conv whose input node carries more physical channels than logical ones (the
    GPU's channel-padded network input) cannot regroup them: init_connection says so."""
    from cxxnet_amd.layers.base import LayerContext, Node
    from cxxnet_amd.layers.std import ConvolutionLayer

    def layer():
        lay = ConvolutionLayer(LayerContext(torch.device("cpu")))
        for k, v in (("kernel_size", "3"), ("pad", "1"), ("nchannel", "3"), ("ngroup", "3")):
            lay.set_param(k, v)
        return lay
    x, y = Node("in"), Node("out")
    x.set_shape(2, 3, 8, 8, cp=4)
    with pytest.raises(ValueError, match="depthwise conv"):
        layer().init_connection([x], [y])
    x.set_shape(2, 3, 8, 8)
    layer().init_connection([x], [y])
    assert y.shape == (2, 3, 8, 8)
