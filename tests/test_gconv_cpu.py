"""Narrow-group convolution without a GPU: the dispatch predicates of ops/gemm.py as pure functions
of the geometry, the Python mirror of the weight-gradient launcher's slab formula, and
models/confs/resnext50_32x4d.conf on the CPU executor."""
import numpy as np
import pytest
import torch

from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

# (blocks, grouped width, output channels, input resolution of the stage's first 3 x 3) per stage
STAGES = [(3, 128, 256, 56), (4, 256, 512, 56), (6, 512, 1024, 28), (3, 1024, 2048, 14)]


def _g(C, Cout, K, stride, pad, groups, N=2, H=9, W=9):
    Ho, Wo = gemm.conv_out_size(H, W, K, K, stride, pad, pad)
    return ConvGeom(N, H, W, C, Ho, Wo, Cout, K, K, stride, pad, pad, groups)


@pytest.mark.parametrize("C,groups", [(16, 4), (48, 12), (48, 6), (64, 4), (64, 16), (128, 32), (512, 32)])
@pytest.mark.parametrize("stride", [1, 2])
def test_served_geometries(C, groups, stride):
    g = _g(C, C, 3, stride, 1, groups)
    assert gemm.is_narrow_group(g) and gemm.gconv_served(g) and not gemm.is_depthwise(g)


@pytest.mark.parametrize("name,g", [
    ("AlexNet conv2 (ngroup = 2)", ConvGeom(256, 27, 27, 96, 27, 27, 256, 5, 5, 1, 2, 2, 2)),
    ("AlexNet conv4 (ngroup = 2)", ConvGeom(256, 13, 13, 384, 13, 13, 384, 3, 3, 1, 1, 1, 2)),
    ("AlexNet conv5 (ngroup = 2)", ConvGeom(256, 13, 13, 384, 13, 13, 256, 3, 3, 1, 1, 1, 2)),
    ("launch-hygiene c2b (ngroup = 2)", _g(16, 16, 3, 1, 1, 2)),
    ("depthwise", _g(32, 32, 3, 1, 1, 32)),
    ("plain 3 x 3", _g(32, 32, 3, 1, 1, 1)),
    ("pad 0", _g(32, 32, 3, 1, 0, 4)),
    ("5 x 5", _g(32, 32, 5, 1, 2, 4)),
    ("1 x 1", _g(32, 32, 1, 1, 0, 4)),
    ("stride 3", _g(32, 32, 3, 3, 1, 4)),
    ("C != Cout", _g(32, 64, 3, 1, 1, 4)),
    ("12 channels per group", _g(48, 48, 3, 1, 1, 4)),
    ("2 channels per group", _g(32, 32, 3, 1, 1, 16)),
    ("64 channels per group", _g(256, 256, 3, 1, 1, 4)),
    ("32 channels per group (kept on the GEMM route: slower there)", _g(1024, 1024, 3, 1, 1, 32)),
    ("five groups of 4: C % 16", _g(20, 20, 3, 1, 1, 5)),
])
def test_declined_geometries(name, g):
    assert not gemm.gconv_served(g), name


# (N, C, cg, Ho, Wo, stride) -> (P, workspace floats), worked by hand: patches of R x 16 output pixels
# (R = 8 / 4 at stride 1 / 2), ny = C / 64, C / 32 or C / 16 slices, ipb = ceil(items / (512 // ny))
WGRAD_TABLE = [
    ((3, 48, 4, 19, 20, 1), (18, 18 * 48 * 9 * 4)),            # 3 x 3 x 2 patches, ny 3 -> 170 slabs at most: ipb 1
    ((1, 16, 4, 1, 1, 1), (1, 16 * 9 * 4)),
    ((64, 128, 4, 56, 56, 1), (256, 256 * 128 * 9 * 4)),       # 64 x 7 x 4 = 1792 patches, ny 2: ipb 7
    ((64, 256, 8, 28, 28, 2), (128, 128 * 256 * 9 * 8)),       # 64 x 7 x 2 = 896, ny 4: ipb 7
    ((64, 1024, 32, 7, 7, 1), (32, 32 * 1024 * 9 * 32)),       # 64 patches, ny 16 -> 32 slabs: ipb 2
    ((2, 160, 32, 5, 3, 2), (4, 4 * 160 * 9 * 32)),            # 2 x 2 x 1 patches, ny 5
]


@pytest.mark.parametrize("shape,want", WGRAD_TABLE)
def test_wgrad_partial_formula(shape, want):
    N, C, cg, Ho, Wo, S = shape
    H, W = (Ho - 1) * S + 1, (Wo - 1) * S + 1
    assert gemm.gconv_wgrad_partials(ConvGeom(N, H, W, C, Ho, Wo, C, 3, 3, S, 1, 1, C // cg)) == want


@pytest.fixture(scope="module")
def resnext():
    from cxxnet_amd.models import load_conf
    from cxxnet_amd.nnet import NetTrainer
    tr = NetTrainer()
    for k, v in load_conf("resnext50_32x4d", [("batch_size", "2"), ("dev", "cpu"), ("eval_train", "0"),
                                              ("silent", "1"), ("seed", "1")]):
        tr.set_param(k, v)
    tr.init_model()
    return tr


def test_resnext50_conf_builds(resnext):
    net = resnext.net
    assert net.nodes[-1].shape == (2, 1, 1, 1000)
    convs = [c.layer for c in net.connections if c.type == 10]
    assert len(convs) == 1 + 3 * 16 + 4 and all(l.lp.no_bias == 1 for l in convs)
    grouped = [l for l in convs if l.geo.groups > 1]
    want, nparam, cin = [], 3 * 49 * 64 + 2 * 64, 64
    for i, (blocks, width, cout, res) in enumerate(STAGES):
        for b in range(blocks):
            stride = 2 if (b == 0 and i > 0) else 1
            want.append((32, width, width, width // 32, res, stride))
            res //= stride
            nparam += cin * width + 9 * width * (width // 32) + width * cout + 2 * (2 * width + cout)
            if b == 0:
                nparam += cin * cout + 2 * cout
            cin = cout
    nparam += 2048 * 1000 + 1000
    assert [(l.geo.groups, l.geo.C, l.geo.Cout, l.geo.C // l.geo.groups, l.geo.H, l.geo.stride) for l in grouped] == want
    assert [sum(1 for w in want if w[3] == cg) for cg in (4, 8, 16, 32)] == [3, 4, 6, 3]
    for l in grouped:
        g = l.geo
        assert (g.KH, g.KW, g.pad_y, g.pad_x) == (3, 3, 1, 1)
        g64 = ConvGeom(64, g.H, g.W, g.C, g.Ho, g.Wo, g.Cout, 3, 3, g.stride, 1, 1, g.groups)
        assert gemm.is_narrow_group(g64) and gemm.gconv_served(g64) == (g.C // g.groups != 32)  # (32: the GEMM route)
    assert nparam == 25028904  # (Xie et al.'s 25.0 M)
    assert sum(s.numel for _, s in net.arena.specs) == nparam


def test_resnext50_one_training_step(resnext):
    from cxxnet_amd.io.data import DataBatch
    tr = resnext
    g = torch.Generator().manual_seed(1)
    b = DataBatch(torch.randn(2, 3, 224, 224, generator=g), torch.randint(0, 1000, (2, 1), generator=g).float())
    before = tr.net.arena.w.clone()
    tr.update(b)
    after = tr.net.arena.w
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    out = tr.forward_to([len(tr.net.nodes) - 1], b)[0].reshape(2, -1)
    assert out.shape == (2, 1000) and np.isfinite(out).all() and np.allclose(out.sum(1), 1.0, atol=1e-5)
