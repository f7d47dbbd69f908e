"""softmax_rows_reg<4 | 8 | 16>, softmax_rows and loss_grad element by element against the float64
references and derived bounds of tests/bounds.py, through cxxnet_amd.ops only.

max-error over max-value (the earlier assertion) is blind below the row's largest probability: a
tail element left out of the sum, or a probability of 1e-4 that is wrong by half, pass it
(tests/test_norm_bounds_cpu.py).  Here every probability is held to its own relative bound -- the
fp32 copy that feeds the loss gradient and the metrics to ~(K + |x - max|) 2^-23, the bf16 copy
to its rounding -- and every row to summing to 1.  K covers each register width on both sides of
its edge (256 | 257, 512 | 513, 1024 | 1025) and the strided kernel; rows = 5 leaves a partial
block there; the recipes put the row maximum at the first index, the last one and in the middle
of a lane's slice, 80 above the rest (exp(-80) is still a normal number), and rows near -80."""
import pytest
import torch

import bounds
import norm_cases as nc
from cxxnet_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("K", nc.SOFTMAX_K)
def test_softmax_and_loss_grad_within_bound(K, rows):
    worst = [0.0, 0.0, 0.0]
    for recipe in nc.SOFTMAX_RECIPES:
        x = nc.softmax_input(recipe, rows, K)
        what = "K %d rows %d %s" % (K, rows, recipe)
        ref, b32, b16 = bounds.softmax_ref(x)
        p = torch.full((rows, K), NAN, device=DEV, dtype=torch.bfloat16)
        p32 = torch.full((rows, K), NAN, device=DEV)
        ops.softmax_forward(x.to(DEV), p, p32)
        assert torch.isfinite(p32).all() and torch.isfinite(p.float()).all(), what
        worst[0] = max(worst[0], bounds.assert_within(p32, ref, b32, "softmax fp32 " + what, axes="rk"))
        worst[1] = max(worst[1], bounds.assert_within(p, ref, b16, "softmax bf16 " + what, axes="rk"))
        off = (p32.cpu().double().sum(1) - 1).abs()
        assert (off <= bounds.softmax_sum_bound(x)).all(), (what, off.tolist(), bounds.softmax_sum_bound(x).tolist())
        lab = nc.softmax_labels(rows, K)
        for scale in (0.5, 1.0 / 256):
            g = p.clone()
            ops.loss_grad("softmax", g, lab.to(DEV), scale, p32)
            worst[2] = max(worst[2], bounds.assert_within(g, *bounds.loss_grad_ref(p32, lab, scale),
                                                          "loss gradient scale %g " % scale + what, axes="rk"))
    print("d/bound softmax fp32 %.3f bf16 %.3f loss_grad %.3f  K %d rows %d" % (*worst, K, rows))


@pytest.mark.parametrize("kind", ["l2", "multi_logistic"])
def test_loss_grad_kinds_with_wide_labels(kind):
    """the kinds that read a label per element (label width K) and the prediction from the node"""
    rows, K = 5, 65
    pred = torch.sigmoid(nc.bf16_randn((rows, K), 90).float()).to(torch.bfloat16)
    lab = (torch.rand(rows, K, generator=torch.Generator().manual_seed(91)) > 0.5).float()
    g = pred.to(DEV)
    ops.loss_grad(kind, g, lab.to(DEV), 0.5)
    w = bounds.assert_within(g, *bounds.loss_grad_ref(pred, lab, 0.5, kind=kind), kind, axes="rk")
    print("d/bound loss_grad %s %.3f" % (kind, w))
