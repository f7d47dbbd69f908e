"""The 13 x 13 direct weight gradient's wide form (csrc/kernels/conv_wgrad_direct.hip: 64 co x 64 ci
block tiles, 2 ci halves x 2 K halves of waves, one image per stage, balanced split ranges)
against fp32 torch, at the points where that layout can go wrong: a single block whose two K
halves share one image, more splits than divide the stages evenly, 3 and 4 ci blocks (the bias
K-steps spread over them), two co blocks, odd image counts, and channel counts that only the
64 x 32 form serves.  Every case also runs on a dy channel slice, accumulates into non-zero dW / db,
and must be bitwise reproducible and give the same dW with and without db.
Reference and bounds as tests/test_conv_wgrad_direct_gpu.py: torch.nn.grad.conv2d_weight in fp32
on the bf16 inputs, dy.sum for the bias, relative error under 1e-5 (fp32 accumulation of exact
bf16 products: only the summation order differs)."""
import pytest
import torch

from cxxnet_amd.ops import gemm
from cxxnet_amd.ops.gemm import ConvGeom

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 13

# (N, C, Cout, groups, splits)
CASES = [
    (1, 64, 64, 1, 1),     # one block; the K halves of a single image
    (3, 64, 64, 1, 2),     # 3 stages over 2 splits: ranges [0, 1) and [1, 3)
    (5, 384, 384, 2, 0),   # conv4: grouped, 3 ci blocks of 64 per group, odd N
    (2, 256, 128, 1, 0),   # 4 ci blocks, 2 co blocks
    (2, 256, 128, 1, 3),   # ... and more splits asked for than there are stages
    (4, 96, 64, 1, 0),     # Cg % 64 != 0: the 64 x 32 form
]


def _rnd(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV).to(torch.bfloat16)


def _ref(x, dy, groups):
    C, Cout = x.shape[3], dy.shape[3]
    return torch.nn.grad.conv2d_weight(x.float().permute(0, 3, 1, 2), (Cout, C // groups, 3, 3),
                                       dy.float().permute(0, 3, 1, 2), stride=1, padding=1, groups=groups)


def _err(got, ref):
    return ((got - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_direct_tile(case):
    N, C, Cout, groups, splits = case
    g = ConvGeom(N, H, H, C, H, H, Cout, 3, 3, 1, 1, 1, groups)
    x = _rnd((N, H, H, C), 21)
    big = _rnd((N, H, H, Cout + 64), 22)
    dy = big[..., 64:]  # a channel slice: ldy = groups * Cog + 64
    ref = _ref(x, dy.contiguous(), groups)
    dbref = dy.float().sum((0, 1, 2))

    def run(with_db=True):
        dw = torch.full((Cout, 3, 3, C // groups), 0.5, device=DEV)
        db = torch.full((Cout,), 0.25, device=DEV) if with_db else None
        assert gemm.conv_wgrad_direct(x, dy, dw, g, splits=splits, db=db)
        torch.cuda.synchronize()
        return dw, db

    dw, db = run()
    e_w, e_b = _err((dw - 0.5).permute(0, 3, 1, 2), ref), _err(db - 0.25, dbref)
    print(f"{case}: dW rel err {e_w:.3e}, db rel err {e_b:.3e}")
    assert e_w < 1e-5, e_w
    assert e_b < 1e-5, e_b
    dw2, db2 = run()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)  # fixed split order, no atomics
    dw3, _ = run(with_db=False)
    assert torch.equal(dw, dw3)  # without the bias: same dW
    # += alpha * g: a second call on the same buffers adds the gradient again
    assert gemm.conv_wgrad_direct(x, dy, dw, g, splits=splits, db=db)
    torch.cuda.synchronize()
    assert _err((dw - 0.5).permute(0, 3, 1, 2), 2 * ref) < 1e-5
    assert _err(db - 0.25, 2 * dbref) < 1e-5
