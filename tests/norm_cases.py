"""Seeded inputs of the LRN / fused pool -> LRN / softmax bound tests, shared by the CPU self-test
(test_norm_bounds_cpu.py) and the GPU tests (test_lrn_bounds_gpu.py, test_softmax_bounds_gpu.py),
so that the emulation is checked at exactly the recipes the kernels are.  Every tensor holds exact
bf16 values, drawn on the CPU.

LRN parameters: the shipped nets' alpha = 1e-4 .. 1e-3 keeps norm = k + alpha / n sum x^2 within
[1, 1.03], where a missing window channel moves an output by less than bf16 rounding.  Here alpha
is 0.25 .. 1 on x of scale 2: the median norm is about 2 and the largest 4 .. 8 (up to 40 at
n = 9, alpha = 1), so every window channel carries weight."""
import torch

# (alpha, beta, k)
LRN_PARAMS = [(0.25, 0.75, 1.0), (1.0, 0.75, 1.0), (0.5, 0.5, 2.0)]
LRN_PARAM_IDS = ["a.25-b.75-k1", "a1-b.75-k1", "a.5-b.5-k2"]
LRN_SIZES = [1, 3, 4, 5, 7, 9]


def bf16_randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def lrn_inputs(npix, C, seed, relu=False):
    """(x, dy) bf16 [1][1][npix][C]: the pixels lie back to back, so a window that runs over its
    row's end reads the neighbouring pixel, not padding.  relu: x is a relu output (about half
    zeros), as in front of a mask_relu backward."""
    x = bf16_randn((1, 1, npix, C), seed, 2.0)
    if relu:
        x = x.clamp_min(0)
    return x, bf16_randn((1, 1, npix, C), seed + 1000)


def pool_inputs(N, H, W, C, seed, nonneg):
    """(x, dY) for the fused pool -> LRN: signed x ~ N(-1.5, 2.5), so that a window's maximum is
    about 2 but not > 0 in ~5 % of the windows (the relu' bit), or (nonneg, the integer-key path's
    contract) a relu output drawn from few values, three quarters of them zeros with -0.0 among
    them: windows hold ties, and ~7 % are all zero; dY bf16 of the pooled shape."""
    g = torch.Generator().manual_seed(seed)
    if nonneg:
        vals = torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0, 0.0, -0.0, 0.0, -0.0, 0.5, 1.0, 2.0, 4.0])
        x = vals[torch.randint(0, 16, (N, H, W, C), generator=g)].to(torch.bfloat16)
    else:
        x = (torch.randn(N, H, W, C, generator=g) * 2.5 - 1.5).to(torch.bfloat16)
    Ho, Wo = min(H - 2, H - 1) // 2 + 1, min(W - 2, W - 1) // 2 + 1
    return x, bf16_randn((N, Ho, Wo, C), seed + 1000)


SOFTMAX_K = [1, 63, 64, 65, 256, 257, 512, 513, 1000, 1024, 1025, 1500]
SOFTMAX_RECIPES = ["scale3", "scale8", "const", "peak_first", "peak_last", "peak_lane", "neg80"]


def peak_index(recipe, K):
    """where the one element of 80 sits: index 0, K - 1, or a lane other than the row's first (lane
    37; of the second 64-element slice when the row has one)"""
    if recipe == "peak_first":
        return 0
    if recipe == "peak_last":
        return K - 1
    return 101 if K > 101 else (37 if K > 37 else K - 1)


def softmax_input(recipe, rows, K, seed=0):
    if recipe == "scale3":
        return bf16_randn((rows, K), seed + 1, 3.0)
    if recipe == "scale8":
        return bf16_randn((rows, K), seed + 2, 8.0)
    if recipe == "const":
        return (torch.arange(rows, dtype=torch.float32).reshape(rows, 1) * 1.5 - 2.0).expand(rows, K).to(torch.bfloat16).contiguous()
    if recipe == "neg80":
        return (bf16_randn((rows, K), seed + 3).float() - 80.0).to(torch.bfloat16)
    x = bf16_randn((rows, K), seed + 4, 0.5)
    x[:, peak_index(recipe, K)] = 80.0
    return x


def softmax_labels(rows, K, seed=0):
    """fp32 [rows][1] class labels that include class 0 and class K - 1"""
    g = torch.Generator().manual_seed(seed + 5)
    lab = torch.randint(0, K, (rows, 1), generator=g)
    lab[0, 0] = 0
    lab[rows - 1, 0] = K - 1
    return lab.float()
