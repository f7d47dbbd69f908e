"""Seeded inputs of the batch_norm / element-wise / optimizer bound tests, shared by the CPU self-test
(test_layer_bounds_cpu.py) and the GPU tests (test_bn_layer_bounds_gpu.py,
test_elementwise_bounds_gpu.py, test_fused_update_bounds_gpu.py), so that the emulation and the
injected defects are judged on exactly the inputs the kernels are.  Every tensor is drawn on the
CPU and holds exact bf16 values (activations) or fp32 values (statistics, parameters, state)."""
import functools

import torch

import bn_bounds as BN

SENTINEL = 7.25  # exact in bf16 and fp32; no test writes it


def bf16_randn(shape, seed, scale=1.0, shift=0.0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=gen) * scale + shift).to(torch.bfloat16)


def guarded(t, device, guard=64):
    """(buffer, view): t copied to the device as the head of a sentinel-filled flat buffer with
    `guard` elements behind it; the view has t's shape."""
    buf = torch.full((t.numel() + guard,), SENTINEL, dtype=t.dtype, device=device)
    buf[:t.numel()].copy_(t.reshape(-1))
    return buf, buf[:t.numel()].view(t.shape)


def guarded_empty(shape, dtype, device, guard=64):
    """(buffer, view) of an output: the whole buffer holds the sentinel."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + guard,), SENTINEL, dtype=dtype, device=device)
    return buf, buf[:n].view(shape)


def assert_guard(buf, n, what=""):
    tail = buf[n:].float().cpu()
    assert bool((tail == SENTINEL).all()), "%s: written behind the end of the output" % what


# ------------------------------------------------------------------------------------ batch_norm
# name -> (rows, C); "const" has channel 5 constant
BN_CASES = {
    "r3": (3, 8),          # one of the four row lanes is idle
    "r98": (98, 24),       # the layer test's shape
    "c": (130, 64),        # bn_bounds.case_c_inputs: mean / std ~ 50
    "r257": (257, 72),     # two row blocks (129 + 128 rows), a second channel group of 8 channels
    "r1030": (1030, 136),  # five row blocks; three channel groups, the last with 8 channels
    "const": (98, 24),     # a constant channel (eps = 1e-5 only)
}
BN_EPS = [1e-10, 1e-5]
BN_RUNS = [(n, e) for n in BN_CASES for e in BN_EPS if not (n == "const" and e != 1e-5)]
BN_IDS = ["%s-eps%g" % r for r in BN_RUNS]


@functools.lru_cache(maxsize=None)
def bn_inputs(name):
    """dict x, gy (bf16 [R][C]), slope, bias, gs0, gb0 (fp32 [C]).  gy has a non-zero column mean
    and is correlated with x, so that both correction terms of dx carry weight."""
    R, C = BN_CASES[name]
    seed = sum(ord(ch) for ch in name)
    gen = torch.Generator().manual_seed(seed)
    if name == "c":
        x = BN.case_c_inputs(R, C, 3)
        xn = (x.float() - 64.0) / 1.3
    else:
        x = (torch.randn(R, C, generator=gen) * 2.0 + 0.5).to(torch.bfloat16)
        xn = (x.float() - 0.5) / 2.0
    if name == "const":
        x[:, 5] = 1.5
        xn[:, 5] = 0.0
    gy = (torch.randn(R, C, generator=gen) + 0.5 + 0.25 * xn).to(torch.bfloat16)
    slope = torch.rand(C, generator=gen) + 0.5
    bias = torch.randn(C, generator=gen)
    gs0, gb0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    return dict(R=R, C=C, x=x, gy=gy, slope=slope, bias=bias, gs0=gs0, gb0=gb0)


# ------------------------------------------------------------------------------------ prelu
PRELU_SHAPES = [(3, 8), (75, 16), (300, 72)]
PRELU_RND = [0.0, 0.3]
PRELU_SEED, PRELU_COUNTER = 1234, 3


@functools.lru_cache(maxsize=None)
def prelu_inputs(rows, C):
    gen = torch.Generator().manual_seed(rows * 131 + C)
    x = bf16_randn((rows, C), rows + C)
    x[0, 0], x[0, 1] = 0.0, -0.0
    gy = bf16_randn((rows, C), rows + C + 1)
    slope = torch.rand(C, generator=gen) * 0.5
    slope[0], slope[1], slope[2] = -0.3, 1.7, 0.25  # clamps to 0, clamps to 1, plain
    gs0 = torch.randn(C, generator=gen)
    return dict(x=x, gy=gy, slope=slope, gs0=gs0)


# ------------------------------------------------------------------------------------ insanity
INSANITY_N = [5, 8, 1152, 2053]
INSANITY_LB, INSANITY_UB, INSANITY_SEED, INSANITY_COUNTER = 3.0, 8.0, 99, 11


@functools.lru_cache(maxsize=None)
def insanity_inputs(n):
    return bf16_randn((n,), 80 + n), bf16_randn((n,), 90 + n)


# ------------------------------------------------------------------------------------ insanity pooling
INS_POOL_SHAPES = [(2, 9, 9, 8, 3, 2), (2, 5, 5, 24, 2, 2), (1, 6, 7, 8, 3, 1), (2, 1, 4, 8, 3, 2), (1, 2, 2, 8, 3, 2)]
INS_POOL_KEEP = [1.0, 0.6, 0.0]
INS_POOL_SEED, INS_POOL_COUNTER = 77, 5


@functools.lru_cache(maxsize=None)
def ins_pool_inputs(N, H, W, C, K, S):
    """x in multiples of 0.5 (windows hold ties, which all take the gradient), gy of the pooled shape"""
    from layer_bounds import ins_pool_out
    x = (bf16_randn((N, H, W, C), 10 + H * W + C, 2.0).float() * 2).round().div(2).to(torch.bfloat16)
    return x, bf16_randn((N, ins_pool_out(H, K, S), ins_pool_out(W, K, S), C), 11 + H * W + C)


# ------------------------------------------------------------------------------------ activations, dropout
ACT_N = [1, 7, 8, 1003, 2048 * 8 + 5]
ACT_HEAD = [0.0, -0.0, 2.0 ** -130, -2.0 ** -130, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 3e38, -3e38]
# for n <= 8 (n < 8: no vector body, every element goes through block 0's tail): zeros, a
# denormal and saturating values among the first seven
ACT_HEAD_SHORT = [-0.0, -88.0, 3e38, -100.0, 2.0 ** -130, -3e38, 0.0, 88.0]
XELU_B = 5.0


@functools.lru_cache(maxsize=None)
def act_inputs(n):
    """x: N(0, 3) with the fixed head in front (the 8-wide body) and once more at the end (the last
    n % 8 elements, the saturating ones, go through block 0's tail); n <= 8: the short head.
    dy: N(0, 1)."""
    x = bf16_randn((n,), 40 + n, 3.0)
    if n <= len(ACT_HEAD_SHORT):
        x[:] = torch.tensor(ACT_HEAD_SHORT[:n]).to(torch.bfloat16)
    else:
        head = torch.tensor(ACT_HEAD).to(torch.bfloat16)
        x[:head.numel()] = head
        x[-head.numel():] = head
    return x, bf16_randn((n,), 50 + n)


DROPOUT_N = [5, 8, 4099]
DROPOUT_PKEEP = [0.5, 0.3, 1.0]
DROPOUT_SEED, DROPOUT_COUNTER = 4321, 9


@functools.lru_cache(maxsize=None)
def dropout_inputs(n):
    return bf16_randn((n,), 60 + n)


# ------------------------------------------------------------------------------------ fused_update
def update_table():
    """(arena size, segments (offset, n, lr, wd, mom, clip)): 4-aligned segments with n % 4 in
    {0, 1, 2, 3}, n in {1, 3, 0}, an unaligned offset (element-wise path), gaps between the
    segments, and different lr / wd / mom / clip in neighbouring segments; wd = 0 and wd > 0, clip
    = 0 and clip > 0.  (lr, wd and mom are not fp32 numbers: the reference takes their fp32
    roundings, as the kernel is handed them.)"""
    segs = [
        (0, 1024, 0.01, 0.0005, 0.9, 0.0),    # n % 4 == 0
        (1088, 301, 0.02, 0.01, 0.8, 0.5),    # n % 4 == 1, clip > 0 (NaN / +-inf gradients live here)
        (1408, 6, 0.005, 0.0, 0.95, 0.0),     # n % 4 == 2, wd = 0
        (1472, 1027, 0.03, 0.02, 0.5, 1.0),   # n % 4 == 3, more than one block row of vectors
        (2560, 1, 0.01, 0.01, 0.9, 0.0),      # n = 1
        (2564, 3, 0.04, 0.0, 0.7, 0.25),      # n = 3, directly behind a gap of 3
        (2568, 0, 0.5, 0.5, 0.5, 0.0),        # n = 0: a no-op
        (2571, 130, 0.015, 0.005, 0.85, 0.0),  # unaligned offset: element-wise path
        (2703, 5, 0.025, 0.03, 0.6, 2.0),     # unaligned, directly behind its neighbour's gap of 2
    ]
    return 2816, segs


def chunk_table(nseg):
    """(arena size, nseg segments) of mixed small sizes, with gaps: cxn_fused_update launches 48
    segments at a time, so 49 and 97 segments take 2 and 3 launches."""
    sizes = [1, 3, 4, 7, 16, 0, 33, 64, 5, 130]
    segs, off = [], 0
    for i in range(nseg):
        n = sizes[i % len(sizes)]
        if i % 3 == 1:
            off += 1  # an unaligned start
        segs.append((off, n, 0.01 + 0.001 * (i % 7), 0.0 if i % 4 == 0 else 0.001 * (1 + i % 5), 0.5 + 0.05 * (i % 8),
                     0.0 if i % 2 else 0.75))
        off = (off + n + 3 + i % 3) // 4 * 4 if i % 5 else off + n + 2
    return off + 64, segs


def update_state(size, segs, algo, seed=0, special=True):
    """dict of the fp32 state before the step: w, g, m1, m2 (adam: positive), with the sentinel in
    every gap.  special: NaN and +-inf among the gradients of the sgd segments with clip > 0."""
    gen = torch.Generator().manual_seed(seed + 17)
    w = torch.full((size,), SENTINEL)
    gr, m1, m2 = w.clone(), w.clone(), w.clone()
    for off, n, lr, wd, mom, clip in segs:
        w[off:off + n] = torch.randn(n, generator=gen) * 1.5
        gr[off:off + n] = torch.randn(n, generator=gen)
        m1[off:off + n] = torch.randn(n, generator=gen) * 0.1
        m2[off:off + n] = torch.rand(n, generator=gen) * 0.5 + 0.01
        if special and algo == "sgd" and clip > 0 and n >= 5:
            gr[off] = float("nan")
            gr[off + 1] = float("inf")
            gr[off + n - 1] = float("-inf")  # (in the tail of a vector segment)
            gr[off + 2] = 3.0 * clip
    return dict(w=w, g=gr, m1=m1, m2=m2)
