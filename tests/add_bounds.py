"""Float64 reference, derived per-element bound and shared test inputs of the `add` kernels
(csrc/kernels/add_kernels.hip): y = [relu](x0 + x1 (+ x2 + x3)) stored as bf16.

The bound has the form of tests/bounds.py:
    ref   = sum_k x_k  in float64 (the bf16 inputs are exact there)
    A     = sum_k |x_k|
    g     = (N + 2) 2^-23     N - 1 fp32 additions in any order err by at most (N - 1) 2^-24 A;
                              the rest covers a second rounding of the sum before the store
    bound = u (|ref| + g A) + g A,   u = 2^-8 the bf16 unit roundoff
It is taken before the relu, which is 1-Lipschitz: |relu(a) - relu(b)| <= |a - b|.  Where
ref < -bound every value within the bound of ref is negative, so the relu'd output must be
exactly 0: the bound there is 0.  Derived, not tuned.  Everything runs on the CPU."""
import functools

import torch

from bounds import EPS_F32, U_BF16, assert_within, violations  # noqa: F401

# name -> (node shape, element offset of the view into a 16-byte aligned buffer)
CASES = {
    "n8": ((8,), 0),                 # a single run, the vector path
    "n225": ((3, 5, 5, 3), 0),       # scalar path, 28 full runs and a tail of 1
    "n10": ((1, 10), 0),             # a matrix node: scalar path, one full run and a tail of 2
    "n6272": ((2, 7, 7, 64), 0),     # vector path, 784 runs: 3 full blocks of 256 threads and one of 16
    "off1": ((4, 16), 1),            # n % 8 == 0 but every buffer starts 2 bytes past alignment: scalar path
}
NS = (2, 3, 4)


def numel(name):
    n = 1
    for s in CASES[name][0]:
        n *= s
    return n


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(xs, g): four bf16 inputs and a bf16 output gradient of the case, flat, on the CPU, the same
    for every N (an N-input test takes xs[:N]).  Planted: x1 = -x0 on every 5th element (an exact
    cancellation: with N = 2, y = 0, the mask bit is 0 and the gradient is exactly 0), -0.0 in
    x0 and x1 at element 1 (and 0 in x2, x3, so that the sum is -0.0 for every N), and 2^8 in x0
    next to 2^-8 in x1 at element 2."""
    n = numel(name)
    gen = torch.Generator().manual_seed(1000 + n + CASES[name][1])
    xs = [torch.randn(n, generator=gen).to(torch.bfloat16) for _ in range(4)]
    xs[1][::5] = -xs[0][::5]
    xs[0][1] = xs[1][1] = -0.0
    xs[2][1] = xs[3][1] = 0.0
    xs[0][2], xs[1][2] = 2.0 ** 8, 2.0 ** -8
    g = torch.randn(n, generator=gen).to(torch.bfloat16)
    return tuple(xs), g


def add_ref(xs, relu):
    """(ref, bound), float64, flat, of y = [relu](sum xs) stored as bf16."""
    x64 = [x.detach().to("cpu", torch.float64).reshape(-1) for x in xs]
    ref = sum(x64[1:], x64[0])
    A = sum((x.abs() for x in x64[1:]), x64[0].abs())
    gA = (len(xs) + 2) * EPS_F32 * A
    bound = U_BF16 * (ref.abs() + gA) + gA
    if relu:
        bound = torch.where(ref < -bound, torch.zeros_like(bound), bound)
        ref = ref.clamp_min(0)
    return ref, bound


@functools.lru_cache(maxsize=None)
def case_ref(name, N, relu):
    """add_ref of the case's first N inputs, computed once and shared."""
    return add_ref(inputs(name)[0][:N], bool(relu))


def emulate(xs, relu):
    """What the kernels compute: fp32 sum in input order, relu, one rounding to bf16."""
    acc = xs[0].float()
    for x in xs[1:]:
        acc = acc + x.float()
    if relu:
        acc = torch.where(acc > 0, acc, torch.zeros_like(acc))
    return acc.to(torch.bfloat16)
