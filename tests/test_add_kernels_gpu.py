"""add kernels (csrc/kernels/add_kernels.hip): the forward per element against the float64 bound
of tests/add_bounds.py, the mask and the backward bit for bit.  The cases are the smallest at which
the kernels can go wrong (add_bounds.CASES): one run; the scalar path with a tail (n = 225, n = 10);
several blocks with a ragged last one -- 2 x 7 x 7 x 64 = 6272 elements are 784 runs of 8, three
blocks of 256 threads and one with 16 live threads; buffers that start 2 bytes past a 16-byte
boundary with n % 8 == 0; and one size past the grid cap, where a thread walks more than one run."""
import numpy as np
import pytest
import torch

import add_bounds as A
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24  # elements (bytes for the mask) after each buffer that must stay untouched
FILL = 3.0


def _buf(n, off, src=None):
    """A device bf16 buffer of `off` + n + GUARD elements filled with FILL; the view of its n
    elements from element `off` (holding src) and the whole buffer."""
    whole = torch.full((off + n + GUARD,), FILL, dtype=torch.bfloat16, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + n]
    if src is not None:
        view.copy_(src)
    return view, whole


def _guards_intact(whole, off, n):
    w = whole.cpu()
    return bool((w[:off] == FILL).all() and (w[off + n:] == FILL).all())


def _state(n):
    st = L.AddState(n, DEV, True)
    nb = (n + 7) // 8
    assert st.mask.numel() == nb and st.mask.dtype == torch.uint8
    whole = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    st.mask = whole[:nb]
    return st, whole


def _bits(t):
    return t.cpu().view(torch.int16)


def _packed(y):
    """the mask bytes of a stored y: bit j of byte r = (y[8 r + j] > 0)"""
    return torch.from_numpy(np.packbits((y.cpu().float() > 0).numpy(), bitorder="little"))


def _run(xs_cpu, g_cpu, off, relu, ref, bound, what):
    n, N = g_cpu.numel(), len(xs_cpu)
    xs = [_buf(n, off, x) for x in xs_cpu]
    y, y_whole = _buf(n, off)
    st, mask_whole = _state(n) if relu else (None, None)
    L.add_forward([v for v, _ in xs], y, bool(relu), st)
    A.assert_within(y, ref, bound, what + " y", axes="i")
    assert _guards_intact(y_whole, off, n), "forward wrote past y"
    for (v, whole), x in zip(xs, xs_cpu):
        assert torch.equal(_bits(v), _bits(x)) and _guards_intact(whole, off, n), "an input was written"
    y_cpu = y.cpu()
    if relu:
        assert (y_cpu.float() >= 0).all() and not (_bits(y_cpu) == -32768).any()  # no -0.0 behind a relu
        assert torch.equal(st.mask.cpu(), _packed(y_cpu)), "mask != (stored y > 0)"
        assert (mask_whole.cpu()[st.mask.numel():] == 0xA5).all(), "forward wrote past the mask"
    if N == 2:  # x1 = -x0 on every 5th element: exactly 0
        assert (y_cpu[::5].float() == 0).all()
    # inference (no mask) writes the same y; so does a second training run, mask included
    y2, _ = _buf(n, off)
    L.add_forward([v for v, _ in xs], y2, bool(relu), None)
    assert torch.equal(_bits(y2), _bits(y_cpu))
    if relu:
        st2, _ = _state(n)
        y3, _ = _buf(n, off)
        L.add_forward([v for v, _ in xs], y3, True, st2)
        assert torch.equal(_bits(y3), _bits(y_cpu)) and torch.equal(st2.mask, st.mask)

    g, g_whole = _buf(n, off, g_cpu)
    ds = [_buf(n, off) for _ in range(N)]
    L.add_backward(g, [v for v, _ in ds], st)
    want = torch.where(y_cpu.float() > 0, g_cpu, torch.zeros_like(g_cpu)) if relu else g_cpu
    for k, (v, whole) in enumerate(ds):
        assert torch.equal(_bits(v), _bits(want)), "%s: gradient of input %d" % (what, k)
        assert _guards_intact(whole, off, n), "backward wrote past destination %d" % k
    assert torch.equal(_bits(g), _bits(g_cpu)) and _guards_intact(g_whole, off, n)
    if relu:
        assert torch.equal(st.mask.cpu(), _packed(y_cpu)), "backward changed the mask"
        if N == 2:
            assert (_bits(ds[0][0])[::5] == 0).all()  # the cancellations: gradient exactly +0
    ds2 = [_buf(n, off) for _ in range(N)]
    L.add_backward(g, [v for v, _ in ds2], st)
    for (a, _), (b, _) in zip(ds, ds2):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", A.NS)
@pytest.mark.parametrize("name", list(A.CASES))
def test_forward_and_backward(name, N, relu):
    xs, g = A.inputs(name)
    ref, bound = A.case_ref(name, N, relu)
    off = A.CASES[name][1]
    if name == "n6272":
        assert A.numel(name) % 8 == 0 and (A.numel(name) // 8) % 256 == 16  # a ragged last block
    _run(xs[:N], g, off, relu, ref, bound, "%s N=%d relu=%d" % (name, N, relu))


def test_the_planted_values_are_there():
    xs, _ = A.inputs("n8")
    assert _bits(xs[0])[1] == -32768 and _bits(xs[1])[1] == -32768  # -0.0
    assert xs[0][2] == 256 and xs[1][2] == 2.0 ** -8
    assert torch.equal(xs[1][::5], -xs[0][::5])
    y = torch.empty(8, dtype=torch.bfloat16, device=DEV)
    L.add_forward([x.to(DEV) for x in xs[:2]], y, False)
    assert _bits(y)[1] == -32768  # -0.0 + -0.0 without relu stays -0.0
    assert y[2] == 256            # 2^8 + 2^-8 rounds to 2^8


@pytest.mark.parametrize("tail", [0, 3])
def test_past_the_grid_cap(tail):
    """More runs than 2048 blocks x 256 threads: the grid-stride loop takes a second, partial sweep
    (tail = 3: on the scalar path, ending in a short run)."""
    n = 2048 * 256 * 8 + 2400 + tail
    gen = torch.Generator().manual_seed(n)
    xs = [torch.randn(n, generator=gen).to(torch.bfloat16) for _ in range(4)]
    g = torch.randn(n, generator=gen).to(torch.bfloat16)
    ref, bound = A.add_ref(xs, True)
    _run(xs, g, 0, 1, ref, bound, "n=%d" % n)


def test_launcher_rejects_bad_counts():
    from cxxnet_amd import native
    k = native.kernels()
    t = torch.zeros(8, dtype=torch.bfloat16, device=DEV)
    p = t.data_ptr()
    assert k.cxn_add_fwd(p, None, None, None, 1, p, None, 8, 0, None) != 0
    assert k.cxn_add_fwd(p, p, None, None, 3, p, None, 8, 0, None) != 0   # a null input among the first n_in
    assert k.cxn_add_fwd(p, p, p, p, 5, p, None, 8, 0, None) != 0
    assert k.cxn_add_bwd(p, None, p, None, None, None, 2, 8, None) != 0
    assert k.cxn_add_bwd(p, None, p, p, p, p, 5, 8, None) != 0
    assert k.cxn_add_fwd(p, p, None, None, 2, p, None, 0, 0, None) != 0
    torch.cuda.synchronize()
    assert (t == 0).all()
