"""relu6 / hsigmoid / hswish kernels (csrc/kernels/hact_kernels.hip): every kind, forward and backward,
per element against the float64 bounds of tests/hact_bounds.py (relu6 bit for bit), with sentinel guards
around every buffer.  The cases are flat element counts, the smallest at which the kernels can go
wrong: one element; a tail alone; one vector and no tail; a full block and a tail; one more than a pass
of the capped grid covers, so that a thread makes a second grid-stride trip (2048 blocks x 256 threads
x 8 elements and 256 runs more: 8.4 MB a buffer, a third of a second a test); and the scalar path by
alignment, of every buffer and of the output alone."""
import pytest
import torch

import hact_bounds as H
from cxxnet_amd import native
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24  # elements after (and `off` before) each buffer that must stay untouched
FILL = 3.0
PASS = 2048 * 256 * 8  # elements one pass of the capped grid covers: asserted in test_the_second_trip_case
# name -> (n, element offset of x / g into their 16-byte aligned buffers, offset of the output)
CASES = {
    "n1": (1, 0, 0),
    "tail7": (7, 0, 0),
    "vec8": (8, 0, 0),
    "block": (8 * 256 + 5, 0, 0),
    "trip2": (PASS + 8 * 256, 0, 0),          # vector path, 256 runs left for the second trip
    "off1": (40, 1, 1),                       # every buffer starts 2 bytes past alignment
    "out_off1": (40, 0, 1),                   # only the output does
}


def _buf(n, off, src=None):
    """A device bf16 buffer of off + n + GUARD elements filled with FILL; the view of its n elements
    from element `off` (holding src) and the whole buffer."""
    whole = torch.full((off + n + GUARD,), FILL, dtype=torch.bfloat16, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + n]
    if src is not None:
        view.copy_(src)
    return view, whole


def _guards_intact(whole, off, n):
    return bool((whole[:off] == FILL).all() and (whole[off + n:] == FILL).all())


def _same_bits(t, cpu):
    return torch.equal(t.view(torch.int16), cpu.to(t.device).view(torch.int16))


def _check(kind, key, n, got):
    ref, bound = H.case_ref(kind, n)[key]
    worst = H.assert_within(got, ref, bound, "%s %s n=%d" % (kind, key, n), axes="i")
    if kind == "relu6":  # exact, the sign of a zero included
        assert torch.equal(H.bits(got), H.ref_bits(ref))
    return worst


def test_the_second_trip_case():
    assert L.hact_pass_elems() == PASS == native.kernels().cxn_hact_pass_elems()
    assert CASES["trip2"][0] > PASS and CASES["trip2"][0] % 8 == 0
    assert CASES["block"][0] < PASS


def _forward(kind, name):
    n, off_in, off_out = CASES[name]
    x_cpu, _ = H.inputs(n)
    x, x_whole = _buf(n, off_in, x_cpu)
    y, y_whole = _buf(n, off_out)
    L.hact_forward(kind, x, y)
    torch.cuda.synchronize()
    assert _guards_intact(y_whole, off_out, n), "forward wrote past y"
    assert _same_bits(x, x_cpu) and _guards_intact(x_whole, off_in, n), "x was written"
    return y.cpu()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", H.KINDS)
def test_forward(kind, name):
    n = CASES[name][0]
    y = _forward(kind, name)
    print(kind, name, "forward worst d/bound", _check(kind, "y", n, y))
    yb = H.bits(y)
    x_cpu = H.inputs(n)[0]
    if kind == "relu6":
        assert yb[0] == 0                                   # relu6(-0.0) = +0
    if kind == "hsigmoid":
        assert y[0] == 0.5
    if kind == "hswish" and n >= 18:                        # x >= 3: the same bits (3, 6, 3.015625, 5.96875, 6.03125, 2^8)
        for i in (2, 4, 8, 11, 12, 14):
            assert float(x_cpu[i]) >= 3 and yb[i] == H.bits(x_cpu)[i]
    if n >= 18:                                             # the subnormal neighbours of 0, x[9] = -2^-133, x[10] = 2^-133
        assert H.bits(x_cpu)[9:11].tolist() == [-32767, 1]
        if kind == "relu6":
            assert yb[9:11].tolist() == [0, 1]              # +0 and the subnormal's own bits: nothing flushed
        if kind == "hsigmoid":
            assert (y[9:11] == 0.5).all()
    assert torch.equal(H.bits(_forward(kind, name)), yb)    # a second run: the same bits


def _backward(kind, name, alias):
    n, off_in, off_out = CASES[name]
    x_cpu, g_cpu = H.inputs(n)
    x, x_whole = _buf(n, off_out if alias else off_in, x_cpu)
    g, g_whole = _buf(n, off_in, g_cpu)
    off_dx = off_out
    dx, dx_whole = (x, x_whole) if alias else _buf(n, off_dx)
    L.hact_backward(kind, x, g, dx)
    torch.cuda.synchronize()
    assert _guards_intact(dx_whole, off_dx, n), "backward wrote past dx"
    assert _same_bits(g, g_cpu) and _guards_intact(g_whole, off_in, n), "g was written"
    if not alias:
        assert _same_bits(x, x_cpu) and _guards_intact(x_whole, off_in, n), "x was written"
    return dx.cpu()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", H.KINDS)
def test_backward(kind, name):
    """dx of its own and dx = x (the in-place node) give the same bits, inside the bounds; so does a
    second run"""
    n = CASES[name][0]
    dx = _backward(kind, name, False)
    print(kind, name, "backward worst d/bound", _check(kind, "dx", n, dx))
    assert torch.equal(H.bits(_backward(kind, name, True)), H.bits(dx)), "dx = x gives other bits"
    assert torch.equal(H.bits(_backward(kind, name, False)), H.bits(dx))
    if kind == "relu6" and n >= 18:  # x = +-2^-133 with g = 1 / -0.0: 2^-133 is inside, its g kept; -2^-133 is not
        assert H.bits(dx)[9:11].tolist() == [0, H.bits(H.inputs(n)[1])[10]]
    if kind in ("relu6", "hswish") and n >= 18:
        g_cpu = H.inputs(n)[1]
        j = 15 if kind == "relu6" else 14  # x = 2^-8 (relu6: inside) / 2^8 (hswish: x >= 3) keep g's bits, 1 / -0.0
        assert H.bits(dx)[j] == H.bits(g_cpu)[j]


def test_launchers_reject_bad_arguments():
    """x = g = 1 and an output of its own filled with FILL = 3: every kind's forward (1, 2/3, 2/3) and
    backward (1, 1/6, 5/6) would change the output, so a launch behind a non-zero return shows"""
    k = native.kernels()
    x = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    out = torch.full((64,), FILL, dtype=torch.bfloat16, device=DEV)
    px, pg, po = x.data_ptr(), g.data_ptr(), out.data_ptr()
    for kind in (0, 1, 2):
        assert k.cxn_hact_fwd(None, po, 64, kind, None) != 0
        assert k.cxn_hact_fwd(px, None, 64, kind, None) != 0
        assert k.cxn_hact_fwd(px, po, 0, kind, None) != 0
        assert k.cxn_hact_fwd(px, po, -8, kind, None) != 0
        assert k.cxn_hact_bwd(None, pg, po, 64, kind, None) != 0
        assert k.cxn_hact_bwd(px, None, po, 64, kind, None) != 0
        assert k.cxn_hact_bwd(px, pg, None, 64, kind, None) != 0
        assert k.cxn_hact_bwd(px, pg, po, 0, kind, None) != 0
        assert k.cxn_hact_bwd(px, pg, po, -8, kind, None) != 0
    for kind in (3, -1, 43):
        assert k.cxn_hact_fwd(px, po, 64, kind, None) != 0
        assert k.cxn_hact_bwd(px, pg, po, 64, kind, None) != 0
    torch.cuda.synchronize()
    assert (out == FILL).all() and (x == 1).all() and (g == 1).all()
    with pytest.raises(ValueError, match="hact"):
        L.hact_forward("swish", x, out)
    with pytest.raises(ValueError, match="bf16"):
        L.hact_forward("hswish", x.float(), torch.empty(64, device=DEV))
    with pytest.raises(ValueError, match="alias"):
        L.hact_forward("hswish", x, x)
    with pytest.raises(ValueError, match="alias"):
        L.hact_backward("hswish", x, g, g)
    torch.cuda.synchronize()
    assert (out == FILL).all() and (x == 1).all() and (g == 1).all()
    assert k.cxn_hact_fwd(px, po, 64, 1, None) == 0  # and the same call with good arguments does write
    torch.cuda.synchronize()
    assert (out != FILL).all()


@pytest.mark.parametrize("kind", H.KINDS)
def test_a_layer_sized_for_batch_3_runs_at_batch_2(kind):
    """A smaller current batch (nodes sliced to their first rows, as the executor does) gives those
    rows' results and leaves the third row of every node untouched."""
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    C, Hh, W = 5, 3, 4  # 60 elements per row: 120 at batch 2
    n = 2 * C * Hh * W
    x_cpu, g_cpu = H.inputs(n)
    x, o = Node("x"), Node("o")
    x.set_shape(3, C, Hh, W)
    lay = create_layer({"relu6": 43, "hsigmoid": 44, "hswish": 45}[kind], LayerContext(torch.device(DEV)))
    lay.init_connection([x], [o])
    full = {}
    for nd in (x, o):
        nd.alloc(DEV, torch.bfloat16)
        nd.data.fill_(FILL)
        full[nd.name] = nd.data
        nd.data = nd.data[:2]
    x.data.copy_(x_cpu.view(x.data.shape))
    lay.forward(True, [x], [o])
    H.assert_within(o.data.reshape(-1), *H.forward_ref(kind, x_cpu), kind + " y at batch 2", axes="i")
    o.data.copy_(g_cpu.view(o.data.shape))
    lay.backprop(True, [x], [o])
    torch.cuda.synchronize()
    H.assert_within(x.data.reshape(-1), *H.backward_ref(kind, x_cpu, g_cpu), kind + " dx at batch 2", axes="i")
    assert _same_bits(o.data.reshape(-1), g_cpu)
    for nd in (x, o):
        assert (full[nd.name][2:] == FILL).all()
