"""silu kernels (csrc/kernels/silu_kernels.hip): forward and backward, per element against the float64
bounds of tests/silu_bounds.py, with sentinel guards around every buffer.  The cases are flat element
counts, the smallest at which the kernels can go wrong: one vector and no tail; a tail alone; a run and a
tail of one (the scalar path by n); 64 elements in buffers that start 8 bytes past a 16-byte boundary
(the scalar path by alignment); 4099, several blocks and a tail; and one more than a pass of the capped
grid covers, so that a thread makes a second grid-stride trip (2048 blocks x 256 threads x 8 elements
and 256 runs more: 8.4 MB a buffer)."""
import pytest
import torch

import silu_bounds as S
from cxxnet_amd import native
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24  # elements after (and `off` before) each buffer that must stay untouched
FILL = 3.0
PASS = 2048 * 256 * 8  # elements one pass of the capped grid covers: asserted in test_the_second_trip_case
NP = len(S.PLANTED_X)
# name -> (n, element offset of every buffer from a 16-byte boundary)
CASES = {
    "vec8": (8, 0),
    "tail7": (7, 0),
    "run9": (9, 0),
    "off4": (64, 4),                          # n % 8 == 0, every buffer 8 bytes past alignment
    "blocks": (4099, 0),
    "trip2": (PASS + 8 * 256, 0),             # vector path, 256 runs left for the second trip
}


def _buf(n, off, src=None):
    """A device bf16 buffer of off + n + GUARD elements filled with FILL; the view of its n elements
    from element `off` (holding src) and the whole buffer."""
    whole = torch.full((off + n + GUARD,), FILL, dtype=torch.bfloat16, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + n]
    assert view.data_ptr() % 16 == (2 * off) % 16
    if src is not None:
        view.copy_(src)
    return view, whole


def _guards_intact(whole, off, n):
    return bool((whole[:off] == FILL).all() and (whole[off + n:] == FILL).all())


def _same_bits(t, cpu):
    return torch.equal(t.view(torch.int16), cpu.to(t.device).view(torch.int16))


def _check(key, n, got):
    ref, bound = S.case_ref(n)[key]
    return S.assert_within(got, ref, bound, "silu %s n=%d" % (key, n), axes="i")


def test_the_second_trip_case():
    assert L.silu_pass_elems() == PASS == native.kernels().cxn_silu_pass_elems()
    assert CASES["trip2"][0] > PASS and CASES["trip2"][0] % 8 == 0
    assert CASES["blocks"][0] < PASS


def _forward(name):
    n, off = CASES[name]
    x_cpu, _ = S.inputs(n)
    x, x_whole = _buf(n, off, x_cpu)
    y, y_whole = _buf(n, off)
    L.silu_forward(x, y)
    torch.cuda.synchronize()
    assert _guards_intact(y_whole, off, n), "forward wrote past y"
    assert _same_bits(x, x_cpu) and _guards_intact(x_whole, off, n), "x was written"
    return y.cpu()


def _planted_places(n):
    """the element ranges that hold PLANTED_X in full: the head, and the tail where inputs() wrote it"""
    return [b for b in ([0] if n >= NP else []) + ([n - NP] if n >= 2 * NP else [])]


@pytest.mark.parametrize("name", list(CASES))
def test_forward(name):
    n = CASES[name][0]
    y = _forward(name)
    print(name, "forward worst d/bound", _check("y", n, y))
    yb, xb = S.bits(y), S.bits(S.inputs(n)[0])
    assert torch.isfinite(y.float()).all()
    assert yb[0] == -32768 and (n < 2 or yb[1] == 0)         # silu(-0.0) = -0, silu(0) = +0
    for base in _planted_places(n):
        for j in (13, 15, 17):                               # x = 2^8, 88, 100: sigma = 1, y = x, the same bits
            assert yb[base + j] == xb[base + j]
        assert yb[base + 12] == -32768 and yb[base + 16] == -32768   # x = -2^8, -100: e^-x overflows, y = -0
        assert y[base + 14] == 0 or y[base + 14] < 0         # x = -88: ref = -5e-37 or a zero (the bound holds which)
    assert torch.equal(S.bits(_forward(name)), yb)           # a second run: the same bits


def _backward(name, alias):
    n, off = CASES[name]
    x_cpu, g_cpu = S.inputs(n)
    x, x_whole = _buf(n, off, x_cpu)
    g, g_whole = _buf(n, off, g_cpu)
    dx, dx_whole = (x, x_whole) if alias else _buf(n, off)
    L.silu_backward(x, g, dx)
    torch.cuda.synchronize()
    assert _guards_intact(dx_whole, off, n), "backward wrote past dx"
    assert _same_bits(g, g_cpu) and _guards_intact(g_whole, off, n), "g was written"
    if not alias:
        assert _same_bits(x, x_cpu) and _guards_intact(x_whole, off, n), "x was written"
    return dx.cpu()


@pytest.mark.parametrize("name", list(CASES))
def test_backward(name):
    """dx of its own and dx = x (the in-place node) give the same bits, inside the bounds; so does a
    second run"""
    n = CASES[name][0]
    dx = _backward(name, False)
    print(name, "backward worst d/bound", _check("dx", n, dx))
    assert torch.isfinite(dx.float()).all()
    assert torch.equal(S.bits(_backward(name, True)), S.bits(dx)), "dx = x gives other bits"
    assert torch.equal(S.bits(_backward(name, False)), S.bits(dx))
    db, gb = S.bits(dx), S.bits(S.inputs(n)[1])
    for base in _planted_places(n):
        for j in (13, 15, 17):                               # x = 2^8, 88, 100: dx = g, the same bits (1, or -0.0 in the tail)
            assert db[base + j] == gb[base + j]
        assert dx[base + 12] == 0 and dx[base + 16] == 0     # x = -2^8, -100: a zero


def test_launchers_reject_bad_arguments():
    """x = g = 1 and an output of its own filled with FILL = 3: forward (0.73) and backward (0.93) would
    change the output, so a launch behind a non-zero return shows"""
    k = native.kernels()
    x = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    out = torch.full((64,), FILL, dtype=torch.bfloat16, device=DEV)
    px, pg, po = x.data_ptr(), g.data_ptr(), out.data_ptr()
    assert k.cxn_silu_fwd(None, po, 64, None) != 0
    assert k.cxn_silu_fwd(px, None, 64, None) != 0
    assert k.cxn_silu_fwd(px, po, 0, None) != 0
    assert k.cxn_silu_fwd(px, po, -8, None) != 0
    assert k.cxn_silu_bwd(None, pg, po, 64, None) != 0
    assert k.cxn_silu_bwd(px, None, po, 64, None) != 0
    assert k.cxn_silu_bwd(px, pg, None, 64, None) != 0
    assert k.cxn_silu_bwd(px, pg, po, 0, None) != 0
    assert k.cxn_silu_bwd(px, pg, po, -8, None) != 0
    torch.cuda.synchronize()
    assert (out == FILL).all() and (x == 1).all() and (g == 1).all()
    with pytest.raises(ValueError, match="bf16"):
        L.silu_forward(x.float(), torch.empty(64, device=DEV))
    with pytest.raises(ValueError, match="alias"):
        L.silu_forward(x, x)
    with pytest.raises(ValueError, match="alias"):
        L.silu_backward(x, g, g)
    with pytest.raises(ValueError, match="size"):
        L.silu_forward(x, out[:32])
    torch.cuda.synchronize()
    assert (out == FILL).all() and (x == 1).all() and (g == 1).all()
    assert k.cxn_silu_fwd(px, po, 64, None) == 0  # and the same call with good arguments does write
    torch.cuda.synchronize()
    assert (out != FILL).all()


def test_a_layer_sized_for_batch_3_runs_at_batch_2():
    """A smaller current batch (nodes sliced to their first rows, as the executor does) gives those
    rows' results and leaves the third row of every node untouched."""
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    C, Hh, W = 5, 3, 4  # 60 elements per row: 120 at batch 2
    n = 2 * C * Hh * W
    x_cpu, g_cpu = S.inputs(n)
    x, o = Node("x"), Node("o")
    x.set_shape(3, C, Hh, W)
    lay = create_layer(47, LayerContext(torch.device(DEV)))
    lay.init_connection([x], [o])
    full = {}
    for nd in (x, o):
        nd.alloc(DEV, torch.bfloat16)
        nd.data.fill_(FILL)
        full[nd.name] = nd.data
        nd.data = nd.data[:2]
    x.data.copy_(x_cpu.view(x.data.shape))
    lay.forward(True, [x], [o])
    S.assert_within(o.data.reshape(-1), *S.forward_ref(x_cpu), "y at batch 2", axes="i")
    o.data.copy_(g_cpu.view(o.data.shape))
    lay.backprop(True, [x], [o])
    torch.cuda.synchronize()
    S.assert_within(x.data.reshape(-1), *S.backward_ref(x_cpu, g_cpu), "dx at batch 2", axes="i")
    assert _same_bits(o.data.reshape(-1), g_cpu)
    for nd in (x, o):
        assert (full[nd.name][2:] == FILL).all()
