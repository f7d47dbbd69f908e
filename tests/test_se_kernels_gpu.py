"""Squeeze-and-excitation kernels (csrc/kernels/se_kernels.hip): `ch_scale` forward, backward and the
global sum / avg pooling, per element against the float64 bounds of tests/se_bounds.py, with sentinel
guards around every output and the workspace, for every aliasing the layer can meet.  The cases are
the smallest at which the kernels can go wrong (se_bounds.CASES): one pixel; fewer pixels than pixel
lanes; several channel groups; a group count that leaves a thread idle; the scalar path by C % 8 and
by alignment; and maps cut into parts (fp32 partials and the merge launch) on both paths."""
import pytest
import torch

import se_bounds as S
from cxxnet_amd import native, ops
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24  # elements after (and `off` before) each buffer that must stay untouched
FILL = 3.0
WS_FILL = -7.0


def _buf(shape, off, src=None):
    """A device bf16 buffer of off + n + GUARD elements filled with FILL; the view of its n elements
    from element `off` in `shape` (holding src) and the whole buffer."""
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((off + n + GUARD,), FILL, dtype=torch.bfloat16, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[off:off + n].view(shape)
    if src is not None:
        view.copy_(src.reshape(shape))
    return view, whole


def _guards_intact(whole, off, n):
    w = whole.cpu()
    return bool((w[:off] == FILL).all() and (w[off + n:] == FILL).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _state(B, HW, C):
    """(state with its workspace inside a guarded buffer, that buffer, the workspace's size)"""
    st = L.ChScaleState(B, HW, C, DEV, True)
    parts = L.se_parts(B, HW, C)
    if parts == 1:
        assert st.ws is None
        return st, None, 0
    n = st.ws.numel()
    assert st.ws.dtype == torch.float32 and n >= parts * B * C
    whole = torch.full((n + GUARD,), WS_FILL, dtype=torch.float32, device=DEV)
    st.ws = whole[:n]
    return st, whole, n


def _gate_shape(gate, B, C):
    return (B, 1, C, 1) if gate == "mat" else (B, 1, 1, C)  # the buffers of nodes (B,1,1,C) and (B,C,1,1)


def test_part_counts():
    for name, ((B, H, W, C), _) in S.CASES.items():
        parts = L.se_parts(B, H * W, C)
        assert (parts > 1) is (name in S.MULTI), (name, parts)
    # 8 pixels per pixel lane at least: 3136 / (8 * 128 lanes) and 3136 / (8 * 32 lanes)
    assert L.se_parts(2, 56 * 56, 16) == 3 and L.se_parts(64, 7 * 7, 512) == 1 and L.se_parts(64, 56 * 56, 64) == 12
    k = native.kernels()
    assert k.cxn_se_ws_floats(2, 56 * 56, 16) == 3 * 2 * 16 and k.cxn_se_ws_floats(64, 49, 512) == 0


@pytest.mark.parametrize("gate", ["mat", "ch"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_forward(name, gate):
    (B, H, W, C), off = S.CASES[name]
    x_cpu, s_cpu, _ = S.inputs(name)
    ref, bound = S.case_ref(name)["y"]
    x, x_whole = _buf((B, H, W, C), off, x_cpu)
    s, s_whole = _buf(_gate_shape(gate, B, C), off, s_cpu)
    y, y_whole = _buf((B, H, W, C), off)
    L.ch_scale_forward(x, s, y)
    S.assert_within(y, ref, bound, name + " y")
    n = x.numel()
    assert _guards_intact(y_whole, off, n), "forward wrote past y"
    assert torch.equal(_bits(x), _bits(x_cpu)) and _guards_intact(x_whole, off, n), "x was written"
    assert torch.equal(_bits(s).reshape(B, C), _bits(s_cpu)) and _guards_intact(s_whole, off, B * C), "s was written"
    yb = _bits(y)
    assert yb[0, 0, 0, 1] == -32768                       # -0.0 * 1
    assert (y[..., 0] == 0).all()                         # s = 0 exactly
    assert torch.equal(yb[..., 1], _bits(x_cpu)[..., 1])  # s = 1 exactly: the same bits
    y2, _ = _buf((B, H, W, C), off)
    L.ch_scale_forward(x, s, y2)
    assert torch.equal(_bits(y2), yb)


def _backward(name, gate, alias_dx, alias_ds):
    (B, H, W, C), off = S.CASES[name]
    x_cpu, s_cpu, g_cpu = S.inputs(name)
    n = x_cpu.numel()
    g, g_whole = _buf((B, H, W, C), off, g_cpu)
    x, x_whole = _buf((B, H, W, C), off, x_cpu)
    s, s_whole = _buf(_gate_shape(gate, B, C), off, s_cpu)
    dx, dx_whole = (x, x_whole) if alias_dx else _buf((B, H, W, C), off)
    ds, ds_whole = (s, s_whole) if alias_ds else _buf(_gate_shape(gate, B, C), off)
    st, ws_whole, ws_n = _state(B, H * W, C)
    L.ch_scale_backward(g, x, s, dx, ds, st)
    torch.cuda.synchronize()
    assert _guards_intact(dx_whole, off, n), "backward wrote past dx"
    assert _guards_intact(ds_whole, off, B * C), "backward wrote past ds"
    assert torch.equal(_bits(g), _bits(g_cpu)) and _guards_intact(g_whole, off, n), "g was written"
    if not alias_dx:
        assert torch.equal(_bits(x), _bits(x_cpu)) and _guards_intact(x_whole, off, n), "x was written"
    if not alias_ds:
        assert torch.equal(_bits(s).reshape(B, C), _bits(s_cpu)) and _guards_intact(s_whole, off, B * C), "s was written"
    if ws_whole is not None:
        assert (ws_whole.cpu()[ws_n:] == WS_FILL).all(), "backward wrote past the workspace"
    return dx.detach().cpu().clone(), ds.detach().cpu().reshape(B, C).clone()


@pytest.mark.parametrize("alias_ds", [False, True])
@pytest.mark.parametrize("alias_dx", [False, True])
@pytest.mark.parametrize("gate", ["mat", "ch"])
@pytest.mark.parametrize("name", list(S.CASES))
def test_backward(name, gate, alias_dx, alias_ds):
    refs = S.case_ref(name)
    dx, ds = _backward(name, gate, alias_dx, alias_ds)
    what = "%s %s dx%s ds%s" % (name, gate, "=x" if alias_dx else "", "=s" if alias_ds else "")
    S.assert_within(dx, *refs["dx"], what + " dx")
    S.assert_within(ds, *refs["ds"], what + " ds", axes="bc")
    assert (dx[..., 0] == 0).all()  # s = 0 exactly
    assert torch.equal(_bits(dx)[..., 1], _bits(S.inputs(name)[2])[..., 1])  # s = 1 exactly
    dx2, ds2 = _backward(name, gate, alias_dx, alias_ds)  # a second run: the same bits
    assert torch.equal(_bits(dx2), _bits(dx)) and torch.equal(_bits(ds2), _bits(ds))


def test_every_aliasing_gives_the_same_bits():
    for name in ("c64", "multi", "c3"):
        base = _backward(name, "mat", False, False)
        for gate, adx, ads in (("ch", False, False), ("mat", True, False), ("mat", False, True), ("ch", True, True)):
            got = _backward(name, gate, adx, ads)
            assert torch.equal(_bits(got[0]), _bits(base[0])) and torch.equal(_bits(got[1]), _bits(base[1]))


@pytest.mark.parametrize("name", ["c24", "multi"])
def test_a_layer_sized_for_batch_3_runs_at_batch_2(name):
    """The layer allocates its workspace once for the connection's batch; a smaller current batch
    (nodes sliced to their first rows, as the executor does) gives those rows' results."""
    from cxxnet_amd.layers import LayerContext, Node, create_layer
    (B, H, W, C), _ = S.CASES[name]
    x_cpu, s_cpu, g_cpu = S.inputs(name)
    x_cpu, s_cpu, g_cpu = x_cpu[:2], s_cpu[:2], g_cpu[:2]
    x, s, o = Node("x"), Node("s"), Node("o")
    x.set_shape(3, C, H, W)
    s.set_shape(3, 1, 1, C)
    lay = create_layer(42, LayerContext(torch.device(DEV)))
    lay.init_connection([x, s], [o])
    full = {}
    for n in (x, s, o):
        n.alloc(DEV, torch.bfloat16)
        n.data.fill_(FILL)
        full[n.name] = n.data
        n.data = n.data[:2]
    x.data.copy_(x_cpu)
    s.data.copy_(s_cpu.reshape(s.data.shape))
    lay.forward(True, [x, s], [o])
    S.assert_within(o.data, *S.scale_ref(x_cpu, s_cpu), name + " y at batch 2")
    o.data.copy_(g_cpu)
    lay.backprop(True, [x, s], [o])
    torch.cuda.synchronize()
    assert (lay._st.ws is not None) is (name == "multi")
    S.assert_within(x.data, *S.scale_ref(g_cpu, s_cpu), name + " dx at batch 2")
    S.assert_within(s.data.reshape(2, C), *S.ds_ref(g_cpu, x_cpu), name + " ds at batch 2", axes="bc")
    for n in (x, s, o):  # the third row of every node was not touched
        assert (full[n.name][2:] == FILL).all()


def test_launchers_reject_bad_arguments():
    k = native.kernels()
    t = torch.zeros(2 * 56 * 56 * 16, dtype=torch.bfloat16, device=DEV)
    p = t.data_ptr()
    assert k.cxn_ch_scale_fwd(p, p, None, 1, 4, 8, None) != 0
    assert k.cxn_ch_scale_fwd(p, p, p, 0, 4, 8, None) != 0
    assert k.cxn_ch_scale_fwd(p, p, p, 70000, 1, 8, None) != 0
    assert k.cxn_ch_scale_bwd(p, p, p, p, None, None, 0, 1, 4, 8, None) != 0
    assert k.cxn_ch_scale_bwd(p, p, p, p, p, None, 0, 2, 56 * 56, 16, None) != 0   # parts without a workspace
    ws = torch.zeros(64, dtype=torch.float32, device=DEV)
    assert k.cxn_ch_scale_bwd(p, p, p, p, p, ws.data_ptr(), 64, 2, 56 * 56, 16, None) != 0   # too small a one
    assert k.cxn_global_pool_fwd(p, p, ws.data_ptr(), 64, 2, 56 * 56, 16, 1.0, None) != 0
    assert k.cxn_se_parts(0, 4, 8) < 0 and k.cxn_se_ws_floats(2, 0, 8) < 0
    torch.cuda.synchronize()
    assert (t == 0).all() and (ws == 0).all()


# ------------------------------------------------------------------ global pooling
def _pool(name, mode, x_cpu=None):
    B, H, W, C = S.POOL_CASES[name]
    x_cpu = S.inputs(name)[0] if x_cpu is None else x_cpu
    assert ops.pool_global_native(mode, H, W, C, H, W, 0, 1, 1)
    x, x_whole = _buf((B, H, W, C), 0, x_cpu)
    y, y_whole = _buf((B, 1, 1, C), 0)
    ops.pool_forward(x, y, None, H, W, 1, 0, mode)
    torch.cuda.synchronize()
    assert _guards_intact(y_whole, 0, B * C), "pooling wrote past y"
    assert torch.equal(_bits(x), _bits(x_cpu)) and _guards_intact(x_whole, 0, x.numel()), "x was written"
    return y.detach().cpu().reshape(B, C).clone()


@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("name", list(S.POOL_CASES))
def test_global_pool(name, mode):
    B, H, W, C = S.POOL_CASES[name]
    assert (L.se_parts(B, H * W, C) > 1) is (name == "p56")
    y = _pool(name, mode)
    S.assert_within(y, *S.pool_case_ref(name, mode), "%s %s" % (name, mode), axes="bc")
    assert torch.equal(_bits(_pool(name, mode)), _bits(y))  # a second run: the same bits
    if mode == "avg":  # the avg of a constant map is the constant, exactly
        for c in (1.5, -0.3125):
            yc = _pool(name, mode, torch.full((B, H, W, C), c, dtype=torch.bfloat16))
            assert (yc == c).all(), (name, c)


@pytest.mark.parametrize("mode", ["sum", "avg"])
def test_global_pool_workspace_guards(mode):
    """The launcher with a workspace of its exact size inside a guarded buffer: nothing past it is
    written, and the result is that of ops.pool_forward."""
    B, H, W, C = S.POOL_CASES["p56"]
    x_cpu = S.inputs("p56")[0]
    k = native.kernels()
    n = int(k.cxn_se_ws_floats(B, H * W, C))
    assert n == L.se_parts(B, H * W, C) * B * C > 0
    whole = torch.full((n + GUARD,), WS_FILL, dtype=torch.float32, device=DEV)
    x = x_cpu.to(DEV)
    y, y_whole = _buf((B, 1, 1, C), 0)
    scale = 1.0 / (H * W) if mode == "avg" else 1.0
    from cxxnet_amd.ops.gemm import _stream
    native.check(k.cxn_global_pool_fwd(x.data_ptr(), y.data_ptr(), whole.data_ptr(), n, B, H * W, C, scale, _stream()),
                 "global_pool_fwd")
    torch.cuda.synchronize()
    assert (whole.cpu()[n:] == WS_FILL).all() and _guards_intact(y_whole, 0, B * C)
    assert torch.equal(_bits(y).reshape(B, C), _bits(_pool("p56", mode)))


def test_the_generic_kernel_keeps_its_shapes_and_agrees(monkeypatch):
    """A 7 x 7 global avg pooling is not routed (and gives what it gave); with the switch off a routed
    shape runs the generic kernel, whose result lies inside the same bound."""
    from cxxnet_amd.ops import nn
    assert not ops.pool_global_native("avg", 7, 7, 64, 7, 7, 0, 1, 1)
    name, mode = "p14", "avg"
    new = _pool(name, mode)
    monkeypatch.setattr(nn, "GLOBAL_POOL", False)
    old = _pool(name, mode)
    S.assert_within(old, *S.pool_case_ref(name, mode), "generic kernel", axes="bc")
    ref, bound = S.pool_case_ref(name, mode)
    assert ((new.double() - old.double()).abs() <= 2 * bound).all()
