"""The bounds of tests/silu_bounds.py hold for a correct fp32 computation in two evaluation orders, see
a planted error, and their float64 references are torch's silu and its autograd; the `silu` layer
(type id 47) on the CPU executor; the type names and ids of `silu` and `drop_path`.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import silu_bounds as S

SIZES = (1, 7, 8, 40, 8 * 256 + 5)
NP = len(S.PLANTED_X)


def _fresh():
    from cxxnet_amd.layers import LayerContext, create_layer
    return create_layer(47, LayerContext(torch.device("cpu")))


def _nodes(*shapes):
    from cxxnet_amd.layers import Node
    out = []
    for i, s in enumerate(shapes):
        n = Node("n%d" % i)
        n.set_shape(*s)
        out.append(n)
    return out


def test_the_planted_values_are_there():
    px = S.planted_x()
    for v in (0.0, -2.0 ** -133, 2.0 ** -133, -2.0 ** -125, 2.0 ** -125, -1.28125, -1.2734375, -8.0, 8.0, -16.0, 16.0,
              2.0 ** 8, -2.0 ** 8, -88.0, 88.0, -100.0, 100.0):
        assert v in px, v
    assert NP == 18 and -1.28125 < S.SILU_GRAD_ZERO < -1.2734375
    lo, hi = torch.tensor([-1.28125, -1.2734375], dtype=torch.bfloat16)
    assert S.bits(lo.view(1))[0] - S.bits(hi.view(1))[0] == 1   # adjacent bf16 numbers around the zero of silu'
    x, g = S.inputs(8 * 256 + 5)
    assert torch.equal(x[:NP].double(), torch.tensor(px, dtype=torch.float64))     # every planted value is a bf16 number
    assert S.bits(x)[0] == -32768 and S.bits(x)[1] == 0                           # -0.0, then +0.0
    assert S.bits(x)[2:4].tolist() == [-32767, 1]                                 # the smallest subnormals, kept by bf16
    assert S.bits(g)[0] == -32768 and g[1] == 1.0                                 # -0.0 and 1 in g
    assert torch.equal(x[-NP:].double(), torch.tensor(px, dtype=torch.float64))   # and in the tail run
    assert g[-NP] == 1.0 and S.bits(g)[-NP + 1] == -32768                         # each x meets the other g there
    xr = x[NP:-NP].double()
    assert xr.min() < -15 and xr.max() > 15 and xr.abs().max() <= 16
    assert S.inputs(1)[0].numel() == 1 and S.bits(S.inputs(1)[0])[0] == -32768
    # silu' changes sign between the two neighbours and is about 1e-3 at both: the absolute term, nothing
    # next to u |ref| elsewhere, is more than half of u |ref| here (and all of the bound at the zero itself)
    ref, bound = S.backward_ref(torch.stack([lo, hi]), torch.ones(2, dtype=torch.bfloat16))
    assert ref[0] < 0 < ref[1] and ref.abs().max() < 2e-3
    assert (bound > 1.5 * S.U_BF16 * ref.abs()).all()


def test_the_ends_and_the_subnormals():
    """x = -100 and -2^8: e^-x overflows fp32, y = -0 and dx a zero; x = 88, 100, 2^8: sigma = 1, y = x and
    dx = g with the same bits; x = +-2^-133: y = x / 2 lies between two stored values, and only the forward
    bound has the subnormal term.  In every order."""
    x = torch.tensor([-100.0, -256.0, 88.0, 100.0, 256.0, -2.0 ** -133, 2.0 ** -133], dtype=torch.bfloat16)
    g = torch.tensor([1.0, -1.0, 0.5, -0.0, 3.0, 1.0, 1.0], dtype=torch.bfloat16)
    for order in S.ORDERS:
        y, dx = S.emulate_forward(x, order), S.emulate_backward(x, g, order)
        assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
        assert S.bits(y)[:2].tolist() == [-32768, -32768]                 # -0
        assert (dx[:2] == 0).all()
        assert torch.equal(S.bits(y)[2:5], S.bits(x)[2:5])
        assert torch.equal(S.bits(dx)[2:5], S.bits(g)[2:5])               # -0.0 among them
        S.assert_within(y, *S.forward_ref(x), "ends y " + order, axes="i")
        S.assert_within(dx, *S.backward_ref(x, g), "ends dx " + order, axes="i")
    ref, fb = S.forward_ref(x)
    assert (ref[:2] < 0).all() and (ref[:2].abs() < 2.0 ** -133).all()   # float64 keeps the tiny negative value
    assert (fb[5:] >= S.BF16_HALF_SUBNORMAL).all() and (fb[5:] < 1.01 * S.BF16_HALF_SUBNORMAL).all()
    assert (fb[2:5] <= 1.05 * S.U_BF16 * ref[2:5].abs()).all()            # no such term at the positive end
    # x = -88: s = 6e-39 is an fp32 subnormal; ref = -5e-37 is a normal bf16 number, and both it and a zero are inside
    x88 = torch.tensor([-88.0], dtype=torch.bfloat16)
    ref, b = S.forward_ref(x88)
    assert ref.abs() > S.BF16_MIN_NORMAL and b >= ref.abs()
    for got in (ref.to(torch.bfloat16), torch.tensor([-0.0], dtype=torch.bfloat16)):
        assert S.violations(got, ref, b)[0] == 0
    assert S.violations(-ref.to(torch.bfloat16), ref, b)[0] == 1          # but not the value of the other sign


@pytest.mark.parametrize("n", SIZES)
def test_emulations_stay_inside_the_bounds(n):
    x, g = S.inputs(n)
    refs = S.case_ref(n)
    for order in S.ORDERS:
        worst_y = S.assert_within(S.emulate_forward(x, order), *refs["y"], "y " + order, axes="i")
        worst_dx = S.assert_within(S.emulate_backward(x, g, order), *refs["dx"], "dx " + order, axes="i")
        print(n, order, "worst d/bound", worst_y, worst_dx)


def test_two_ulps_on_one_element_are_caught():
    """wherever u |ref| is the bound (everywhere but next to a zero of the reference and at the far negative
    end), a stored value two bf16 ulps off is outside it; the unbumped emulation is inside"""
    n = 8 * 256 + 5
    x, g = S.inputs(n)
    for key, good in (("y", S.emulate_forward(x, "recip")), ("dx", S.emulate_backward(x, g, "recip"))):
        ref, bound = S.case_ref(n)[key]
        assert S.violations(good, ref, bound)[0] == 0
        dominated = (bound > 0) & (S.U_BF16 * ref.abs() >= 0.99 * bound)
        assert dominated.sum() > n // 4, key
        for i in torch.nonzero(dominated).reshape(-1)[::37].tolist():
            cnt, _, bad = S.violations(S.bump_ulps(good, i), ref, bound)
            assert cnt == 1 and int(bad[0]) == i, (key, i)


def test_a_raw_sign_or_finiteness_error_at_the_ends_is_caught():
    """e / (1 + e) formulations give NaN (inf / inf) at x = -100; y = +x, +0 where -0 is due (by the bits),
    inf and NaN at +-100 are all outside"""
    x = torch.tensor([-100.0, 100.0], dtype=torch.bfloat16)
    g = torch.ones(2, dtype=torch.bfloat16)
    v = x.float()
    e = torch.exp(-v)
    naive = (v * (1.0 - e / (1.0 + e))).to(torch.bfloat16)   # 1 - e / (1 + e): inf / inf at x = -100
    ref, bound = S.forward_ref(x)
    cnt, _, bad = S.violations(naive, ref, bound)
    assert cnt == 1 and int(bad[0]) == 0 and torch.isnan(naive[0])
    for wrong in ([100.0, 100.0], [-100.0, 100.0], [-0.0, -100.0], [float("inf"), 100.0], [-0.0, float("nan")],
                  [-0.0, float("inf")]):
        assert S.violations(torch.tensor(wrong, dtype=torch.bfloat16), ref, bound)[0] == 1, wrong
    good = S.emulate_forward(x, "recip")
    assert S.violations(good, ref, bound)[0] == 0 and S.bits(good).tolist() == [-32768, S.bits(x)[1]]
    ref, bound = S.backward_ref(x, g)
    for wrong in ([1.0, 1.0], [0.0, -1.0], [0.0, 0.0], [float("nan"), 1.0], [0.0, float("inf")]):
        assert S.violations(torch.tensor(wrong, dtype=torch.bfloat16), ref, bound)[0] == 1, wrong
    assert S.violations(S.emulate_backward(x, g, "quot"), ref, bound)[0] == 0


def test_references_are_torchs_silu_and_autograd():
    x, g = S.inputs(8 * 256 + 5)
    xa = x.double().requires_grad_()
    y = F.silu(xa)
    y.backward(g.double())
    ref_y, ref_dx = S.forward_ref(x)[0], S.backward_ref(x, g)[0]
    assert ((y.detach() - ref_y).abs() <= 1e-12 * ref_y.abs() + 1e-300).all()
    assert ((xa.grad - ref_dx).abs() <= 1e-12 * g.double().abs() * (1 + x.double().abs())).all()


# ------------------------------------------------------------------ the layer on the CPU executor
@pytest.mark.parametrize("alias", [True, False])
def test_the_layer_matches_the_float64_references(alias):
    """fp32 nodes: the only error is the formulas' fp32 arithmetic, the eps32 part of the bounds plus one
    eps32 |ref|.  alias: dx overwrites x (the usual in-place node), else it goes to a private buffer."""
    n = 2 * 3 * 4 * 5
    xb, gb = S.inputs(n)
    x, o = _nodes((2, 3, 4, 5), (0, 0, 0, 0))
    lay = _fresh()
    lay.init_connection([x], [o])
    assert o.shape == (2, 3, 4, 5) and lay.params == []
    for nd in (x, o):
        nd.alloc("cpu", torch.float32)
    x.data.copy_(xb.float().view(x.data.shape))
    if not alias:
        x.grad_buf = torch.full_like(x.data, 9.0)
    ys = []
    for is_train in (True, False):
        lay.forward(is_train, [x], [o])
        ys.append(o.data.clone())
    assert torch.equal(ys[0], ys[1])
    assert torch.equal(x.data.view(-1), xb.float())  # forward only reads x

    def fp32_bound(ref, bound):
        return bound - S.U_BF16 * ref.abs() + S.EPS_F32 * ref.abs()

    ref, bound = S.forward_ref(xb)
    S.assert_within(ys[0].view(-1), ref, fp32_bound(ref, bound), "y", axes="i")
    o.data.copy_(gb.float().view(o.data.shape))  # the output node now holds the gradient
    lay.backprop(False, [x], [o])  # prop_grad = False writes nothing
    assert torch.equal(x.data.view(-1), xb.float())
    lay.backprop(True, [x], [o])
    ref, bound = S.backward_ref(xb, gb)
    S.assert_within(x.gdst.view(-1), ref, fp32_bound(ref, bound), "dx", axes="i")
    assert torch.equal(o.data.view(-1), gb.float())  # g is only read
    if not alias:
        assert torch.equal(x.data.view(-1), xb.float())


def test_connection_checks():
    from cxxnet_amd.layers import Node
    x, x2 = _nodes((2, 3, 4, 5), (2, 3, 4, 5))
    o, o2 = Node("o"), Node("o2")
    for nin, nout in [([x, x2], [o]), ([x], [o, o2]), ([], [o]), ([x], [])]:
        with pytest.raises(ValueError, match="SiluLayer"):
            _fresh().init_connection(nin, nout)
    with pytest.raises(ValueError, match="SiluLayer: silu reads its input again in backward.*self-loop"):
        _fresh().init_connection([x], [x])
    (p,) = _nodes((2, 3, 4, 5))
    p.cp = 4
    with pytest.raises(ValueError, match="padded-channel"):
        _fresh().init_connection([p], [o])
    for shape in ((2, 3, 4, 5), (2, 1, 1, 7), (2, 6, 1, 1)):
        (n,) = _nodes(shape)
        o = Node("o")
        _fresh().init_connection([n], [o])
        assert o.shape == shape and o.cp == shape[1]


def test_ops_reject_aliases_and_other_sizes():
    from cxxnet_amd.ops import layer_ops as L
    x, g = torch.zeros(2, 3), torch.ones(2, 3)
    with pytest.raises(ValueError, match="silu"):
        L.silu_forward(x, torch.zeros(2, 4))
    with pytest.raises(ValueError, match="silu"):
        L.silu_backward(x, torch.zeros(2, 4), x)
    with pytest.raises(ValueError, match="alias"):
        L.silu_forward(x, x)
    with pytest.raises(ValueError, match="alias"):
        L.silu_backward(x, g, g)
    L.silu_backward(x, g, x)  # dx = x is the in-place gradient
    assert (x == 0.5).all()


def test_type_names_and_ids_round_trip():
    from cxxnet_amd import native
    from cxxnet_amd.layers import LayerContext, create_layer
    from cxxnet_amd.nnet import neural_net
    for name, tid, cls in (("silu", 47, "SiluLayer"), ("drop_path", 48, "DropPathLayer")):
        assert native.rt().get_layer_type(name) == tid
        assert native.rt().get_layer_type("pairtest-%s-%s" % (name, name)) == 1024 * tid + tid
        assert tid < 1024 and tid not in neural_net._SPLIT_SAFE
        lay = create_layer(tid, LayerContext(torch.device("cpu")))
        assert type(lay).__name__ == cls and lay.type_name == name and lay.type_id == tid
        assert type(lay).__dict__["replay_audited"] is False
        lay.set_param("add_relu", "1")  # another layer's key: ignored
        lay.set_param("threshold", "0.5")  # dropout's key: not drop_path's
        assert lay.params == []
    assert create_layer(48, LayerContext(torch.device("cpu"))).drop_prob == 0.0
    assert neural_net.K_DROP_PATH == 48
