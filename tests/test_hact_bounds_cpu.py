"""The bounds of tests/hact_bounds.py hold for a correct fp32 computation in every evaluation order,
see a planted error, and their float64 references are torch's relu6 / hardsigmoid / hardswish and
their autograd.  CPU only."""
import pytest
import torch
import torch.nn.functional as F

import hact_bounds as H

SIZES = (1, 7, 8, 40, 8 * 256 + 5)
TORCH_FN = {"relu6": F.relu6, "hsigmoid": F.hardsigmoid, "hswish": F.hardswish}


def test_the_planted_values_are_there():
    px = H.planted_x()
    for v in (0.0, 3.0, -3.0, 6.0, -1.5, 2.0 ** 8, 2.0 ** -8,
              -3.015625, -2.984375, 2.984375, 3.015625, 5.96875, 6.03125, -2.0 ** -133, 2.0 ** -133,
              -2.0 ** -125, 2.0 ** -125):
        assert v in px, v
    assert len(px) == 18 and px[9:11] == [-2.0 ** -133, 2.0 ** -133]
    x, g = H.inputs(8 * 256 + 5)
    assert torch.equal(x[:18].double(), torch.tensor(px, dtype=torch.float64))
    assert H.bits(x)[9] == -32767 and H.bits(x)[10] == 1                   # the smallest subnormals, kept by bf16
    assert H.bits(x)[0] == -32768 and H.bits(x)[1] == 0                  # -0.0, then +0.0
    assert H.bits(g)[0] == -32768 and g[1] == 1.0                          # -0.0 and 1 in g
    assert torch.equal(x[-18:].double(), torch.tensor(px, dtype=torch.float64))   # and in the tail run
    assert g[-18] == 1.0 and H.bits(g)[-17] == -32768                      # each x meets the other g there
    for kind in H.KINDS:  # every piece of every kind is hit by the random part too
        lo, hi = H.LO_HI[kind]
        xr = x[18:-18].double()
        assert (xr <= lo).any() and (xr >= hi).any() and ((xr > lo) & (xr < hi)).any()
    assert H.inputs(1)[0].numel() == 1 and H.bits(H.inputs(1)[0])[0] == -32768


def test_the_subnormal_neighbours_of_zero():
    """x = +-2^-133: relu6 keeps the bits of the positive one (forward and, for g, backward), and only
    the hswish forward, whose result 2^-134 lies between two stored values, has the subnormal term"""
    x = torch.tensor([-2.0 ** -133, 2.0 ** -133], dtype=torch.bfloat16)
    g = torch.tensor([1.0, 1.0], dtype=torch.bfloat16)
    assert H.bits(x).tolist() == [-32767, 1]
    for order in H.ORDERS:
        assert H.bits(H.emulate_forward("relu6", x, order)).tolist() == [0, 1]
        assert H.bits(H.emulate_backward("relu6", x, g, order)).tolist() == [0, H.bits(g)[1]]
    assert H.ref_bits(H.forward_ref("relu6", x)[0]).tolist() == [0, 1]
    for kind in H.KINDS:
        fb, bb = H.forward_ref(kind, x)[1], H.backward_ref(kind, x, g)[1]
        if kind == "hswish":
            assert (fb >= H.BF16_HALF_SUBNORMAL).all() and (fb < 1.01 * H.BF16_HALF_SUBNORMAL).all()
        else:
            assert (fb == 0).all() if kind == "relu6" else (fb <= 1.01 * H.U_BF16 * 0.5).all()  # u hsigmoid(0)
        assert (bb <= 1.01 * H.U_BF16 * 0.5).all()  # no backward has the term: |dx| <= |g| / 2 there
    n = 8 * 256 + 5
    fb = H.case_ref("hswish", n)["y"][1]
    assert int((fb - H.U_BF16 * H.case_ref("hswish", n)["y"][0].abs() >= H.BF16_HALF_SUBNORMAL).sum()) >= 4
    xs = H.inputs(n)[0].double()
    ref = H.case_ref("hswish", n)["y"][0]
    sub = (ref != 0) & (ref.abs() < H.BF16_MIN_NORMAL)
    assert int(sub.sum()) == 4 and (xs[sub].abs() == 2.0 ** -133).all()   # the term touches those elements alone


def test_the_table_at_the_breakpoints():
    """strictly inside: a breakpoint belongs to the outer piece, forward and backward"""
    x = torch.tensor([-3.0, 0.0, -0.0, 3.0, 6.0], dtype=torch.bfloat16)
    g = torch.ones(5, dtype=torch.bfloat16)
    want = {"relu6": ([0, 0, 0, 3, 6], [0, 0, 0, 1, 0]),
            "hsigmoid": ([0, 0.5, 0.5, 1, 1], [0, 1 / 6, 1 / 6, 0, 0]),
            "hswish": ([0, 0, 0, 3, 6], [0, 0.5, 0.5, 1, 1])}
    for kind, (y, dx) in want.items():
        ref, bound = H.forward_ref(kind, x)
        assert torch.equal(ref, torch.tensor(y, dtype=torch.float64)), kind
        assert (bound[[0, 3, 4]] == 0).all(), kind
        ref, bound = H.backward_ref(kind, x, g)
        assert torch.equal(ref, torch.tensor(dx, dtype=torch.float64)), kind
        assert (bound[[0, 3, 4]] == 0).all(), kind
    assert H.ref_bits(H.forward_ref("relu6", x)[0])[2] == 0      # relu6(-0.0) = +0
    assert H.backward_ref("hswish", torch.tensor([-1.5], dtype=torch.bfloat16), g[:1])[0][0] == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", H.KINDS)
def test_emulations_stay_inside_the_bounds(kind, n):
    x, g = H.inputs(n)
    refs = H.case_ref(kind, n)
    for order in H.ORDERS:
        y = H.emulate_forward(kind, x, order)
        dx = H.emulate_backward(kind, x, g, order)
        H.assert_within(y, *refs["y"], "%s y %s" % (kind, order), axes="i")
        H.assert_within(dx, *refs["dx"], "%s dx %s" % (kind, order), axes="i")
        if kind == "relu6":  # exact: the same bits, the sign of a zero included
            assert torch.equal(H.bits(y), H.ref_bits(refs["y"][0]))
            assert torch.equal(H.bits(dx), H.ref_bits(refs["dx"][0]))
        lo, hi = H.LO_HI[kind]
        outside = ~((x.double() > lo) & (x.double() < hi))
        assert (refs["y"][1][outside] == 0).all() and (refs["dx"][1][outside] == 0).all()


@pytest.mark.parametrize("kind", ["hsigmoid", "hswish"])
def test_two_ulps_on_one_element_are_caught(kind):
    """wherever u |ref| dominates the bound (everywhere but next to a zero of the reference), a stored
    value two bf16 ulps off is outside it; the unbumped emulation is inside"""
    n = 8 * 256 + 5
    x, g = H.inputs(n)
    for key, good in (("y", H.emulate_forward(kind, x, "sum_mul")), ("dx", H.emulate_backward(kind, x, g, "sum_mul"))):
        ref, bound = H.case_ref(kind, n)[key]
        assert H.violations(good, ref, bound)[0] == 0
        dominated = (bound > 0) & (H.U_BF16 * ref.abs() >= 0.99 * bound)
        assert dominated.sum() > n // 4, (kind, key)
        for i in torch.nonzero(dominated).reshape(-1)[::37].tolist() + [int(ref.abs().argmax())]:
            cnt, _, bad = H.violations(H.bump_ulps(good, i), ref, bound)
            assert cnt == 1 and int(bad[0]) == i, (kind, key, i)


def test_one_wrong_bit_of_relu6_is_caught():
    n = 40
    x, g = H.inputs(n)
    for key, good in (("y", H.emulate_forward("relu6", x, "fma")), ("dx", H.emulate_backward("relu6", x, g, "fma"))):
        ref, bound = H.case_ref("relu6", n)[key]
        assert (bound == 0).all()
        i = int(ref.abs().argmax())
        assert H.violations(H.bump_ulps(good, i, 1), ref, bound)[0] == 1


@pytest.mark.parametrize("kind", H.KINDS)
def test_references_are_torchs_functions_and_autograd(kind):
    """float64 torch: 1e-6 relative (torch multiplies by an fp32 1/6 there, so not bit for bit), at
    the planted breakpoints too -- the "strictly inside" convention is torch's"""
    x, g = H.inputs(8 * 256 + 5)
    xa = x.double().requires_grad_()
    y = TORCH_FN[kind](xa)
    y.backward(g.double())
    ref_y = H.forward_ref(kind, x)[0]
    ref_dx = H.backward_ref(kind, x, g)[0]
    assert ((y.detach() - ref_y).abs() <= 1e-6 * ref_y.abs()).all()
    assert ((xa.grad - ref_dx).abs() <= 1e-6 * ref_dx.abs()).all()
    brk = torch.tensor([-3.0, -0.0, 0.0, 3.0, 6.0], dtype=torch.float64, requires_grad=True)
    yb = TORCH_FN[kind](brk)
    yb.backward(torch.ones(5, dtype=torch.float64))
    xb = brk.detach().to(torch.bfloat16)
    assert torch.allclose(yb.detach(), H.forward_ref(kind, xb)[0], rtol=1e-6, atol=0)
    assert torch.allclose(brk.grad, H.backward_ref(kind, xb, torch.ones(5, dtype=torch.bfloat16))[0], rtol=1e-6, atol=0)
