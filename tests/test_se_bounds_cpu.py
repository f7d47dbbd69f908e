"""The bounds of tests/se_bounds.py hold for a correct fp32 computation in any summation order, see
a planted error, and the routing predicate of the global pooling kernel is pinned.  CPU only."""
import pytest
import torch

import se_bounds as S
from cxxnet_amd import ops


@pytest.mark.parametrize("name", list(S.CASES))
def test_emulation_stays_inside_the_bounds(name):
    x, s, g = S.inputs(name)
    refs = S.case_ref(name)
    S.assert_within(S.emulate_scale(x, s), *refs["y"], name + " y")
    S.assert_within(S.emulate_scale(g, s), *refs["dx"], name + " dx")
    for order in S.ORDERS:
        S.assert_within(S.emulate_ds(g, x, order), *refs["ds"], "%s ds %s" % (name, order), axes="bc")


@pytest.mark.parametrize("mode", ["sum", "avg"])
@pytest.mark.parametrize("name", list(S.POOL_CASES))
def test_pool_emulation_stays_inside_the_bounds(name, mode):
    x = S.inputs(name)[0]
    for order in S.ORDERS:
        S.assert_within(S.emulate_pool(x, mode, order), *S.pool_case_ref(name, mode), "%s %s %s" % (name, mode, order),
                        axes="bc")


def test_the_planted_values_are_there():
    for name, ((B, H, W, C), _) in S.CASES.items():
        x, s, g = S.inputs(name)
        assert (s[:, 0] == 0).all() and (s[:, 1] == 1).all()
        assert x.view(torch.int16)[0, 0, 0, 1] == -32768  # -0.0
        y = S.emulate_scale(x, s)
        assert y.view(torch.int16)[0, 0, 0, 1] == -32768 and (y[..., 0] == 0).all()
        assert torch.equal(y[..., 1].view(torch.int16), x[..., 1].view(torch.int16))  # s = 1: the same bits
        if H * W >= 2:
            ref, bound = S.case_ref(name)["ds"]
            assert ref[B - 1, C - 1] == 0 and bound[B - 1, C - 1] > 0  # the cancelling column
            xf = x.reshape(B, H * W, C)
            assert xf[0, 0, 2] == 2.0 ** 8 and xf[0, 1, 2] == 2.0 ** -8


@pytest.mark.parametrize("name", list(S.CASES))
def test_two_ulps_on_one_product_are_caught(name):
    x, s, g = S.inputs(name)
    for key, a in (("y", x), ("dx", g)):
        ref, bound = S.case_ref(name)[key]
        good = S.emulate_scale(a, s)
        i = int(ref.abs().reshape(-1).argmax())
        n, _, bad = S.violations(S.bump_ulps(good, i), ref, bound)
        assert n == 1 and int(bad[0]) == i, (name, key)
        assert S.violations(good, ref, bound)[0] == 0


@pytest.mark.parametrize("name", [n for n, (sh, _) in S.CASES.items() if sh[1] * sh[2] <= 196])
def test_two_ulps_on_one_sum_are_caught(name):
    """Up to N = 196 terms the rounding term u |ref| dominates the bound of a sum at its largest element."""
    x, s, g = S.inputs(name)
    ref, bound = S.case_ref(name)["ds"]
    good = S.emulate_ds(g, x, "forward")
    i = int((ref.abs() / bound).reshape(-1).argmax())
    n, _, bad = S.violations(S.bump_ulps(good, i), ref, bound)
    assert n == 1 and int(bad[0]) == i, name


@pytest.mark.parametrize("name", S.MULTI)
def test_a_missing_part_is_caught(name):
    """At N = 56 x 56 the summation term dominates; what the bound sees there is a part left out."""
    x, s, g = S.inputs(name)
    B, H, W, C = x.shape
    ref, bound = S.case_ref(name)["ds"]
    t = (g.float() * x.float()).reshape(B, H * W, C)
    part = H * W // 12
    short = S.emulate_sum(t[:, part:], "forward").to(torch.bfloat16)  # the first twelfth of the map never merged
    n, _, _ = S.violations(short, ref, bound)
    assert n > B * C // 2, (name, n)


def test_global_pool_routing_is_pinned():
    def routed(mode, H, W, C, K, P=0, out=1, **kw):
        return ops.pool_global_native(mode, H, W, C, K, K, P, out, out, **kw)
    # the old kernels keep: windows of up to 64 elements, non-global, padded, max, C % 8 != 0, relu flags
    assert not routed("avg", 7, 7, 512, 7)
    assert not routed("sum", 8, 8, 64, 8)
    assert not routed("avg", 6, 6, 256, 6) and not routed("avg", 3, 3, 16, 3)
    assert not routed("avg", 14, 14, 64, 9, out=6)          # not global
    assert not routed("avg", 12, 12, 64, 14, P=1)           # padded
    assert not routed("avg", 14, 14, 64, 14, P=1, out=3)
    assert not routed("max", 14, 14, 64, 14)
    assert not routed("avg", 14, 14, 60, 14) and not routed("sum", 56, 56, 3, 56)
    assert not routed("avg", 14, 14, 64, 14, relu=True) and not routed("avg", 14, 14, 64, 14, nonneg=True)
    assert not ops.pool_global_native("avg", 14, 10, 64, 14, 14, 0, 1, 1)   # the window is not the map
    # the new kernel serves: global sum / avg of more than 64 elements
    for mode in ("sum", "avg"):
        assert routed(mode, 9, 9, 8, 9) and routed(mode, 14, 14, 256, 14) and routed(mode, 56, 56, 64, 56)
    assert ops.pool_global_native("avg", 5, 13, 8, 5, 13, 0, 1, 1)          # 65 elements, not square
    from cxxnet_amd.ops import nn
    assert nn.GLOBAL_POOL_MIN_WINDOW == 64 and nn.GLOBAL_POOL is True
