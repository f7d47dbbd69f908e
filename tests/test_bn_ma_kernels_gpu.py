"""batch_norm_ma kernels (csrc/kernels/bn_ma_kernels.hip) element by element against float64
references computed on the CPU from the exact bf16 inputs, with the derived bounds of
tests/bn_bounds.py.  The fp32 statistics are checked directly, the bf16 outputs against bounds
that carry the statistics' bounds to first order.  Each shape is the smallest that reaches a
distinct code path."""
import functools

import pytest
import torch

import bn_bounds as B
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS, MOM = 1e-5, 0.75  # (0.75 and 1 - 0.75 are exact in fp32: the reference needs no rounded momentum)

CASES = {
    "a": (1, 8),        # a single row, var = 0
    "b": (7, 3),        # scalar path, C < 8
    "c": (130, 64),     # vector path, one partial per channel; mean / std ~ 50
    "d": (513, 200),    # C % 8 == 0 but C % 64 != 0; row tail
    "e": (4099, 72),    # many partials per channel, R prime, fixed-order merge
    "f": (64, 1000),    # matrix node, C % 8 == 0, wide
    "g": (33, 10),      # scalar path with C % 8 != 0, C > 8
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (CPU, exact bf16 / fp32) and float64 references of one case, computed once."""
    R, C = CASES[name]
    gen = torch.Generator().manual_seed(ord(name))
    if name == "c":
        x1, x2 = B.case_c_inputs(R, C, 3), B.case_c_inputs(R, C, 4)
    else:
        x1 = (torch.randn(R, C, generator=gen) * 1.5 + 0.7).to(torch.bfloat16)
        x2 = (torch.randn(R, C, generator=gen) * 0.5 - 1.0).to(torch.bfloat16)
    gy = torch.randn(R, C, generator=gen).to(torch.bfloat16)
    slope = torch.rand(C, generator=gen) + 0.5
    bias = torch.randn(C, generator=gen)
    gs0, gb0 = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    y1, y1_b, s1 = B.forward_ref(x1, slope, bias, EPS)
    _, _, s2 = B.forward_ref(x2, slope, bias, EPS)
    zero, one = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    rm, e_rm = B.running_ref(zero, zero, s1["mean"], s1["e_mean"], MOM)
    rm, e_rm = B.running_ref(rm, e_rm, s2["mean"], s2["e_mean"], MOM)
    rv, e_rv = B.running_ref(one, zero, s1["var"], s1["e_var"], MOM)
    rv, e_rv = B.running_ref(rv, e_rv, s2["var"], s2["e_var"], MOM)
    bwd = B.backward_ref(gy, x1, slope, gs0, gb0, EPS)
    return dict(R=R, C=C, x1=x1, x2=x2, gy=gy, slope=slope, bias=bias, gs0=gs0, gb0=gb0, y1=y1, y1_b=y1_b, s1=s1,
                rm=rm, e_rm=e_rm, rv=rv, e_rv=e_rv, bwd=bwd)


def _state(c, keep_x=False):
    return L.BNMAState(c["C"], c["R"], DEV, torch.bfloat16, keep_x)


def _dev(c, *names):
    return [c[n].to(DEV) for n in names]


def _running(C):
    return torch.zeros(C, device=DEV), torch.ones(C, device=DEV)


def _train_fwd(c, x, y, st, rmean, rvar):
    slope, bias = _dev(c, "slope", "bias")
    L.bn_ma_forward(x, y, slope, bias, EPS, MOM, st, rmean, rvar, True)


@pytest.mark.parametrize("name", list(CASES))
def test_training_forward_and_running_statistics(name):
    c = _case(name)
    x1, x2 = _dev(c, "x1", "x2")
    st = _state(c)
    rmean, rvar = _running(c["C"])
    y = torch.full_like(x1, 3.0)
    _train_fwd(c, x1, y, st, rmean, rvar)
    s1 = c["s1"]
    stat = st.stat.cpu()
    assert torch.equal(x1.cpu(), c["x1"]), "the input must not be overwritten"
    B.assert_within(stat[0], s1["mean"], s1["e_mean"], "mean", axes="c")
    B.assert_within(stat[1], s1["var"], s1["e_var"], "var", axes="c")
    B.assert_within(stat[2], s1["inv"], s1["e_inv"], "inv", axes="c")
    B.assert_within(y, c["y1"], c["y1_b"], "y", axes="rc")
    _train_fwd(c, x2, y, st, rmean, rvar)
    B.assert_within(rmean, c["rm"], c["e_rm"], "running mean after two calls", axes="c")
    B.assert_within(rvar, c["rv"], c["e_rv"], "running var after two calls", axes="c")


@pytest.mark.parametrize("name", list(CASES))
def test_inference_forward(name):
    c = _case(name)
    (x1,) = _dev(c, "x1")
    slope, bias = _dev(c, "slope", "bias")
    gen = torch.Generator().manual_seed(7)
    rmean = torch.randn(c["C"], generator=gen)
    rvar = torch.rand(c["C"], generator=gen) + 0.25
    rm_d, rv_d = rmean.to(DEV), rvar.to(DEV)
    st = _state(c)
    y = torch.full_like(x1, 3.0)
    L.bn_ma_forward(x1, y, slope, bias, EPS, MOM, st, rm_d, rv_d, False)
    ref, bound = B.infer_ref(c["x1"], c["slope"], c["bias"], rmean, rvar, EPS)
    B.assert_within(y, ref, bound, "inference y", axes="rc")
    assert torch.equal(rm_d.cpu(), rmean) and torch.equal(rv_d.cpu(), rvar), "inference moved the running statistics"
    # a row's output does not depend on the other rows: bit-identical alone
    y1 = torch.empty_like(x1[:1])
    L.bn_ma_forward(x1[:1].clone(), y1, slope, bias, EPS, MOM, st, rm_d, rv_d, False)
    assert torch.equal(y1, y[:1])


def _check_bwd(c, dx, gslope, gbias):
    bwd = c["bwd"]
    B.assert_within(gslope, *bwd["gslope"], "gslope", axes="c")
    B.assert_within(gbias, *bwd["gbias"], "gbias", axes="c")
    if dx is not None:
        B.assert_within(dx, *bwd["dx"], "dx", axes="rc")


@pytest.mark.parametrize("name", list(CASES))
def test_backward_dx_aliasing_x(name):
    c = _case(name)
    x1, gy, slope, gslope, gbias = _dev(c, "x1", "gy", "slope", "gs0", "gb0")
    st = _state(c)
    _train_fwd(c, x1, torch.empty_like(x1), st, *_running(c["C"]))
    L.bn_ma_backward(gy, x1, x1, slope, gslope, gbias, st, True)  # dx overwrites x element by element
    assert (c["gs0"] != 0).all() and (c["gb0"] != 0).all()  # accumulation onto non-zero gradients
    _check_bwd(c, x1, gslope, gbias)
    assert torch.equal(gy.cpu(), c["gy"])


@pytest.mark.parametrize("name", list(CASES))
def test_self_loop_arrangement(name):
    """y overwrites x (a copy of x is kept), and backward's dx overwrites the gradient."""
    c = _case(name)
    buf, gy, slope, gslope, gbias = _dev(c, "x1", "gy", "slope", "gs0", "gb0")
    st = _state(c, keep_x=True)
    _train_fwd(c, buf, buf, st, *_running(c["C"]))
    B.assert_within(buf, c["y1"], c["y1_b"], "y in place", axes="rc")
    assert torch.equal(st.xsave.cpu(), c["x1"])
    buf.copy_(gy)
    L.bn_ma_backward(buf, st.xsave, buf, slope, gslope, gbias, st, True)
    _check_bwd(c, buf, gslope, gbias)


@pytest.mark.parametrize("name", list(CASES))
def test_backward_without_prop_grad(name):
    c = _case(name)
    x1, gy, slope, gslope, gbias = _dev(c, "x1", "gy", "slope", "gs0", "gb0")
    st = _state(c)
    _train_fwd(c, x1, torch.empty_like(x1), st, *_running(c["C"]))
    L.bn_ma_backward(gy, x1, x1, slope, gslope, gbias, st, False)
    _check_bwd(c, None, gslope, gbias)
    assert torch.equal(x1.cpu(), c["x1"]) and torch.equal(gy.cpu(), c["gy"]), "only the weight gradients may change"


@pytest.mark.parametrize("det", [0, 1])
@pytest.mark.parametrize("name", ["d", "e"])
def test_bitwise_reproducible(name, det):
    """(The bn_ma launchers never read the deterministic flag: there is one code path, without
    atomics, and both settings run it.  The parametrisation pins that no second path appears.)"""
    from cxxnet_amd.ops import gemm
    gemm.set_deterministic(bool(det))
    c = _case(name)
    runs = []
    for _ in range(2):
        x1, gy, slope, gslope, gbias = _dev(c, "x1", "gy", "slope", "gs0", "gb0")
        st = _state(c)
        rmean, rvar = _running(c["C"])
        y = torch.empty_like(x1)
        _train_fwd(c, x1, y, st, rmean, rvar)
        L.bn_ma_backward(gy, x1, x1, slope, gslope, gbias, st, True)
        runs.append([t.cpu() for t in (y, st.stat, rmean, rvar, x1, gslope, gbias)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_workspace_too_small_is_an_error():
    """The launcher checks the partial workspace against the geometry instead of writing past it."""
    c = _case("e")
    (x1,) = _dev(c, "x1")
    st = _state(c)
    st.ws = torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError):
        _train_fwd(c, x1, torch.empty_like(x1), st, *_running(c["C"]))
