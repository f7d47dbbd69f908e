"""group_norm kernels (csrc/kernels/gn_kernels.hip) element by element against float64 references
computed on the CPU from the exact bf16 inputs, with the derived bounds of tests/gn_bounds.py.  The
fp32 statistics are checked directly, the bf16 outputs against bounds that carry the statistics'
bounds to first order.  Each shape (gn_bounds.CASES) is the smallest that reaches a distinct code
path.  Every buffer a kernel writes sits between guard bands, checked after every call."""
import re

import pytest
import torch

import gn_bounds as GB
from cxxnet_amd.ops import layer_ops as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64  # elements on either side (a multiple of 8: the guarded bf16 buffers stay 16-byte aligned)
SENT16, SENT32 = 777.0, -12345.0


class Guarded:
    """A tensor of `shape` cut from the middle of a buffer whose margins hold a sentinel.  offset:
    shift the view by that many elements (1: a bf16 view that is not 16-byte aligned)."""

    def __init__(self, shape, dtype, fill=None, offset=0):
        n = 1
        for s in shape:
            n *= s
        self.sent = SENT16 if dtype == torch.bfloat16 else SENT32
        self.buf = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device=DEV)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.buf[:self.lo] == self.sent).all() and (self.buf[self.hi:] == self.sent).all())


class Run:
    """One forward (and backward) of a case on guarded buffers."""

    def __init__(self, c, B=None, st_batch=None, offset=0):
        self.c = c
        B = c["B"] if B is None else B
        HW, C, G = c["HW"], c["C"], c["G"]
        self.B = B
        shape = (B, HW, C)
        self.x = Guarded(shape, torch.bfloat16, c["x"][:B], offset)
        self.g = Guarded(shape, torch.bfloat16, c["gy"][:B], offset)
        self.y = Guarded(shape, torch.bfloat16, None, offset)
        self.dx = Guarded(shape, torch.bfloat16, None, offset)
        self.slope, self.bias = c["slope"].to(DEV), c["bias"].to(DEV)
        self.gslope, self.gbias = Guarded((C,), torch.float32, c["gs0"]), Guarded((C,), torch.float32, c["gb0"])
        sb = B if st_batch is None else st_batch
        st = L.GNState(sb, HW, C, G, DEV)
        self.gst = [Guarded((sb, G), torch.float32), Guarded((sb, G), torch.float32), Guarded((sb, G, 2), torch.float32),
                    Guarded((st.ws.numel(),), torch.float32)]
        st.mean, st.rstd, st.coef, st.ws = (q.t for q in self.gst)
        for q in self.gst:
            q.t.fill_(3.0)  # stale values: nothing may depend on what the buffers held
        self.st = st
        self.all = [self.x, self.g, self.y, self.dx, self.gslope, self.gbias] + self.gst

    def forward(self):
        L.gn_forward(self.x.t, self.y.t, self.slope, self.bias, GB.EPS, self.st)
        return self

    def backward(self, dx="own", prop_grad=True):
        self.dx_t = {"own": self.dx.t, "x": self.x.t, "g": self.g.t}[dx]
        L.gn_backward(self.g.t, self.x.t, self.dx_t, self.slope, self.gslope.t, self.gbias.t, self.st, prop_grad)
        return self

    def intact(self):
        return all(q.intact() for q in self.all)

    def outputs(self):
        return [t.cpu().clone() for t in (self.y.t, self.st.mean[:self.B], self.st.rstd[:self.B], self.dx_t,
                                          self.gslope.t, self.gbias.t)]


def _check_fwd(r, rows=None):
    c, s = r.c, r.c["s"]
    sl = slice(0, r.B if rows is None else rows)
    assert torch.equal(r.x.t.cpu(), c["x"][:r.B]), "x must not change in forward"
    GB.assert_within(r.st.mean[sl], s["mean"][sl], s["e_mean"][sl], "mean", axes="bg")
    GB.assert_within(r.st.rstd[sl], s["rstd"][sl], s["e_rstd"][sl], "rstd", axes="bg")
    GB.assert_within(r.y.t, c["y"][sl], c["y_b"][sl], "y", axes="brc")


def _check_bwd(r, dx=True):
    bwd = r.c["bwd"]
    assert (r.c["gs0"] != 0).all() and (r.c["gb0"] != 0).all()  # accumulation onto non-zero gradients
    GB.assert_within(r.gslope.t, *bwd["gslope"], "gslope", axes="c")
    GB.assert_within(r.gbias.t, *bwd["gbias"], "gbias", axes="c")
    if dx:
        GB.assert_within(r.dx_t, *bwd["dx"], "dx", axes="brc")


@pytest.mark.parametrize("name", list(GB.CASES))
def test_forward_and_backward_within_the_bounds(name):
    c = GB.case(name)
    r = Run(c).forward()
    _check_fwd(r)
    r.backward()
    _check_bwd(r)
    assert torch.equal(r.x.t.cpu(), c["x"]) and torch.equal(r.g.t.cpu(), c["gy"]), "backward only reads x and g"
    assert r.intact(), "a guard band was written"


def test_one_element_groups_give_the_bias_and_a_zero_gradient_exactly():
    c = GB.case("one_elem")
    r = Run(c).forward().backward()
    assert torch.equal(r.st.mean.cpu().view(-1), c["x"].float().view(-1))
    assert torch.equal(r.y.t.cpu().view(-1), c["bias"].to(torch.bfloat16)), "var = 0 exactly: y is the bias, bit for bit"
    assert torch.equal(r.dx.t.cpu(), torch.zeros(1, 1, 8, dtype=torch.bfloat16)), "dx = 0 exactly"
    assert r.intact()


@pytest.mark.parametrize("alias", ["x", "g"])
@pytest.mark.parametrize("name", list(GB.CASES))
def test_dx_may_overwrite_x_or_g(name, alias):
    c = GB.case(name)
    ref = Run(c).forward().backward()
    r = Run(c).forward().backward(dx=alias)
    _check_bwd(r)
    for a, b in zip(ref.outputs(), r.outputs()):
        assert torch.equal(a, b), "aliasing changed the bits"
    assert torch.equal(r.dx.t.cpu(), torch.full_like(c["x"], SENT16)), "the separate dx buffer was written"
    assert r.intact()


@pytest.mark.parametrize("name", ["scalar", "lane4groups", "straddle", "matrix"])
def test_backward_without_prop_grad_writes_no_dx(name):
    c = GB.case(name)
    r = Run(c).forward().backward(prop_grad=False)
    _check_bwd(r, dx=False)
    assert torch.equal(r.dx.t.cpu(), torch.full_like(c["x"], SENT16)), "dx was written"
    assert torch.equal(r.x.t.cpu(), c["x"]) and torch.equal(r.g.t.cpu(), c["gy"])
    assert r.intact()


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


def _variants(names, kernel):
    """The template arguments V with which `kernel` ran (demangled gn_stats<8> or mangled gn_statsILi8E)."""
    out = set()
    for n in names:
        for m in re.finditer(kernel + r"(?:<(?:\(int\))?(\d+)>|ILi(\d+)E)", n):
            out.add(int(m.group(1) or m.group(2)))
    return out


def test_an_unaligned_view_takes_the_scalar_variant():
    """A vector-eligible shape (C % 8 == 0) passed as views offset by one element (2 bytes): the
    16-byte accesses would be misaligned, so the launchers must pick V = 1 -- read off the kernels'
    names -- and the results meet the same bounds."""
    c = GB.case("lane4groups")
    r = Run(c, offset=1)
    assert r.x.t.data_ptr() % 16 == 2 and r.y.t.data_ptr() % 16 == 2
    r.forward()
    _check_fwd(r)
    r.backward()
    _check_bwd(r)
    assert r.intact()
    kernels = ("gn_stats", "gn_apply", "gn_bwd_reduce", "gn_bwd_apply")
    names = _kernel_names(lambda: Run(c, offset=1).forward().backward())
    for k in kernels:
        assert _variants(names, k) == {1}, (k, sorted(names))
    names = _kernel_names(lambda: Run(c).forward().backward())
    for k in kernels:
        assert _variants(names, k) == {8}, (k, sorted(names))


def test_a_state_sized_for_five_samples_serves_two():
    c = GB.case("matrix")  # B = 5
    full = Run(c).forward().backward()
    r = Run(c, B=2, st_batch=5).forward()
    s = c["s"]
    GB.assert_within(r.st.mean[:2], s["mean"][:2], s["e_mean"][:2], "mean", axes="bg")
    GB.assert_within(r.y.t, c["y"][:2], c["y_b"][:2], "y", axes="brc")
    assert torch.equal(r.st.mean[2:].cpu(), torch.full((3, 1), 3.0)), "statistics rows past the batch were written"
    r.backward()
    assert torch.equal(r.st.coef[2:].cpu(), torch.full((3, 1, 2), 3.0))
    assert r.intact()
    # y and dx of a sample do not depend on the batch: the same bits as inside the batch of 5
    assert torch.equal(r.y.t.cpu(), full.y.t[:2].cpu()) and torch.equal(r.dx.t.cpu(), full.dx.t[:2].cpu())
    # the weight gradients are those of the two samples alone
    two = {k: c[k][:2] if k in ("x", "gy") else c[k] for k in c}
    bwd = GB.backward_ref(two["gy"], two["x"], c["slope"], c["gs0"], c["gb0"], c["G"], GB.EPS)
    GB.assert_within(r.gslope.t, *bwd["gslope"], "gslope of 2", axes="c")
    GB.assert_within(r.gbias.t, *bwd["gbias"], "gbias of 2", axes="c")


@pytest.mark.parametrize("name", ["lane4groups", "group2lanes", "scalar", "bigmean"])
def test_a_sample_alone_gives_the_bits_it_gives_inside_the_batch(name):
    c = GB.case(name)
    full = Run(c).forward().backward()
    one = Run(c, B=1).forward().backward()
    assert torch.equal(one.y.t.cpu(), full.y.t[:1].cpu())
    assert torch.equal(one.dx.t.cpu(), full.dx.t[:1].cpu())
    assert torch.equal(one.st.mean.cpu(), full.st.mean[:1].cpu()) and torch.equal(one.st.rstd.cpu(), full.st.rstd[:1].cpu())
    assert one.intact() and full.intact()


@pytest.mark.parametrize("name", list(GB.CASES))
def test_bitwise_reproducible(name):
    """There is one code path, without atomics: two runs from stale buffers give the same bits in
    every output, the statistics included."""
    c = GB.case(name)
    a = Run(c).forward().backward().outputs()
    b = Run(c).forward().backward().outputs()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_bad_arguments_are_errors():
    """The launchers check the workspace against the geometry instead of writing past it, and refuse
    a group count that does not divide the channels."""
    c = GB.case("partials")
    r = Run(c)
    r.st.ws = torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError):
        r.forward()
    r = Run(GB.case("scalar"))
    r.st.groups = 4  # 6 channels
    with pytest.raises((RuntimeError, ValueError)):
        r.forward()
