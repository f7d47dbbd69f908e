"""The pooling kernels (csrc/kernels/pool_kernels.hip behind cxn_pool_fwd, cxn_pool_bwd and
cxn_pool_bwd_tie_all) per element against the float64 references of tests/pool_bounds.py, on its
case table: max outputs and first-max offsets exactly, sum / avg outputs and every data gradient
within the derived bound, the folded bias gradient against bounds.dbias_ref of the dx the kernel
stored.  Every output is a slice of a larger buffer prefilled with NaN (0xA5 for the offsets), with
more than one image row of it before and after: an element left unwritten fails, and so does a
write outside the tensor (the strip and cell kernels walk rows and cells that reach past the map).
The backward is fed the reference's state, so the two checks stay independent.

Max outputs and offsets: exact on every case, float-compare and integer-key (NN) kernels alike.
Worst d / bound per kernel family as measured on the MI355X (1 would be the bound):
    pool_fwd<1>          sum 0.979  avg 0.951
    pool_fwd_rows<2,3>   sum 0.996  avg 0.953
    pool_fwd_rows<1,3>   sum 0.988  avg 0.988
    pool_fwd_rows<2,2>              avg 0.996
    pool_fwd_rows<0,0>   sum 0.988  avg 0.978
    pool_bwd<1>          max 0.973  sum 0.872  avg 0.995
    pool_bwd<8>          max 0.996  sum 0.981  avg 0
    pool_bwd_rows<2,3>   max 0.996  sum 0.996  avg 0.937
    pool_bwd_rows<1,3>              sum 0.985  avg 0.996
    pool_bwd_rows<2,2>   max 0                 avg 0
    pool_bwd_rows<0,0>   max 0.996  sum 0.996  avg 0.956
    pool_bwd_s1k3<4>     max 0.996
    pool_bwd_s2k3        max 0.996
    pool_bwd_tie_all     0.996
    dbias (pool_bwd<8> + partials_reduce, plain and deterministic; pool_bwd<1> + bias_grad)  0
0.996 = 1 / (1 + 2^-8) is the bf16 store alone (round to nearest of a value just above a power of
two, which u charges in full); 0 where each pixel has one window (2 x 2 / 2: a single term, and
avg's 1/4 is a power of two) and for the bias sums (a few hundred bf16 values of like
size add up exactly in fp32).  Every family equals the CPU emulation's worst or stays below it.
"""
import pytest
import torch

import pool_bounds as PB
from cxxnet_amd import native, ops
from cxxnet_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE_FILL = 0xA5  # bit 7 and tap 37: no window of the table has that many taps
DB_INIT = 0.5


def _bits(t):
    return t.detach().cpu().contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


class Guarded:
    """A device tensor of `shape` cut out of a larger 1-d buffer filled with `fill`, with a guard of
    more than one image row (a multiple of 8 elements, which keeps the 16-byte alignment) on each
    side; src: what the tensor holds instead of the fill."""

    def __init__(self, shape, dtype, fill, src=None):
        n = 1
        for s in shape:
            n *= s
        row = shape[-2] * shape[-1] if len(shape) > 1 else shape[-1]
        self.g, self.n = (row + 7) // 8 * 8 + 8, n
        self.whole = torch.full((n + 2 * self.g,), fill, dtype=dtype, device=DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.g:self.g + n].view(shape)
        if src is not None:
            self.t.copy_(src)
        self.before = _bits(self.whole)

    def assert_guards_intact(self, what):
        now = _bits(self.whole)
        assert torch.equal(now[:self.g], self.before[:self.g]), what + ": written before the tensor"
        assert torch.equal(now[self.g + self.n:], self.before[self.g + self.n:]), what + ": written past the tensor"

    def assert_unchanged(self, what):
        assert torch.equal(_bits(self.whole), self.before), what + ": an input was written"


def _geo(c):
    return c.KH, c.KW, c.S, c.P


def _note(family, name, worst):
    print("WORST %s %s %.3g" % (family, name, worst))


def _bf16(shape, src=None):
    return Guarded(shape, torch.bfloat16, float("nan"), src)


# ------------------------------------------------------------------------------------- forward
def _forward(name):
    c = PB.CASES[name]
    runs = [(k, f) for k in ("signed", "nonneg") for f in PB.FWD_FLAGS[k]] if c.mode == "max" else \
        [("signed", f) for f in PB.SUM_FLAGS]
    marked = False
    for kind, flags in runs:
        what = "%s %s flags %d (%s)" % (name, kind, flags, PB.fwd_kernel(c, flags))
        x = _bf16((c.N, c.H, c.W, c.C), PB.data(name, kind))
        y = _bf16(PB.out_shape(c))
        st = Guarded(PB.out_shape(c), torch.uint8, STATE_FILL) if c.mode == "max" else None
        ops.pool_forward(x.t, y.t, st.t if st else None, *_geo(c), c.mode, relu=bool(flags & 1),
                         mark_mask=bool(flags & 2), nonneg=bool(flags & 4))
        torch.cuda.synchronize()
        x.assert_unchanged(what)
        y.assert_guards_intact(what + " y")
        if c.mode == "max":
            y_ref, st_ref = PB.forward_ref(name, kind, flags)
            PB.assert_exact(y.t, y_ref, what + " y")
            st.assert_guards_intact(what + " state")
            PB.assert_exact(st.t, st_ref.double(), what + " state")
            assert torch.equal(st.t.cpu(), st_ref)
            marked = marked or bool((st_ref >= 128).any())
        else:
            ref, bound = PB.forward_ref(name, kind, flags)
            _note("forward %s %s" % (c.mode, c.fwd), name, PB.assert_within(y.t, ref, bound, what))
    assert marked or c.mode != "max", "bit 7 never occurred"


def _named(pred):
    return [n for n, c in PB.CASES.items() if pred(c)]


@pytest.mark.parametrize("name", _named(lambda c: c.fwd == "pool_fwd<1>"))
def test_pool_fwd_scalar(name):
    _forward(name)


@pytest.mark.parametrize("name", _named(lambda c: c.fwd.startswith("pool_fwd_rows")))
def test_pool_fwd_rows(name):
    _forward(name)


@pytest.mark.parametrize("name", _named(lambda c: c.fwd.startswith("pool_fwd_s1k3")))
def test_pool_fwd_s1k3(name):
    _forward(name)


# ------------------------------------------------------------------------------------- backward
def _backward_once(name, kind, flags, relu, what, dbias=False, alias=False):
    """one ops.pool_backward of the case with the reference state of (kind, flags); returns the
    worst d / bound of dx"""
    c = PB.CASES[name]
    x = _bf16((c.N, c.H, c.W, c.C), PB.data(name, kind))
    dy = _bf16(PB.out_shape(c), PB.inputs(name)["dy"])
    st = Guarded(PB.out_shape(c), torch.uint8, STATE_FILL, PB.forward_ref(name, kind, flags)[1]) if c.mode == "max" else None
    dx = x if alias else _bf16((c.N, c.H, c.W, c.C))
    db = Guarded((c.C,), torch.float32, float("nan"), torch.full((c.C,), DB_INIT)) if dbias else None
    ops.pool_backward(x.t, st.t if st else None, dy.t, dx.t, *_geo(c), c.mode, relu, dbias=db.t if db else None)
    torch.cuda.synchronize()
    if not alias:
        x.assert_unchanged(what)
    dy.assert_unchanged(what)
    if st:
        st.assert_unchanged(what)
    dx.assert_guards_intact(what + " dx")
    ref, bound = PB.backward_ref(name, kind, flags, relu)
    worst = PB.assert_within(dx.t, ref, bound, what + " dx")
    if db:
        db.assert_guards_intact(what + " dbias")
        r, b = PB.dbias_ref(dx.t, DB_INIT)
        _note("dbias " + PB.bwd_kernel(c, dbias=True), name, PB.assert_within(db.t, r, b, what + " dbias", axes="c"))
    return worst


def _backward(name):
    c = PB.CASES[name]
    for kind, flags, relu in PB.BWD_RUNS[c.mode]:
        what = "%s %s relu %d (%s)" % (name, kind, relu, c.bwd)
        _note("backward %s %s" % (c.mode, c.bwd), name, _backward_once(name, kind, flags, relu, what))


@pytest.mark.parametrize("name", _named(lambda c: c.bwd == "pool_bwd<1>"))
def test_pool_bwd_scalar(name):
    _backward(name)


@pytest.mark.parametrize("name", _named(lambda c: c.bwd.startswith("pool_bwd_rows")))
def test_pool_bwd_rows(name):
    _backward(name)


@pytest.mark.parametrize("name", _named(lambda c: c.bwd.startswith("pool_bwd_s1k3")))
def test_pool_bwd_s1k3(name):
    _backward(name)


@pytest.mark.parametrize("name", _named(lambda c: c.bwd == "pool_bwd_s2k3"))
def test_pool_bwd_s2k3_and_its_one_pixel_variant(name):
    """3 x 3 / 2 max: the 2 x 2 cell kernel, then (kernel variant 0) pool_bwd_rows<2,3> in max mode"""
    c = PB.CASES[name]
    k = native.kernels()
    try:
        for v in (1, 0):
            native.check(k.cxn_set_kernel_variant(0, v), "variant")
            fam = PB.bwd_kernel(c, cells=bool(v))
            for kind, flags, relu in PB.BWD_RUNS["max"]:
                what = "%s %s relu %d (%s)" % (name, kind, relu, fam)
                _note("backward max " + fam, name, _backward_once(name, kind, flags, relu, what))
    finally:
        native.check(k.cxn_set_kernel_variant(0, 1), "variant")


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", _named(lambda c: c.dbias and c.C % 8 == 0))
def test_pool_bwd_vec8_with_the_folded_bias_gradient(name, det):
    """pool_bwd<8>: dx, and dbias = init + the column sums of the dx it stored (per-block partials,
    then partials_reduce: several row chunks with atomics, or one ordered pass in deterministic
    mode)"""
    c = PB.CASES[name]
    G.set_deterministic(det)  # (tests/conftest.py puts the mode back)
    assert PB.bwd_kernel(c, dbias=True) == "pool_bwd<8>"
    for kind, flags, relu in PB.BWD_RUNS[c.mode]:
        what = "%s %s relu %d det %d (pool_bwd<8>)" % (name, kind, relu, det)
        _note("backward %s pool_bwd<8>" % c.mode, name, _backward_once(name, kind, flags, relu, what, dbias=True))


@pytest.mark.parametrize("name", _named(lambda c: c.dbias and c.C % 8 != 0))
def test_pool_bwd_scalar_with_the_separate_bias_pass(name):
    c = PB.CASES[name]
    for kind, flags, relu in PB.BWD_RUNS[c.mode]:
        what = "%s %s relu %d (pool_bwd<1> + bias_grad)" % (name, kind, relu)
        _backward_once(name, kind, flags, relu, what, dbias=True)


@pytest.mark.parametrize("name", _named(lambda c: c.alias))
def test_pool_bwd_in_place(name):
    """dx aliasing x with relu = 1 (the docstring of ops.pool_backward promises it), one case per
    backward family; the 3 x 3 / 2 max case on both kernel variants"""
    c = PB.CASES[name]
    flags = 1 if c.mode == "max" else 0
    k = native.kernels()
    try:
        for v in ((1, 0) if c.bwd == "pool_bwd_s2k3" else (1,)):
            native.check(k.cxn_set_kernel_variant(0, v), "variant")
            fam = PB.bwd_kernel(c, dbias=c.dbias, cells=bool(v))
            _backward_once(name, "signed", flags, 1, "%s in place (%s)" % (name, fam), dbias=c.dbias, alias=True)
    finally:
        native.check(k.cxn_set_kernel_variant(0, 1), "variant")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", _named(lambda c: c.tie))
def test_pool_bwd_tie_all(name, relu):
    c = PB.CASES[name]
    y_ref, ref, bound = PB.tie_all_ref(name, relu)
    what = "%s relu %d (pool_bwd_tie_all)" % (name, relu)
    x = _bf16((c.N, c.H, c.W, c.C), PB.data(name, "signed"))
    y = _bf16(PB.out_shape(c), y_ref)
    dy = _bf16(PB.out_shape(c), PB.inputs(name)["dy"])
    dx = _bf16((c.N, c.H, c.W, c.C))
    ops.pool_backward_tie_all(x.t, y.t, dy.t, dx.t, *_geo(c), relu=relu)
    torch.cuda.synchronize()
    for t in (x, y, dy):
        t.assert_unchanged(what)
    dx.assert_guards_intact(what)
    _note("tie_all", name, PB.assert_within(dx.t, ref, bound, what))
    # the kernel's own forward gives the y that was fed
    y2 = _bf16(PB.out_shape(c))
    ops.pool_forward(x.t, y2.t, None, *_geo(c), "max", relu)
    torch.cuda.synchronize()
    PB.assert_exact(y2.t, y_ref.double(), what + " forward without a state")
