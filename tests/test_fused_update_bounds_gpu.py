"""fused_update (csrc/kernels/optim_kernels.hip; sgd / nag / adam) element by element against the
float64 reference and the derived bounds of layer_bounds.update_ref: the new weight, the first and
(Adam) second moment and the bf16 shadow of every element of every segment, the gradient after
the step, and the sentinels of every gap between the segments and behind the arena.  The tables
(tests/layer_cases.py) hold 4-aligned segments with n % 4 in {0, 1, 2, 3}, n in {0, 1, 3}, unaligned
offsets (the element-wise path), different hyper-parameters in neighbouring segments, and 49 / 97
segments: the launcher's chunks of 48, the later launches' tables starting at segments 48 and 96.

Worst d / bound observed on an MI355X (`pytest -s` prints them per case):
  sgd   w 0.47  m1 0.28  shadow 0.99
  nag   w 0.28  m1 0.30  shadow 0.975
  adam  w 0.48  m1 0.38  m2 0.28  shadow 0.995
(the shadow's figure is the bf16 store itself).  No element left its bound, and every gap, guard
and -- without zero_grad -- gradient kept its bits.
"""
import pytest
import torch

import layer_bounds as LB
import layer_cases as LC
from cxxnet_amd.ops import optim

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALGOS = ["sgd", "nag", "adam"]
GUARD = 64


def _tables():
    return {"table": LC.update_table(), "chunk49": LC.chunk_table(49), "chunk97": LC.chunk_table(97)}


class Arena:
    """The flat state on the device, each array with GUARD sentinel elements behind it."""

    def __init__(self, st, algo, shadow=True):
        self.n = st["w"].numel()
        self.buf, self.t = {}, {}
        for k in ("w", "g", "m1") + (("m2",) if algo == "adam" else ()):
            self.buf[k], self.t[k] = LC.guarded(st[k], DEV, GUARD)
        if shadow:
            self.buf["wb"], self.t["wb"] = LC.guarded_empty((self.n,), torch.bfloat16, DEV, GUARD)
        self.algo = algo

    def step(self, segs, **kw):
        t = self.t
        optim.fused_update(self.algo, t["w"], t["g"], t["m1"], t.get("m2"), t.get("wb"), segs, **kw)

    def cpu(self):
        return {k: v.cpu() for k, v in self.buf.items()}


def _check(a, st, ref, tag, zero_grad=True):
    """every element of the arena: inside the segments within the bound, outside bit for bit"""
    n, w = a.n, {}
    t = a.t
    w["w"] = LB.assert_within(t["w"], ref["w"], ref["e_w"], "w", axes="i")
    w["m1"] = LB.assert_within(t["m1"], ref["m1"], ref["e_m1"], "m1", axes="i")
    if a.algo == "adam":
        w["m2"] = LB.assert_within(t["m2"], ref["m2"], ref["e_m2"], "m2", axes="i")
    inside = ref["inside"]
    g_after = t["g"].cpu()
    if zero_grad:
        assert bool((g_after[inside] == 0).all()), "the gradient must be exactly 0 after the step"
        assert bool((g_after[~inside] == LC.SENTINEL).all()), "a gradient outside the segments was touched"
    else:
        assert torch.equal(g_after.view(torch.int32), st["g"].view(torch.int32)), "zero_grad=False must leave g alone"
    if "wb" in t:
        wb = t["wb"].cpu()
        # the gaps keep the sentinel (bound 0 there), the segments hold the shadow of the new weight
        sref = torch.where(inside, ref["w"], torch.full_like(ref["w"], LC.SENTINEL))
        w["wb"] = LB.assert_within(wb, sref, ref["e_wb"], "bf16 shadow", axes="i")
        assert torch.equal(wb[inside], t["w"].cpu()[inside].to(torch.bfloat16)), \
            "the shadow must be the bf16 rounding of the stored fp32 weight"
    for k, buf in a.buf.items():
        LC.assert_guard(buf, n, k)
    print("\n%s: worst d/bound %s" % (tag, "  ".join("%s %.3g" % kv for kv in w.items())))


def _ref(algo, st, segs):
    return LB.update_ref(algo, st["w"], st["g"], st["m1"], st["m2"] if algo == "adam" else None, segs)


@pytest.mark.parametrize("table", ["table", "chunk49", "chunk97"])
@pytest.mark.parametrize("algo", ALGOS)
def test_step(algo, table):
    size, segs = _tables()[table]
    if table == "table":
        assert {s[1] % 4 for s in segs if s[0] % 4 == 0 and s[1] > 4} == {0, 1, 2, 3}
        assert {0, 1, 3} <= {s[1] for s in segs} and any(s[0] % 4 for s in segs)
    else:
        assert len(segs) == int(table[5:]) > 48
    st = LC.update_state(size, segs, algo)
    if algo == "sgd":
        assert torch.isnan(st["g"]).any() and torch.isinf(st["g"]).any()
    a = Arena(st, algo)
    a.step(segs)
    _check(a, st, _ref(algo, st, segs), "%s %s" % (algo, table))


@pytest.mark.parametrize("algo", ALGOS)
def test_without_shadow_and_without_zero_grad(algo):
    size, segs = LC.update_table()
    st = LC.update_state(size, segs, algo)
    ref = _ref(algo, st, segs)
    a = Arena(st, algo, shadow=False)
    a.step(segs)
    _check(a, st, ref, "%s wb=None" % algo)
    b = Arena(st, algo)
    b.step(segs, zero_grad=False)
    _check(b, st, ref, "%s zero_grad=False" % algo, zero_grad=False)
    assert torch.equal(a.t["w"], b.t["w"]) and torch.equal(a.t["m1"], b.t["m1"])


@pytest.mark.parametrize("algo", ["nag", "adam"])
def test_clip_is_ignored_by_nag_and_adam(algo):
    size, segs = LC.update_table()
    assert any(s[5] > 0 for s in segs)
    st = LC.update_state(size, segs, algo)
    a, b = Arena(st, algo), Arena(st, algo)
    a.step(segs)
    b.step([s[:5] + (0.0,) for s in segs])
    for (k, x), y in zip(a.cpu().items(), b.cpu().values()):
        assert torch.equal(x, y), k


def test_non_default_adam_decays():
    size, segs = LC.update_table()
    st = LC.update_state(size, segs, "adam", seed=3)
    a = Arena(st, "adam")
    a.step(segs, d1=0.25, d2=0.01)
    _check(a, st, LB.update_ref("adam", st["w"], st["g"], st["m1"], st["m2"], segs, 0.25, 0.01), "adam d1 .25 d2 .01")
