"""tests/pool_bounds.py on the CPU.

The explicit float64 references agree with the project's CPU executor path (ops.pool_forward,
ops.pool_backward, ops.pool_backward_tie_all on CPU tensors), with which they share no code: values
and states exactly in max mode, sum and avg within the bound.  An fp32 emulation of the kernels'
order of operations stays inside every bound on every case of the table, and each planted defect
leaves it at exactly the planted elements.

Worst d / bound of the emulation per family, over every case (1 would be the bound):
    forward sum 0.996, forward avg 0.996, backward max 0.996, backward sum 0.996,
    backward avg 0.996, tie_all 0.996, folded dbias 0
0.996 = 1 / (1 + 2^-8) is the bf16 store alone: round to nearest moves a value just above a power
of two by 2^-8 of itself, which is what u charges, and among some thousand elements one lies
there; the fp32 terms g A are a few 1e-4 of the bound where nothing cancels.  The folded bias gradient is exact: an fp32
sum of a few hundred bf16 values of like size loses no bit.
"""
import pytest
import torch

import pool_bounds as PB
from cxxnet_amd import ops

PREFILL = 1000.0  # what an unwritten output element holds
MAX_CASES = [n for n, c in PB.CASES.items() if c.mode == "max"]
SUM_CASES = [n for n, c in PB.CASES.items() if c.mode != "max"]
WORST = {}


def _note(family, worst):
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print("worst d/bound %s %.3g" % (family, WORST[family]))


def _geo(c):
    return c.KH, c.KW, c.S, c.P


def _flat(shape, *idx):
    f = 0
    for s, i in zip(shape, idx):
        f = f * s + i
    return f


# ----------------------------------------------------------------- the two CPU implementations
@pytest.mark.parametrize("name", list(PB.CASES))
def test_the_case_reaches_the_kernel_it_names(name):
    c = PB.CASES[name]
    assert PB.fwd_kernel(c, 0) == c.fwd and PB.bwd_kernel(c) == c.bwd
    if c.mode == "max" and c.C % 8 == 0 and c.fwd != "pool_fwd_rows<0,0>":
        assert PB.fwd_kernel(c, 4) == c.fwd[:-1] + ",NN>" == PB.fwd_kernel(c, 6)
        assert PB.fwd_kernel(c, 5) == c.fwd  # relu in the pool: float compare
    if c.bwd == "pool_bwd_s2k3":
        assert PB.bwd_kernel(c, cells=False) == "pool_bwd_rows<2,3>"


def test_every_kernel_is_reached():
    fwd = {PB.fwd_kernel(c, f) for c in PB.CASES.values() for f in (0, 4)}
    bwd = {PB.bwd_kernel(c, dbias=d, cells=v) for c in PB.CASES.values() for d in {False, c.dbias} for v in (True, False)}
    assert fwd >= {"pool_fwd<1>", "pool_fwd_rows<2,3>", "pool_fwd_rows<2,3,NN>", "pool_fwd_rows<1,3>", "pool_fwd_rows<2,2>",
                   "pool_fwd_rows<2,2,NN>", "pool_fwd_rows<0,0>", "pool_fwd_s1k3<4>", "pool_fwd_s1k3<4,NN>"}
    assert bwd >= {"pool_bwd<1>", "pool_bwd<1>+bias_grad", "pool_bwd<8>", "pool_bwd_rows<2,3>", "pool_bwd_rows<1,3>",
                   "pool_bwd_rows<2,2>", "pool_bwd_rows<0,0>", "pool_bwd_s1k3<4>", "pool_bwd_s2k3"}
    assert sum(c.tie for c in PB.CASES.values()) >= 2 and {c.C for c in PB.CASES.values() if c.tie} >= {3, 16}
    cs = list(PB.CASES.values())
    assert {c.N for c in cs} == {1, 3} and 2 * sum(c.H != c.W for c in cs) >= len(cs)
    assert {c.C for c in cs if c.dbias and c.C % 8 == 0} == {8, 24, 40}
    for fam in ("pool_bwd_rows", "pool_bwd_s1k3", "pool_bwd_s2k3", "pool_bwd<1>"):
        assert any(c.alias and c.bwd.startswith(fam) for c in cs), fam
    assert any(c.alias and c.dbias and c.C % 8 == 0 for c in cs)  # pool_bwd<8>


@pytest.mark.parametrize("name", MAX_CASES)
def test_max_reference_equals_the_cpu_executor(name):
    c = PB.CASES[name]
    dy = PB.inputs(name)["dy"].float()
    for kind, flags, relu in (("signed", 0, 0), ("signed", 1, 1), ("nonneg", 0, 1)):
        x = PB.data(name, kind).float()
        y_ref, st_ref = PB.forward_ref(name, kind, flags)
        y = torch.full(PB.out_shape(c), float("nan"))
        st = torch.full(PB.out_shape(c), 0xA5, dtype=torch.uint8)
        ops.pool_forward(x, y, st, *_geo(c), "max", bool(flags & 1))
        PB.assert_exact(y, y_ref, "%s %s y" % (name, kind))
        assert torch.equal(st, st_ref), "%s %s state" % (name, kind)
        # bit 7 is the mark of a maximum that is not > 0, on the same taps
        y2, st2 = PB.forward_ref(name, kind, flags | 2)
        assert torch.equal(st2 & 127, st_ref) and torch.equal(st2 >= 128, ~(y_ref > 0)) and torch.equal(y2, y_ref)
        assert bool((st2 >= 128).any()), "no window of %s (%s) is entirely <= 0" % (name, kind)
        dx = torch.full(x.shape, float("nan"))
        ops.pool_backward(x, st, dy, dx, *_geo(c), "max", relu)
        ref, bound = PB.max_backward_ref(x, st_ref, dy, *_geo(c), relu)
        PB.assert_within(dx, ref, bound, "%s %s dx relu %d" % (name, kind, relu))
        if kind == "nonneg":  # relu' read from bit 7 is relu' read from x, for an input >= 0
            ref2, bound2 = PB.backward_ref(name, "nonneg", 2, 2)
            assert torch.equal(ref2, ref) and torch.equal(bound2, bound)
    # ties are frequent, -0.0 is planted
    x = PB.data(name, "signed")
    assert bool(((x == 0) & (x.view(torch.int16) < 0)).any())


@pytest.mark.parametrize("name", SUM_CASES)
def test_sum_and_avg_references_hold_the_cpu_executor(name):
    c = PB.CASES[name]
    dy = PB.inputs(name)["dy"].float()
    x = PB.data(name, "signed").float()
    for flags in PB.SUM_FLAGS:
        ref, bound = PB.forward_ref(name, "signed", flags)
        y = torch.full(PB.out_shape(c), float("nan"))
        ops.pool_forward(x, y, None, *_geo(c), c.mode, bool(flags))
        PB.assert_within(y, ref, bound, "%s y flags %d" % (name, flags))
    for _, _, relu in PB.BWD_RUNS[c.mode]:
        ref, bound = PB.backward_ref(name, "signed", 0, relu)
        dx = torch.full(x.shape, float("nan"))
        db = torch.full((c.C,), 0.5)
        ops.pool_backward(x, None, dy, dx, *_geo(c), c.mode, relu, dbias=db)
        PB.assert_within(dx, ref, bound, "%s dx relu %d" % (name, relu))
        r, b = PB.dbias_ref(dx, 0.5)
        PB.assert_within(db, r, b, name + " dbias", axes="c")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("name", [n for n, c in PB.CASES.items() if c.tie])
def test_tie_all_reference_holds_the_cpu_executor(name, relu):
    c = PB.CASES[name]
    y, ref, bound = PB.tie_all_ref(name, relu)
    x, dy = PB.data(name, "signed").float(), PB.inputs(name)["dy"].float()
    dx = torch.full(x.shape, float("nan"))
    ops.pool_backward_tie_all(x, y.float(), dy, dx, *_geo(c), relu=relu)
    _note("tie_all", PB.assert_within(dx.to(torch.bfloat16), ref, bound, "%s relu %d" % (name, relu)))
    # more inputs than one per window receive a gradient: the data has ties
    first = PB.max_backward_ref(x, PB.forward_ref(name, "signed", int(relu))[1], dy, *_geo(c), int(relu))[0]
    assert int((ref != 0).sum()) > int((first != 0).sum())


# ----------------------------------------------------------------- the fp32 emulation
@pytest.mark.parametrize("name", list(PB.CASES))
def test_fp32_emulation_stays_inside_the_bound(name):
    c = PB.CASES[name]
    dy = PB.inputs(name)["dy"]
    if c.mode != "max":
        for flags in PB.SUM_FLAGS:
            ref, bound = PB.forward_ref(name, "signed", flags)
            y = PB.emulate_forward(PB.data(name, "signed"), *_geo(c), c.mode, flags)
            _note("forward " + c.mode, PB.assert_within(y, ref, bound, "%s flags %d" % (name, flags)))
    for kind, flags, relu in PB.BWD_RUNS[c.mode]:
        x = PB.data(name, kind)
        st = PB.forward_ref(name, kind, flags)[1] if c.mode == "max" else None
        ref, bound = PB.backward_ref(name, kind, flags, relu)
        dx = PB.emulate_backward(x, st, dy, *_geo(c), c.mode, relu)
        _note("backward " + c.mode, PB.assert_within(dx, ref, bound, "%s %s relu %d" % (name, kind, relu)))
        assert bool((bound == 0).any()) or c.mode != "max" or c.S < min(c.KH, c.KW)
        if c.dbias:  # an fp32 column sum of what was stored, onto the initial value
            db = torch.full((c.C,), 0.5) + dx.float().reshape(-1, c.C).sum(0)
            r, b = PB.dbias_ref(dx, 0.5)
            _note("folded dbias", PB.assert_within(db, r, b, name + " dbias", axes="c"))


# ----------------------------------------------------------------- planted defects
def _window_f32(x, c, n, ho, wo, ch, drop=None, clipped_divisor=False):
    """one output of emulate_forward, by hand: optionally without the tap at input (h, w) = drop,
    or (avg) divided by the number of taps inside the map"""
    acc = torch.zeros((), dtype=torch.float32)
    k = 0
    for kh in range(c.KH):
        for kw in range(c.KW):
            h, w = ho * c.S - c.P + kh, wo * c.S - c.P + kw
            if 0 <= h < c.H and 0 <= w < c.W:
                k += 1
                if (h, w) != drop:
                    acc = acc + x[n, h, w, ch].float()
    if c.mode == "avg":
        acc = acc / torch.tensor(float(k), dtype=torch.float32) if clipped_divisor else acc * PB._f32_inv(c.KH, c.KW)
    return acc.to(torch.bfloat16)


def _only(got, ref, bound, want, min_excess=4.0):
    n, worst, bad = PB.violations(got, ref, bound)
    assert sorted(bad.tolist()) == sorted(want) and worst > min_excess, (n, worst, bad.tolist(), want)


def test_a_dropped_far_edge_tap_leaves_the_bound():
    name = "k3s2_avg_9x8"
    c = PB.CASES[name]
    x = PB.data(name, "signed")
    ref, bound = PB.forward_ref(name, "signed", 0)
    Ho, Wo = ref.shape[1:3]
    wo, w = Wo - 1, c.W - 1
    assert wo * c.S + c.KW > c.W  # the last window is clipped at the far edge; w is its last column
    # the window where its last tap (kh = 2, the column at the edge) weighs most against the bound
    score = (x[:, 2:2 * Ho + 1:2, w].double().abs() / 9) / bound[:, :, wo]
    n, ho, ch = [int(i) for i in torch.unravel_index(score.argmax(), score.shape)]
    assert score[n, ho, ch] > 4
    y = PB.emulate_forward(x, *_geo(c), c.mode)
    assert y[n, ho, wo, ch] == _window_f32(x, c, n, ho, wo, ch)
    y[n, ho, wo, ch] = _window_f32(x, c, n, ho, wo, ch, drop=(2 * ho + 2, w))
    _only(y, ref, bound, [_flat(ref.shape, n, ho, wo, ch)])


def test_the_clipped_tap_count_as_divisor_leaves_the_bound():
    """avg divides by KH KW even where the window is clipped"""
    name = "k3s2_avg_9x8"
    c = PB.CASES[name]
    x = PB.data(name, "signed")
    ref, bound = PB.forward_ref(name, "signed", 0)
    wo = ref.shape[2] - 1
    K = PB.tap_count(x.shape, *_geo(c))
    assert K[0, 0, wo, 0] == 6 and K[0, 0, 0, 0] == 9
    n, ho, ch = [int(i) for i in torch.unravel_index((ref[:, :, wo].abs() / bound[:, :, wo]).argmax(), ref[:, :, wo].shape)]
    y = PB.emulate_forward(x, *_geo(c), c.mode)
    y[n, ho, wo, ch] = _window_f32(x, c, n, ho, wo, ch, clipped_divisor=True)
    _only(y, ref, bound, [_flat(ref.shape, n, ho, wo, ch)])


def test_a_tie_routed_to_the_second_maximum_leaves_the_bound():
    name = "k3s2_max_9x8"
    c = PB.CASES[name]
    x, dy = PB.data(name, "signed"), PB.inputs(name)["dy"]
    y, st = PB.forward_ref(name, "signed", 0)
    second = torch.full(st.shape, 255, dtype=torch.uint8)  # the second tap equal to the maximum
    taps, _ = PB._taps(x.shape, *_geo(c))
    for kh, kw, so, si in taps:
        t = kh * c.KW + kw
        hit = (x[si].double() == y[so]) & (st[so] < t) & (second[so] == 255)
        second[so] = torch.where(hit, torch.full_like(second[so], t), second[so])
    tied = second != 255
    assert int(tied.sum()) > 100, "the data has too few ties"
    idx = torch.unravel_index((dy.double().abs() * tied).argmax(), st.shape)
    n, ho, wo, ch = [int(i) for i in idx]
    bad_st = st.clone()
    bad_st[n, ho, wo, ch] = second[n, ho, wo, ch]
    zero = torch.zeros(st.shape, dtype=torch.float64)
    _only(bad_st, st.double(), zero, [_flat(st.shape, n, ho, wo, ch)])
    ref, bound = PB.backward_ref(name, "signed", 0, 0)
    dx = PB.emulate_backward(x, bad_st, dy, *_geo(c), "max", 0)
    pix = []
    for t in (int(st[n, ho, wo, ch]), int(second[n, ho, wo, ch])):
        pix.append(_flat(ref.shape, n, ho * c.S - c.P + t // c.KW, wo * c.S - c.P + t % c.KW, ch))
    _only(dx, ref, bound, pix)


def test_a_border_pixel_with_its_window_range_off_by_one_leaves_the_bound():
    name = "k3s1_sum_6x5"
    c = PB.CASES[name]
    x, dy = PB.data(name, "signed"), PB.inputs(name)["dy"]
    ref, bound = PB.backward_ref(name, "signed", 0, 0)
    Ho, Wo = dy.shape[1:3]
    h = c.H - 1  # the last row: covered by window row Ho - 1 alone; the planted range ends one short
    assert c.P == 0 and c.S == 1 and h - c.KH + 1 == Ho - 1
    score = dy[:, Ho - 1, Wo - 1].double().abs() / bound[:, h, c.W - 1]
    n, ch = [int(i) for i in torch.unravel_index(score.argmax(), score.shape)]
    dx = PB.emulate_backward(x, None, dy, *_geo(c), "sum", 0)
    assert dx[n, h, c.W - 1, ch] == dy[n, Ho - 1, Wo - 1, ch]  # the corner pixel has that one window
    dx[n, h, c.W - 1, ch] = 0.0
    _only(dx, ref, bound, [_flat(ref.shape, n, h, c.W - 1, ch)])


@pytest.mark.parametrize("name", ["c3_max_k3s2", "k5s2_avg_9x12p2"])
def test_an_unwritten_element_of_the_last_image_leaves_the_bound(name):
    c = PB.CASES[name]
    x, dy = PB.data(name, "signed"), PB.inputs(name)["dy"]
    st = PB.forward_ref(name, "signed", 0)[1] if c.mode == "max" else None
    ref, bound = PB.backward_ref(name, "signed", 0, 0)
    dx = PB.emulate_backward(x, st, dy, *_geo(c), c.mode, 0)
    last = (c.N - 1, c.H - 1, c.W - 1, c.C - 1)
    dx[last] = PREFILL
    _only(dx, ref, bound, [_flat(ref.shape, *last)])
    dx[last] = float("nan")
    _only(dx, ref, bound, [_flat(ref.shape, *last)])
    if c.mode == "max":
        y_ref, _ = PB.forward_ref(name, "signed", 0)
        y = y_ref.clone()
        y[c.N - 1, -1, -1, -1] = float("nan")
        n, _, bad = PB.violations(y, y_ref, torch.zeros_like(y_ref))
        assert n == 1 and bad.tolist() == [y_ref.numel() - 1]


def test_an_ignored_bit_7_leaves_the_bound():
    name = "k3s2_max_9x8"
    c = PB.CASES[name]
    x, dy = PB.data(name, "nonneg"), PB.inputs(name)["dy"]
    st = PB.forward_ref(name, "nonneg", 2)[1]
    ref, bound = PB.backward_ref(name, "nonneg", 2, 2)
    marked = st >= 128
    assert bool(marked.any())
    n, ho, wo, ch = [int(i) for i in torch.unravel_index((dy.double().abs() * marked).argmax(), st.shape)]
    bad_st = st.clone()
    bad_st[n, ho, wo, ch] &= 127  # the all-(<= 0) window routes its gradient after all
    t = int(bad_st[n, ho, wo, ch])
    dx = PB.emulate_backward(x, bad_st, dy, *_geo(c), "max", 2)
    _only(dx, ref, bound, [_flat(ref.shape, n, ho * c.S - c.P + t // c.KW, wo * c.S - c.P + t % c.KW, ch)])


def test_a_last_strip_row_taken_from_the_row_above_leaves_the_bound():
    name = "k3s1_max_h5p1"
    c = PB.CASES[name]
    y_ref, st_ref = PB.forward_ref(name, "signed", 0)
    Ho = y_ref.shape[1]
    assert Ho % PB.S1K3_R == 1  # the last strip holds one row
    zero = torch.zeros_like(y_ref)
    for ref in (y_ref, st_ref.double()):
        got = ref.clone()
        got[c.N - 1, Ho - 1] = ref[c.N - 1, Ho - 2]
        want = torch.nonzero((got != ref).reshape(-1)).reshape(-1).tolist()
        assert want and all(i >= _flat(ref.shape, c.N - 1, Ho - 1, 0, 0) for i in want)
        n, worst, bad = PB.violations(got, ref, zero)
        assert sorted(bad.tolist()) == want and worst == float("inf")


# ----------------------------------------------------------------- the formulas, by hand
def test_the_bound_is_the_stated_formula():
    u, e = 2.0 ** -8, 2.0 ** -23
    x = torch.tensor([1.5, -2.0, 0.25]).to(torch.bfloat16).reshape(1, 1, 3, 1)
    dy = torch.tensor([1.0, -3.0]).to(torch.bfloat16).reshape(1, 1, 2, 1)
    geo = (1, 2, 1, 0)  # windows {x0, x1} and {x1, x2}
    assert PB.out_size(3, 2, 1, 0) == 2 and PB.windows_over_a_pixel(1, 2, 1) == 2

    def check(ref, bound, want, A, r):
        assert ref.reshape(-1).tolist() == want
        for i, a in enumerate(A):
            assert abs(bound.reshape(-1)[i].item() - (u * (abs(want[i]) + r * e * a) + r * e * a)) < 1e-18

    check(*PB.sum_forward_ref(x, *geo, "sum"), [-0.5, -1.75], [3.5, 2.25], 2 + PB.C_SUM)
    check(*PB.sum_forward_ref(x, *geo, "avg"), [-0.25, -0.875], [1.75, 1.125], 2 + PB.C_AVG)
    check(*PB.sum_forward_ref(x, *geo, "sum", 1), [1.5, 0.25], [1.5, 0.25], 2 + PB.C_SUM)
    y, st = PB.max_forward_ref(x, *geo, 2)
    assert y.reshape(-1).tolist() == [1.5, 0.25] and st.reshape(-1).tolist() == [0, 1]
    check(*PB.max_backward_ref(x, st, dy, *geo, 2), [1.0, 0.0, -3.0], [1.0, 0.0, 3.0], 4)
    check(*PB.sum_backward_ref(x, dy, *geo, "sum"), [1.0, -2.0, -3.0], [1.0, 4.0, 3.0], 4)
    check(*PB.sum_backward_ref(x, dy, *geo, "avg"), [0.5, -1.0, -1.5], [0.5, 2.0, 1.5], 6)
    check(*PB.sum_backward_ref(x, dy, *geo, "sum", 1), [1.0, 0.0, -3.0], [1.0, 0.0, 3.0], 4)
    # a tie: both inputs of the first window equal its maximum
    xt = torch.tensor([1.5, 1.5, 0.25]).to(torch.bfloat16).reshape(1, 1, 3, 1)
    yt, stt = PB.max_forward_ref(xt, *geo)
    assert yt.reshape(-1).tolist() == [1.5, 1.5] and stt.reshape(-1).tolist() == [0, 0]
    check(*PB.max_backward_ref(xt, stt, dy, *geo), [1.0, -3.0, 0.0], [1.0, 3.0, 0.0], 4)
    check(*PB.tie_all_backward_ref(xt, yt, dy, *geo), [1.0, -2.0, 0.0], [1.0, 4.0, 0.0], 4)
    # an all-negative window is marked and routes nothing
    xm = torch.tensor([-1.0, -0.0, 0.5]).to(torch.bfloat16).reshape(1, 1, 3, 1)
    ym, stm = PB.max_forward_ref(xm, *geo, 2)
    assert ym.reshape(-1).tolist() == [0.0, 0.5] and stm.reshape(-1).tolist() == [129, 1]
    check(*PB.max_backward_ref(xm, stm, dy, *geo, 2), [0.0, 0.0, -3.0], [0.0, 0.0, 3.0], 4)


# ----------------------------------------------------------------- windows wholly in the padding
def _zoo_pool_geometries():
    from cxxnet_amd.layers.std import PoolingLayer
    from cxxnet_amd.models import available, load_conf
    from cxxnet_amd.nnet import NetTrainer
    out = []
    for model in available():
        tr = NetTrainer()
        for k, v in [(k, v) for k, v in load_conf(model) if k != "dev"] + [("batch_size", "1"), ("dev", "cpu"),
                                                                           ("silent", "1")]:
            tr.set_param(k, v)
        tr.net_cfg.configure(tr.cfg)
        net = tr._make_net()
        net.init_net()
        net._connect()  # shape inference only: no parameter is allocated
        for conn in net.connections:
            if isinstance(conn.layer, PoolingLayer):
                lp = conn.layer.lp
                _, _, h, w = conn.nodes_in[0].shape
                out.append((model, (h, lp.kernel_height, lp.stride, lp.pad_y), (w, lp.kernel_width, lp.stride, lp.pad_x)))
    return out


def test_has_empty_window():
    assert PB.has_empty_window(5, 2, 2, 1)       # 4 windows, the last starts at row 5
    assert not PB.has_empty_window(6, 2, 2, 1)   # 4 windows, the last holds row 5
    assert not PB.has_empty_window(5, 2, 2, 0)
    assert PB.has_empty_window(5, 2, 1, 2)       # the first window ends before row 0
    assert not PB.has_empty_window(6, 3, 1, 2) and not PB.has_empty_window(7, 3, 2, 2)
    for H in range(1, 12):
        for K in range(1, 6):
            for S in range(1, 5):
                for P in range(0, 4):
                    if K > H + 2 * P:
                        continue
                    rows = [[h for h in range(o * S - P, o * S - P + K) if 0 <= h < H] for o in range(PB.out_size(H, K, S, P))]
                    assert PB.has_empty_window(H, K, S, P) == any(not r for r in rows), (H, K, S, P)
    with pytest.raises(AssertionError, match="wholly in the padding"):
        PB.assert_no_empty_window("bad", PB.Case(1, 5, 6, 8, 2, 2, 2, 1, "max", "", ""))
    geos = _zoo_pool_geometries()
    assert len(geos) >= 20 and len({g[0] for g in geos}) >= 7
    for model, gh, gw in geos:
        assert not PB.has_empty_window(*gh) and not PB.has_empty_window(*gw), (model, gh, gw)
