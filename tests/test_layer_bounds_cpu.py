"""tests/layer_bounds.py judged without a GPU, on the inputs of the GPU tests (tests/layer_cases.py).

Not too tight: every kernel is emulated in numpy fp32 in its own order of operations (chan_reduce:
four row lanes per block, the lane sums, then the blocks added in two different orders; the
updaters in their fma form and unfused) and stays inside the bound on every GPU case.
Not too loose: each defect of DEFECTS, injected into the emulation, leaves the bound in at least
one element.  The closed forms of the prelu / insanity backward equal float64 autograd.

Worst d / bound of the emulations (this file's own output, `pytest -s`):
  batch_norm   mean 0.12  inv 0.075  y 0.99  xhat 0.99  dx 0.97  gslope 0.050  gbias 0.051  affine 0.995
  prelu        y 0.995  dx 0.99  gslope 0.0071      insanity  y 0.98  dx 0.98
  insanity_max_pooling  dx 0.98 (forward exact)
  activations  forward 0.98  backward 0.995         dropout  0.97
  fused_update sgd w 0.47 m1 0.30 wb 0.99   nag w 0.28 m1 0.30 wb 0.975   adam w 0.48 m1 0.44 m2 0.17 wb 0.995
(Just under 1 is the bf16 store itself: a value just above a power of two is moved by up to
U = 2^-8 of itself.  The fp32 results sit well inside: their bounds charge u per operation where
round to nearest gives u / 2, and worst-case sums.)"""
import functools

import numpy as np
import pytest
import torch

import layer_bounds as LB
import layer_cases as LC

f32 = np.float32
WORST = {}


def _note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), v)


def _bf(a):
    """fp32 array -> its bf16 rounding (round to nearest even), as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).float().numpy()


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _np(t):
    return t.float().numpy()


def _fma(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _check(got, ref, bound, key, axes="rc"):
    _note(key, LB.assert_within(_t(got).reshape(ref.shape), ref, bound, key, axes=axes))


def _violates(got, ref, bound):
    return LB.violations(_t(got).reshape(ref.shape), ref, bound)[0] > 0


# ------------------------------------------------------------------------------------ chan_reduce, batch_norm
def chan_reduce(x, gy, mean, mode, order=1, det=False, skip_row=None):
    """csrc/kernels/layer_kernels.hip chan_reduce + cxn_chan_reduce's block geometry, [nq][C] fp32.
    order: +1 blocks arrive at the atomics first to last, -1 last to first."""
    R, C = x.shape
    rb = (R + 255) // 256
    cg = (C + 63) // 64
    rb = min(rb, 1024 // cg + 1)
    if det:
        rb = 1
    rpb = (R + rb - 1) // rb
    rb = max((R + rpb - 1) // rpb, 1)
    nq = 3 if mode == 2 else 1
    out = np.zeros((nq, C), f32)
    m = mean if mean is not None else np.zeros(C, f32)
    for b in list(range(rb))[::order]:
        lanes = np.zeros((nq, 4, C), f32)
        for r in range(b * rpb, min(R, (b + 1) * rpb)):
            if r == skip_row:
                continue
            rl = (r - b * rpb) & 3
            if mode == 0:
                lanes[0, rl] += x[r]
            elif mode == 1:
                d = x[r] - m
                lanes[0, rl] += d * d
            elif mode == 2:
                d = x[r] - m
                lanes[0, rl] += d
                lanes[1, rl] += gy[r]
                lanes[2, rl] += gy[r] * d
            else:
                lanes[0, rl] += np.minimum(x[r], f32(0)) * gy[r]
        out += ((lanes[:, 0] + lanes[:, 1]) + lanes[:, 2]) + lanes[:, 3]
    return out


def bn_emulate(c, eps, order=1, det=False, skip_row=None, drop_C=False, drop_B=False):
    x, gy = _np(c["x"]), _np(c["gy"])
    slope, bias = c["slope"].numpy(), c["bias"].numpy()
    R, C = x.shape
    scale, eps = f32(1) / f32(R), f32(eps)
    mean = chan_reduce(x, None, None, 0, order, det, skip_row)[0] * scale
    inv = f32(1) / np.sqrt(chan_reduce(x, None, mean, 1, order, det)[0] * scale + eps)
    h = (x - mean) * inv
    y, xhat = _bf(h * slope + bias), _bf(h)
    s0, s1, s2 = chan_reduce(x, gy, mean, 2, order, det)
    ve = f32(1) / (inv * inv)
    gvar = slope * s2 * f32(-0.5) * inv / ve
    gexp = -slope * s1 * inv + gvar * scale * (f32(-2) * s0)
    gslope, gbias = c["gs0"].numpy() + s2 * inv, c["gb0"].numpy() + s1
    cA, cB, cC = slope * inv, gvar * scale * f32(2), gexp * scale
    if drop_B:
        cB = np.zeros_like(cB)
    if drop_C:
        cC = np.zeros_like(cC)
    dx = _bf(gy * cA + (x - mean) * cB + cC)
    return dict(mean=mean, inv=inv, y=y, xhat=xhat, dx=dx, gslope=gslope, gbias=gbias)


@functools.lru_cache(maxsize=None)
def _bn_refs(name, eps):
    c = LC.bn_inputs(name)
    return c, LB.bn_forward_ref(c["x"], c["slope"], c["bias"], eps), \
        LB.bn_backward_ref(c["gy"], c["x"], c["slope"], c["gs0"], c["gb0"], eps)


@pytest.mark.parametrize("name,eps", LC.BN_RUNS, ids=LC.BN_IDS)
def test_batch_norm_emulation_inside_the_bounds(name, eps):
    c, fwd, bwd = _bn_refs(name, eps)
    for order, det in ((1, False), (-1, False), (1, True)):
        e = bn_emulate(c, eps, order, det)
        for k, ax in (("mean", "c"), ("inv", "c"), ("y", "rc"), ("xhat", "rc")):
            _check(e[k], *fwd[k], "bn " + k, ax)
        for k, ax in (("dx", "rc"), ("gslope", "c"), ("gbias", "c")):
            _check(e[k], *bwd[k], "bn " + k, ax)
    assert torch.isfinite(fwd["y"][1]).all() and torch.isfinite(bwd["dx"][1]).all()
    # the bias layer's use of the forward kernel: mean 0, inv 1, slope 1
    C = c["C"]
    zero, one = torch.zeros(C), torch.ones(C)
    x = _np(c["x"])
    _check(_bf((x - f32(0)) * f32(1) * f32(1) + c["bias"].numpy()), *LB.affine_ref(c["x"], zero, one, one, c["bias"]),
           "bn affine")


@pytest.mark.parametrize("name,eps", LC.BN_RUNS, ids=LC.BN_IDS)
def test_batch_norm_defects_leave_the_bounds(name, eps):
    c, fwd, bwd = _bn_refs(name, eps)
    if name != "const":  # (leaving a row out of a constant channel's sum is seen in every other channel)
        e = bn_emulate(c, eps, skip_row=c["R"] // 2)
        assert _violates(e["mean"], *fwd["mean"]), "one row left out of the sum"
    assert _violates(bn_emulate(c, eps, drop_C=True)["dx"], *bwd["dx"]), "Cc dropped"
    assert _violates(bn_emulate(c, eps, drop_B=True)["dx"], *bwd["dx"]), "(x - mean) B dropped"


def test_two_pass_meets_the_variance_bound_on_case_c():
    c = LC.bn_inputs("c")
    s = LB.BN.stats_ref(c["x"])
    x = _np(c["x"])
    mean = chan_reduce(x, None, None, 0)[0] * (f32(1) / f32(130))
    var = chan_reduce(x, None, mean, 1)[0] * (f32(1) / f32(130))
    LB.assert_within(_t(var), s["var"], s["e_var"], "two-pass var", axes="c")


# ------------------------------------------------------------------------------------ prelu, insanity
def _u32(n, seed, counter):
    return LB.draws(n, seed, torch.tensor([counter], dtype=torch.int32)).numpy().astype(f32)


def prelu_emulate(p, rnd, v, by_channel=False):
    x, slope = _np(p["x"]), p["slope"].numpy()
    rows, C = x.shape
    m = np.broadcast_to(slope, (rows, C))
    if rnd > 0:
        u = _u32(rows * C, LC.PRELU_SEED, LC.PRELU_COUNTER)
        u = np.broadcast_to(u[:C], (rows, C)) if by_channel else u.reshape(rows, C)
        m = slope * (f32(1) + u * f32(rnd) * f32(2) - f32(rnd))
    m = np.minimum(np.maximum(m, f32(0)), f32(1))
    return _bf(np.where(x > 0, v, v * m))


@pytest.mark.parametrize("rnd", LC.PRELU_RND)
@pytest.mark.parametrize("rows,C", LC.PRELU_SHAPES)
def test_prelu_emulation_and_defect(rows, C, rnd):
    p = LC.prelu_inputs(rows, C)
    ctr = torch.tensor([LC.PRELU_COUNTER], dtype=torch.int32)
    fw = LB.prelu_ref(p["x"], p["x"], p["slope"], rnd, LC.PRELU_SEED, ctr)
    bw = LB.prelu_ref(p["x"], p["gy"], p["slope"], rnd, LC.PRELU_SEED, ctr)
    _check(prelu_emulate(p, rnd, _np(p["x"])), *fw, "prelu y")
    _check(prelu_emulate(p, rnd, _np(p["gy"])), *bw, "prelu dx")
    for order in (1, -1):
        s = chan_reduce(_np(p["x"]), _np(p["gy"]), None, 3, order)[0]
        _check(p["gs0"].numpy() + s, *LB.prelu_gslope_ref(p["x"], p["gy"], p["gs0"]), "prelu gslope", "c")
    if rnd > 0 and rows > 1:
        assert _violates(prelu_emulate(p, rnd, _np(p["x"]), by_channel=True), *fw), "draw at index c"
        assert _violates(prelu_emulate(p, rnd, _np(p["gy"]), by_channel=True), *bw), "draw at index c (backward)"


def insanity_emulate(sel, v, train, wrap=0):
    n = sel.size
    if train:
        u = _u32(n, LC.INSANITY_SEED, LC.INSANITY_COUNTER)
        if wrap:
            u = u[np.arange(n) % wrap]
        d = f32(LC.INSANITY_LB) + u * (f32(LC.INSANITY_UB) - f32(LC.INSANITY_LB))
    else:
        d = np.full(n, f32(0.5) * (f32(LC.INSANITY_LB) + f32(LC.INSANITY_UB)), f32)
    return _bf(np.where(sel > 0, v, v / d))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("n", LC.INSANITY_N)
def test_insanity_emulation_and_defect(n, train):
    x, gy = LC.insanity_inputs(n)
    ctr = torch.tensor([LC.INSANITY_COUNTER], dtype=torch.int32)
    args = (LC.INSANITY_LB, LC.INSANITY_UB, train, LC.INSANITY_SEED, ctr)
    fw = LB.insanity_ref(x, x, *args)
    y = insanity_emulate(_np(x), _np(x), train)
    _check(y, *fw, "insanity y", "i")
    bw = LB.insanity_ref(torch.from_numpy(y), gy, *args)
    _check(insanity_emulate(y, _np(gy), train), *bw, "insanity dx", "i")
    if train and n > 8:  # the draw of channel i % 8 in place of element i's
        assert _violates(insanity_emulate(_np(x), _np(x), train, wrap=8), *fw), "draw at index c"


def test_prelu_and_insanity_closed_forms_match_autograd():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(9, 4, generator=gen).to(torch.bfloat16)
    gy = torch.randn(9, 4, generator=gen).to(torch.bfloat16)
    slope = torch.rand(4, generator=gen) * 0.8 + 0.1  # inside (0, 1): the clamp is not active
    xd, sd = x.double().requires_grad_(), slope.double().requires_grad_()
    y = torch.where(xd > 0, xd, xd * sd.clamp(0, 1))
    y.backward(gy.double())
    ref, _ = LB.prelu_ref(x, gy, slope, 0.0, 0)
    assert torch.allclose(ref, xd.grad, rtol=1e-12, atol=0)
    gs, _ = LB.prelu_gslope_ref(x, gy, torch.zeros(4))
    assert torch.allclose(gs, sd.grad, rtol=1e-12, atol=1e-14)
    # with noise: the gradient with respect to x under the reference's own mask
    m, _ = LB.prelu_mask_ref(9, 4, slope, 0.3, 5)
    xd = x.double().requires_grad_()
    torch.where(xd > 0, xd, xd * m).backward(gy.double())
    assert torch.allclose(LB.prelu_ref(x, gy, slope, 0.3, 5)[0], xd.grad, rtol=1e-12, atol=0)
    for train in (True, False):
        d, _ = LB.insanity_div_ref(36, 3.0, 8.0, train, 7)
        xd = x.double().reshape(-1).requires_grad_()
        yy = torch.where(xd > 0, xd, xd / d)
        yy.backward(gy.double().reshape(-1))
        ref, _ = LB.insanity_ref(yy.detach(), gy, 3.0, 8.0, train, 7)
        assert torch.allclose(ref, xd.grad, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------ insanity pooling
def ins_pool_bwd_emulate(shifted, ypool, gy, K, S):
    """ins_pool_bwd's own loop: the covering windows from py0 / py1, an fp32 sum in window order"""
    N, H, W, C = shifted.shape
    Ho, Wo = ypool.shape[1], ypool.shape[2]
    dx = np.zeros((N, H, W, C), f32)
    for yy in range(H):
        for xx in range(W):
            py0 = 0 if yy < K else (yy - K + S) // S
            px0 = 0 if xx < K else (xx - K + S) // S
            acc = np.zeros((N, C), f32)
            for py in range(py0, min((yy + S) // S, Ho)):
                for px in range(px0, min((xx + S) // S, Wo)):
                    acc = acc + np.where(shifted[:, yy, xx] == ypool[:, py, px], gy[:, py, px], f32(0))
            dx[:, yy, xx] = acc
    return _bf(dx)


@pytest.mark.parametrize("keep", LC.INS_POOL_KEEP)
@pytest.mark.parametrize("shape", LC.INS_POOL_SHAPES)
def test_ins_pool_emulation_and_defect(shape, keep):
    N, H, W, C, K, S = shape
    x, gy = LC.ins_pool_inputs(*shape)
    ctr = torch.tensor([LC.INS_POOL_COUNTER], dtype=torch.int32)
    sh = LB.ins_pool_shifted(x, keep, LC.INS_POOL_SEED, ctr)
    y = LB.ins_pool_forward_ref(sh, K, S)
    assert tuple(y.shape) == tuple(gy.shape)
    if keep == 1.0:
        assert torch.equal(sh, x.double())
    ref, bound = LB.ins_pool_backward_ref(sh, y, gy, K, S)
    _check(ins_pool_bwd_emulate(sh.numpy().astype(f32), y.numpy().astype(f32), _np(gy), K, S), ref, bound,
           "ins_pool dx", "nhwc")
    assert float((bound == 0).double().mean()) > 0.2  # most elements are no window's max: exactly 0
    if keep < 1.0:  # an unclamped shift reads the neighbouring row / image at the border
        bad = LB.ins_pool_shifted(x, keep, LC.INS_POOL_SEED, ctr, clamp=False)
        assert not torch.equal(LB.ins_pool_forward_ref(bad, K, S), y), "shift not clamped at the border"


# ------------------------------------------------------------------------------------ activations, dropout
def act_emulate(kind, x, b):
    with np.errstate(all="ignore"):
        if kind == "relu":
            return _bf(np.maximum(x, f32(0)))
        if kind == "xelu":
            return _bf(np.where(x > 0, x, x / f32(b)))
        if kind == "sigmoid":
            t = (-x) * f32(1.4426950408889634)  # __expf(t) = exp2(t log2 e)
            e = np.exp2(t.astype(np.float64)).astype(f32)
            return _bf(f32(1) / (f32(1) + e))
        return _bf(np.tanh(x.astype(np.float64)).astype(f32))


def act_bwd_emulate(kind, y, dy, b):
    if kind == "relu":
        gr = np.where(y > 0, f32(1), f32(0))
    elif kind == "sigmoid":
        gr = y * (f32(1) - y)
    elif kind == "tanh":
        gr = f32(1) - y * y
    else:
        gr = np.where(y > 0, f32(1), f32(1) / f32(b))
    return _bf(dy * gr)


@pytest.mark.parametrize("n", LC.ACT_N)
@pytest.mark.parametrize("kind", LB.ACT_KINDS)
def test_activation_emulation(kind, n):
    x, dy = LC.act_inputs(n)
    ref, bound = LB.act_forward_ref(kind, x, LC.XELU_B)
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all()
    y = act_emulate(kind, _np(x), LC.XELU_B)
    _check(y, ref, bound, "act forward", "i")
    rb, bb = LB.act_backward_ref(kind, torch.from_numpy(y), dy, LC.XELU_B)
    assert torch.isfinite(rb).all() and torch.isfinite(bb).all()
    _check(act_bwd_emulate(kind, y, _np(dy), LC.XELU_B), rb, bb, "act backward", "i")


@pytest.mark.parametrize("pkeep", LC.DROPOUT_PKEEP)
@pytest.mark.parametrize("n", LC.DROPOUT_N)
def test_dropout_emulation_and_defect(n, pkeep):
    x = LC.dropout_inputs(n)
    ctr = torch.tensor([LC.DROPOUT_COUNTER], dtype=torch.int32)
    ref, bound, keep = LB.dropout_ref(x, pkeep, LC.DROPOUT_SEED, ctr)
    t = float(f32(pkeep)) * 4294967296.0  # dropout_thresh of nn_shared.h
    thresh = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    h = LB._hash_u32(torch.arange(n, dtype=torch.int64), LB.effective_seed(LC.DROPOUT_SEED, ctr)).numpy()

    def emul(hh):
        return _bf(np.where(hh < thresh, _np(x) * (f32(1) / f32(pkeep)), f32(0)))
    _check(emul(h), ref, bound, "dropout", "i")
    assert abs(float(keep.double().mean()) - pkeep) < (0.5 if n < 100 else 0.03)
    if pkeep < 1.0 and n > 8:
        assert _violates(emul(np.roll(h, 1)), ref, bound), "mask shifted by one element"
        assert not torch.equal(LB.dropout_keep_ref(n, pkeep, LC.DROPOUT_SEED, ctr, shift=1), keep)


# ------------------------------------------------------------------------------------ fused_update
def _clipg(gv, c):
    with np.errstate(all="ignore"):
        return gv if c == 0 else np.where(np.isnan(gv), f32(0), np.minimum(np.maximum(gv, -c), c))


def update_emulate(algo, st, segs, fused, d1=0.1, d2=0.001, defect=None):
    """step1 of optim_kernels.hip per segment; fused: the fma form.  Returns w, m1, m2, wb (fp32)."""
    w, gr, m1, m2 = (st[k].numpy().copy() for k in ("w", "g", "m1", "m2"))
    d1, d2 = f32(d1), f32(d2)
    one = f32(1)
    for j, (off, n, lr, wd, mom, clip) in enumerate(segs):
        if defect == "neighbour_lr" and n:
            lr = segs[(j + 1) % len(segs)][2]
        lr, wd, mom, clip = f32(lr), f32(wd), f32(mom), f32(clip)
        if defect == "no_wd":
            wd = f32(0)
        if defect == "no_tail" and n:
            n -= 1
        sl = slice(off, off + n)
        wv, gv, mv = w[sl], gr[sl], m1[sl]
        with np.errstate(all="ignore"):
            if algo == "sgd":
                gv = _clipg(gv, clip)
                mn = _fma(mom, mv, -(lr * _fma(wd, wv, gv))) if fused else mom * mv - lr * (gv + wd * wv)
                wn = wv + mn
            elif algo == "nag":
                mn = _fma(mom, mv, -(lr * _fma(wd, wv, gv))) if fused else mom * mv - lr * (gv + wd * wv)
                old = np.zeros_like(mv) if defect == "nag_no_old" else mv
                wn = _fma(-mom, old, _fma(one + mom, mn, wv)) if fused else wv + (one + mom) * mn - mom * old
            else:
                if wd > 0:
                    sgn = -wd if defect != "adam_sign" else wd
                    gv = _fma(sgn, wv, gv) if fused else gv + sgn * wv
                m2v = m2[sl]
                mn = _fma(d1, gv - mv, mv) if fused else mv + d1 * (gv - mv)
                m2n = _fma(d2, _fma(gv, gv, -m2v), m2v) if fused else m2v + d2 * (gv * gv - m2v)
                q = mn / (np.sqrt(m2n) + f32(1e-8))
                wn = _fma(-lr, q, wv) if fused else wv - lr * q
                m2[sl] = m2n
        w[sl], m1[sl] = wn, mn
    return dict(w=w, m1=m1, m2=m2, wb=_bf(w))


def _update_tables():
    return [("table",) + LC.update_table(), ("chunk49",) + LC.chunk_table(49), ("chunk97",) + LC.chunk_table(97)]


@pytest.mark.parametrize("algo", ["sgd", "nag", "adam"])
def test_update_emulation_inside_the_bounds(algo):
    for name, size, segs in _update_tables():
        st = LC.update_state(size, segs, algo)
        ref = LB.update_ref(algo, st["w"], st["g"], st["m1"], st["m2"] if algo == "adam" else None, segs)
        assert all(torch.isfinite(ref[k]).all() for k in ("w", "m1", "e_w", "e_m1", "e_wb"))
        for fused in (True, False):
            e = update_emulate(algo, st, segs, fused)
            _check(e["w"], ref["w"], ref["e_w"], algo + " w", "i")
            _check(e["m1"], ref["m1"], ref["e_m1"], algo + " m1", "i")
            _check(e["wb"], ref["w"], ref["e_wb"], algo + " wb", "i")
            if algo == "adam":
                _check(e["m2"], ref["m2"], ref["e_m2"], algo + " m2", "i")


DEFECTS = [("sgd", "no_wd"), ("nag", "no_wd"), ("sgd", "neighbour_lr"), ("nag", "neighbour_lr"), ("adam", "neighbour_lr"),
           ("sgd", "no_tail"), ("nag", "no_tail"), ("adam", "no_tail"), ("nag", "nag_no_old"), ("adam", "adam_sign")]


@pytest.mark.parametrize("algo,defect", DEFECTS)
def test_update_defects_leave_the_bounds(algo, defect):
    for name, size, segs in _update_tables():
        st = LC.update_state(size, segs, algo)
        ref = LB.update_ref(algo, st["w"], st["g"], st["m1"], st["m2"] if algo == "adam" else None, segs)
        e = update_emulate(algo, st, segs, True, defect=defect)
        assert _violates(e["w"], ref["w"], ref["e_w"]), (name, "w")
        # (the first moment does not see NAG's look-ahead term, nor Adam's lr)
        m1_blind = defect == "nag_no_old" or (algo, defect) == ("adam", "neighbour_lr")
        assert _violates(e["m1"], ref["m1"], ref["e_m1"]) or m1_blind, (name, "m1")
        if defect == "no_wd":  # and in every single segment with a weight decay, not only somewhere
            d = (_t(e["w"]) - ref["w"]).abs()
            for off, n, lr, wd, mom, clip in segs:
                if wd > 0 and n:
                    assert bool((d[off:off + n] > ref["e_w"][off:off + n]).any()), (name, off)


def test_update_ref_leaves_the_gaps_alone():
    size, segs = LC.update_table()
    st = LC.update_state(size, segs, "sgd")
    ref = LB.update_ref("sgd", st["w"], st["g"], st["m1"], None, segs)
    gap = ~ref["inside"]
    assert int(gap.sum()) > 100
    assert bool((ref["w"][gap] == LC.SENTINEL).all()) and bool((ref["e_w"][gap] == 0).all())


def test_print_worst_ratios():
    """(runs last in this file: the figures of the module docstring)"""
    for k in sorted(WORST):
        print("worst d/bound %-16s %.3g" % (k, WORST[k]))
        assert WORST[k] <= 1.0
