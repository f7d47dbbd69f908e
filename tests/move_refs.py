"""References, case lists and guards for the kernels that move data between the layers
(csrc/kernels/copy_kernels.hip, layout_kernels.hip and reduce_kernels.hip: transposes, weight
flip, concat, channel copies, pads, casts, split forward / backward, layout conversion, the image input stage) and for the column sums that are
every bias gradient.  Everything here runs on the CPU and is written with explicit index
arithmetic, independent of cxxnet_amd.ops and of U8Images.to_float.

Three kinds of expectation, none of them tuned:

  bits     A permutation or a copy can only be right or wrong bit for bit.  So can an op that
           rounds once: bf16(fl32(a + b)), bf16(fl32(x * scale)) are the same IEEE operation in
           torch (float32 arithmetic, round-to-nearest-even conversion; common.h f2bf is RNE), and
           none of them pairs a multiply with an add, so FMA contraction cannot change them.
  bound    The image stage's ((d - m) * ct + il) * scale may or may not be contracted to an FMA.
           With ref in float64 from the exact fp32 operands and A = (|d - m| |ct| + |il|) |scale|,
               bound = u (|ref| + 4 2^-23 A) + 4 2^-23 A,   u = 2^-8:
           four fp32 roundings (subtract, multiply, add, multiply; three when fused) at the
           doubled unit 2^-23 of tests/bounds.py, each of an intermediate no larger than A, then
           the bf16 store.
  integer  Column sums of bf16 values that are small integers, onto an integer db0, with
               max_c (|db0[c]| + sum_r |dy[r][c]|) < 2^24:
           every fp32 partial sum in any order (atomics included) is then an exactly representable
           integer, so the result must EQUAL the integer sum -- a dropped, doubled or misplaced
           row fails at any row count.  Random inputs get the bias-gradient bound of
           bounds.dbias_ref, (R + 2) 2^-23 (sum |dy| + |db0|), only up to R = 1500 rows."""
import functools

import torch

U_BF16 = 2.0 ** -8
EPS_F32 = 2.0 ** -23
SENTINEL = -3.0
COLSUM_BOUND_MAX_ROWS = 1500  # the limit tests/bounds.py states for its (K + 2) 2^-23 bounds
BF16 = torch.bfloat16


# ------------------------------------------------------------------ bits and guards
def bits(t):
    """integer view (same width) of a tensor: what equality is asserted on"""
    t = t.detach().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits_equal(got, want, what="output"):
    """torch.equal on the bit patterns; a failure names how many elements differ and where."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape,
                                                                               want.shape)
    a, b = bits(got), bits(want)
    if torch.equal(a, b):
        return
    bad = torch.nonzero(a != b)
    f = tuple(bad[0].tolist())
    raise AssertionError("%s: %d of %d elements differ, first at %s (got %r, expected %r), last at %s (shape %s)" % (
        what, bad.shape[0], a.numel(), f, got[f].item(), want[f].item(), tuple(bad[-1].tolist()), tuple(got.shape)))


class Guarded:
    """A written tensor as a view into a larger buffer: .buf is filled with SENTINEL (or `fill_buf`),
    .view = slicer(buf) is what the op is handed (filled with `fill` when given).  check() asserts
    that no bit outside the view changed since construction."""

    def __init__(self, shape, slicer, dtype=BF16, device="cpu", fill=None, fill_buf=None):
        if fill_buf is not None:
            self.buf = fill_buf.to(device=device, dtype=dtype).reshape(shape).clone()
        else:
            self.buf = torch.full(shape, SENTINEL if dtype.is_floating_point else 0xA5, dtype=dtype, device=device)
        self.view = slicer(self.buf)
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        slicer(inside)[...] = True
        self.outside = ~inside
        if fill is not None:
            self.view.copy_(fill.to(device))
        self.before = self.buf.clone()

    def check(self, what="output"):
        touched = self.outside & (bits(self.buf) != bits(self.before))
        if bool(touched.any()):
            idx = torch.nonzero(touched)
            raise AssertionError("%s: %d elements written outside the view, first %s, last %s (buffer %s)" % (
                what, idx.shape[0], idx[0].tolist(), idx[-1].tolist(), tuple(self.buf.shape)))


def flat_guard(n, dtype=BF16, device="cpu", lead=8, fill=None):
    """n elements at element offset `lead` of a 1-D sentinel buffer with 8 more behind them
    (lead = 8 keeps 16-byte alignment; 1 offsets a bf16 view by 2 bytes, 2 by 4 bytes)."""
    return Guarded((lead + n + 8,), lambda b: b[lead:lead + n], dtype, device, fill)


# ------------------------------------------------------------------ inputs
def ramp_bf16(n, start=1):
    """n bf16 values whose bit patterns step through 1 .. 65520 (period 65521, a prime, so that the
    period lines up with no tile, row or image size): any permutation error shows.  Patterns with an
    all-ones exponent (inf / nan) are remapped."""
    k = (torch.arange(n, dtype=torch.int64) + start) % 65521
    k = torch.where((k & 0x7F80) == 0x7F80, k ^ 0x4000, k)
    return torch.where(k >= 32768, k - 65536, k).to(torch.int16).view(BF16)


def rnd_bf16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF16)


def relu_out_bf16(shape, seed):
    """a relu output: about half exact zeros, and every 7th of those is -0.0 (not > 0 either)"""
    t = torch.relu(rnd_bf16(shape, seed)).reshape(-1)
    z = torch.nonzero(t == 0).reshape(-1)[::7]
    t[z] = -0.0
    assert bool((t == 0).any()) and bool((t > 0).any()) and bool((bits(t) == -32768).any())
    return t.reshape(shape)


# ------------------------------------------------------------------ permutations and copies
def transpose_ref(x, B, R, Cc):
    """y[b][c][r] = x[b][r][c], flat"""
    b = torch.arange(B).view(B, 1, 1)
    c = torch.arange(Cc).view(1, Cc, 1)
    r = torch.arange(R).view(1, 1, R)
    return x.reshape(-1)[((b * R + r) * Cc + c).reshape(-1)]


def weight_flip_ref(w, G, Co, KH, KW, Ci):
    """Wt[g][ci][KH-1-kh][KW-1-kw][co] = W[g][co][kh][kw][ci], flat"""
    g, ci, kh, kw, co = torch.meshgrid(torch.arange(G), torch.arange(Ci), torch.arange(KH), torch.arange(KW),
                                       torch.arange(Co), indexing="ij")  # coordinates of Wt
    src = (((g * Co + co) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Ci + ci
    return w.reshape(-1)[src.reshape(-1)]


def concat_forward_ref(ins):
    """out[p][off_k + c] = in_k[p][c]; ins: [npix][C_k]"""
    out = torch.empty((ins[0].shape[0], sum(t.shape[1] for t in ins)), dtype=ins[0].dtype)
    off = 0
    for t in ins:
        for c in range(t.shape[1]):
            out[:, off + c] = t[:, c]
        off += t.shape[1]
    return out


def concat_backward_ref(out, ins_before, mask=()):
    """in_k[p][c] = out[p][off_k + c], and for k in mask only where the old in_k[p][c] > 0 (else +0)"""
    res, off = [], 0
    for k, t in enumerate(ins_before):
        g = out[:, off:off + t.shape[1]].clone()
        if k in mask:
            g = torch.where(t > 0, g, torch.zeros_like(g))
        res.append(g)
        off += t.shape[1]
    return res


def channel_copy_ref(src, soff, dst, doff, cc, mode):
    """the new dst [npix][Cd] after dst[p][doff + c] (op)= src[p][soff + c], c < cc.  mode 0 copy,
    1 dst = bf16(fl32(dst + src)), 2 src where the old dst > 0 and +0 elsewhere"""
    out = dst.clone()
    for c in range(cc):
        s, d = src[:, soff + c], dst[:, doff + c]
        if mode == 1:
            v = (d.float() + s.float()).to(dst.dtype)
        elif mode == 2:
            v = torch.where(d > 0, s, torch.zeros_like(s))
        else:
            v = s
        out[:, doff + c] = v
    return out


def pad_interior_ref(x, xp, py, px):
    """the new xp after xp[n][py + h][px + w][:] = x[n][h][w][:]"""
    out = xp.clone()
    N, H, W, _ = x.shape
    for h in range(H):
        for w in range(W):
            out[:N, py + h, px + w] = x[:, h, w]
    return out


def pad_rows_ref(src, rows, L, Lp):
    """dst[r][:L] = src[r][:L], dst[r][L:Lp] = 0"""
    out = torch.zeros((rows, Lp), dtype=src.dtype)
    s = src.reshape(-1)
    for c in range(L):
        out[:, c] = s[torch.arange(rows) * L + c]
    return out


def add_rows_ref(src, dst, rows, L, Ls):
    """the new dst [rows][L] after dst[r][c] = fl32(dst[r][c] + src[r * Ls + c])"""
    out = dst.reshape(rows, L).clone()
    s = src.reshape(-1)
    for c in range(L):
        out[:, c] = out[:, c] + s[torch.arange(rows) * Ls + c]
    return out


def nhwc_to_nchw_ref(x, C, W):
    """y[n][c][h][w] = float(x[n][h][w][c]), c < C, w < W, of x [N][H][Wp][Cp]"""
    N, H, _, _ = x.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32)
    for c in range(C):
        for w in range(W):
            out[:, c, :, w] = x[:, :, w, c].float()
    return out


def input_to_nhwc_ref(x, Cp, scale):
    """[N][H][W][Cp] bf16 of the NCHW fp32 x: bf16(fl32(x * fl32(scale))), channels >= C zero"""
    N, C, H, W = x.shape
    out = torch.zeros((N, H, W, Cp), dtype=BF16)
    s = torch.tensor(scale, dtype=torch.float32)
    for c in range(C):
        out[..., c] = (x[:, c] * s).to(BF16)
    return out


# ------------------------------------------------------------------ single-rounding ops
def cast_ref(x):
    return x.to(BF16)


def add_ref(a, b):
    return (a.float() + b.float()).to(BF16)


def sum_ref(srcs, y_before=None, mask_relu=False, group=4):
    """sum_bf16 as ops.sum_into chains it: ((s0 + s1) + s2) + s3 in fp32, rounded to bf16 after each
    group of `group` terms, the rounded value leading the next group (group = None: one rounding
    at the end, the torch path).  mask_relu: kept where y_before > 0, +0 elsewhere (each group of
    the chain applies it; it is idempotent)."""
    acc, cnt = srcs[0].float(), 1
    for t in srcs[1:]:
        if group is not None and cnt == group:
            acc, cnt = acc.to(BF16).float(), 1
        acc, cnt = acc + t.float(), cnt + 1
    out = acc.to(BF16)
    if mask_relu:
        out = torch.where(y_before > 0, out, torch.zeros_like(out))
    return out


def cast_inputs(n):
    """fp32 random values that end with the edges of the conversion: exact ties between two bf16 numbers of
    both parities (round to even: down and up), +-0, +-inf, the largest finite fp32 (rounds to inf),
    the largest that stays finite, and the neighbours of a tie."""
    edge = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F800000,
                         0xFF800000, 0x7F7FFFFF, 0x7F7F7FFF, 0x3F808001, 0x3F807FFF], dtype=torch.int64)
    edge = torch.where(edge >= 2 ** 31, edge - 2 ** 32, edge).to(torch.int32).view(torch.float32)
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 3
    k = min(n, edge.numel())
    x[n - k:] = edge[:k]  # at the end of the tensor
    return x


# ------------------------------------------------------------------ image input stage
def image_case(mode, B, h, w, C, seed, scale=1.0 / 64):
    """pix u8 [B][h][w][C], prm int32 [B][4] = (crop_y, crop_x, mirrored, 0), cm fp32 [B][2] =
    (contrast, illumination), mean (mode 1 [C]; 2 [C][h+3][w+5], uniform in [0, 255]; 3 [C][h][w]).
    Contrasts differ by >= 0.35 between neighbouring images; in mode 2 the crop offsets include 0
    and the largest legal value (3, 5), and mirrored and unmirrored images alternate."""
    assert B >= 2
    g = torch.Generator().manual_seed(seed)
    pix = torch.randint(0, 256, (B, h, w, C), generator=g, dtype=torch.uint8)
    prm = torch.zeros((B, 4), dtype=torch.int32)
    b = torch.arange(B)
    cm = torch.stack([0.6 + 0.35 * (b % 4).float() + 0.05 * torch.rand(B, generator=g),
                      -5.0 + 3.1 * (b % 4).float() + torch.rand(B, generator=g)], 1).float()
    mean = None
    if mode == 1:
        mean = torch.tensor([100.0, 110.5, 120.25, 90.0][:C])
    elif mode == 2:
        mean = torch.rand((C, h + 3, w + 5), generator=g) * 255
        prm[:, 0] = torch.tensor([0, 3, 1, 2, 3, 0])[b % 6]
        prm[:, 1] = torch.tensor([5, 0, 2, 5, 0, 3])[b % 6]
        prm[:, 2] = (b + 1) % 2  # images 0, 2, .. mirrored
    elif mode == 3:
        mean = torch.rand((C, h, w), generator=g) * 255
    return dict(pix=pix, prm=prm, cm=cm, mean=mean, mode=mode, scale=scale)


def image_operands(case, mutate=None):
    """(d, m, ct, il) fp32, each [B][h][w][C]: the operands of every output element, m looked up as
    the kernels document it -- mode 1 mean[c]; 2 mean[c][crop_y + r][crop_x + xs], xs = w-1-x on
    mirrored images; 3 mean[c][r][x].  mutate: a deliberate defect for the power checks --
    "col+1" the mean read one column to the right (clamped to the mean image), "nomirror" the mirror
    ignored, "nocrop" the crop offsets dropped, "ct_next" the next image's contrast."""
    pix, prm, cm, mean, mode = case["pix"], case["prm"], case["cm"], case["mean"], case["mode"]
    B, h, w, C = pix.shape
    d = pix.float()
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, h, w, C)
    r = torch.arange(h).view(1, h, 1, 1).expand(B, h, w, C)
    x = torch.arange(w).view(1, 1, w, 1).expand(B, h, w, C)
    c = torch.arange(C).view(1, 1, 1, C).expand(B, h, w, C)
    ctb = (bi + 1) % B if mutate == "ct_next" else bi
    ct, il = cm[:, 0][ctb], cm[:, 1][bi]
    if mode == 0:
        return d, torch.zeros_like(d), torch.ones_like(d), torch.zeros_like(d)
    if mode == 1:
        m = mean.float()[c]
    elif mode == 2:
        Hm, Wm = mean.shape[1], mean.shape[2]
        mir = prm[:, 2].long()[bi] != 0
        if mutate == "nomirror":
            mir = torch.zeros_like(mir)
        xs = torch.where(mir, w - 1 - x, x)
        cy, cx = prm[:, 0].long()[bi], prm[:, 1].long()[bi]
        if mutate == "nocrop":
            cy, cx = torch.zeros_like(cy), torch.zeros_like(cx)
        col = cx + xs + (1 if mutate == "col+1" else 0)
        m = mean.float().reshape(-1)[(c * Hm + cy + r) * Wm + col.clamp_max(Wm - 1)]
    else:
        col = (x + (1 if mutate == "col+1" else 0)).clamp_max(w - 1)
        m = mean.float().reshape(-1)[(c * h + r) * w + col]
    return d, m, ct, il


def _pad_channels(t, Cp):
    out = torch.zeros(tuple(t.shape[:-1]) + (Cp,), dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def image_exact_ref(case, Cp):
    """mode 0: bf16(fl32(d * fl32(scale))) [B][h][w][Cp], pad channels 0"""
    assert case["mode"] == 0
    s = torch.tensor(case["scale"], dtype=torch.float32)
    return _pad_channels((case["pix"].float() * s).to(BF16), Cp)


def image_bound_ref(case, Cp, mutate=None):
    """modes 1..3: (ref, bound) float64 [B][h][w][Cp] of ((d - m) * ct + il) * scale stored as bf16
    (the bound of the module docstring); pad channels have ref = bound = 0: exactly 0."""
    d, m, ct, il = (t.double() for t in image_operands(case, mutate))
    s = float(torch.tensor(case["scale"], dtype=torch.float32))
    ref = ((d - m) * ct + il) * s
    A = ((d - m).abs() * ct.abs() + il.abs()) * abs(s)
    bound = U_BF16 * (ref.abs() + 4 * EPS_F32 * A) + 4 * EPS_F32 * A
    return _pad_channels(ref, Cp), _pad_channels(bound, Cp)


def image_emulate(case, Cp, fused):
    """the kernels' arithmetic in fp32, [B][h][w][Cp] bf16: unfused (four roundings), or with
    (d - m) * ct + il rounded once (the product of two fp32 numbers is exact in float64)"""
    d, m, ct, il = image_operands(case)
    s = torch.tensor(case["scale"], dtype=torch.float32)
    t = d - m
    v = (t.double() * ct.double() + il.double()).float() if fused else t * ct + il
    return _pad_channels((v * s).to(BF16), Cp)


# ------------------------------------------------------------------ column sums
def colsum_mask(rows, C, kind, seed):
    """uint8 [rows][C] max-pool offsets (0..8) with bit 7 set at ~40 % of the entries ("some"), at all
    of them or at none; None for kind None"""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 9, (rows, C), generator=g, dtype=torch.uint8)
    if kind == "all":
        return m | 128
    if kind == "none":
        return m
    return m | ((torch.rand(rows, C, generator=g) < 0.4).to(torch.uint8) * 128)


def colsum_exact_inputs(rows, C, seed=0):
    """(dy bf16 [rows][C], db0 fp32 [C]): dy[r][c] = +-(((digit + 7 r + 3 c) mod 17) - 8), digit the
    base-17 digit c mod 4 of r, with a random sign pattern mixed in: integers in -8 .. 8, no two rows
    equal (asserted by the CPU tests wherever C >= 8).  db0[c] = (5 c mod 11) + 1: non-zero integers"""
    r = torch.arange(rows, dtype=torch.int64).view(rows, 1)
    c = torch.arange(C, dtype=torch.int64).view(1, C)
    g = torch.Generator().manual_seed(1000 + seed)
    sign = torch.randint(0, 2, (rows, C), generator=g) * 2 - 1
    digit = (r // 17 ** (c % 4)) % 17  # column c carries base-17 digit c mod 4 of the row number
    dy = (((digit + 7 * r + 3 * c) % 17) - 8) * sign
    db0 = ((5 * c.reshape(-1)) % 11 + 1).float()
    return dy.to(BF16), db0


def colsum_exact_ref(dy, db0, mask=None):
    """the integer sum db0[c] + sum_r dy[r][c] (masked terms left out) as fp32, after asserting the
    exactness condition max_c (|db0[c]| + sum_r |dy[r][c]|) < 2^24 on the unmasked magnitudes"""
    d, i = dy.to(torch.int64), db0.to(torch.int64)
    assert torch.equal(d.to(BF16), dy) and torch.equal(i.float(), db0), "exact inputs must be integers"
    assert int((i.abs() + d.abs().sum(0)).max()) < 2 ** 24
    if mask is not None:
        d = torch.where(mask >= 128, torch.zeros_like(d), d)
    return (i + d.sum(0)).float()


def colsum_bounded_ref(dy, db0, mask=None):
    """(ref, bound) float64 [C] for random inputs: (R + 2) 2^-23 (sum |dy| + |db0|) over the terms
    that count; R <= COLSUM_BOUND_MAX_ROWS"""
    assert dy.shape[0] <= COLSUM_BOUND_MAX_ROWS
    d, i = dy.double(), db0.double()
    if mask is not None:
        d = torch.where(mask >= 128, torch.zeros_like(d), d)
    return i + d.sum(0), (dy.shape[0] + 2) * EPS_F32 * (d.abs().sum(0) + i.abs())


def colsum_bounded_inputs(rows, C, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return rnd_bf16((rows, C), 3000 + seed), torch.randn(C, generator=g) + 2.0


# ------------------------------------------------------------------ case lists (shared by the CPU and GPU tests)
BIG8 = (1 << 20) + 3  # 16-byte items: one more trip of a grid-stride loop capped at 4096 blocks of 256

TRANSPOSE_TILED = [(3, 1, 1), (2, 31, 33), (2, 32, 32), (2, 33, 31), (3, 36, 256), (5, 7, 70)]
TRANSPOSE_ITEM = [(64, 2, 4), (64, 36, 256), (64, 256, 36), (70, 12, 20), (64, 94, 256)]  # 94 * 258 * 2 = 48504 B
TRANSPOSE_FALLBACK = [(64, 96, 256), (64, 35, 256), (64, 36, 254)]  # over the LDS limit, odd R, Cc % 4 != 0

FLIP_TAPS = [(1, 1), (3, 3), (5, 5), (1, 7)]
FLIP_CHANNELS = [(8, 8), (64, 64), (72, 160), (20, 12), (65, 8), (8, 65)]
FLIP_CASES = [(G, Co, KH, KW, Ci) for G in (1, 2) for KH, KW in FLIP_TAPS for Co, Ci in FLIP_CHANNELS]
FLIP_MANY = [(1 + i % 2, 8 + 4 * (i % 5), 1 + 2 * (i % 2), 1 + i % 3, 8 * (1 + i % 3) + (i % 7 == 0)) for i in range(70)]

CONCAT_SETS = [[8], [8, 8], [64, 128, 32, 24], [24, 8, 16]]
CONCAT_CASES = [(cs, npix) for cs in CONCAT_SETS for npix in (1, 105)] + [([8, 8], BIG8 // 2 + 1)]

# (Cs, soff, Cd, doff, Cc, npix, src_lead): src_lead = 1 offsets the source's base by 2 bytes
CHANNEL_COPY_VECTOR = [(40, 8, 64, 16, 24, 1, 8), (40, 8, 64, 16, 24, 105, 8), (8, 0, 16, 8, 8, BIG8, 8)]
CHANNEL_COPY_SCALAR = [(40, 8, 64, 16, 20, 1, 8), (40, 8, 64, 16, 20, 105, 8), (40, 4, 64, 16, 24, 105, 8),
                       (40, 8, 64, 16, 24, 105, 1), (40, 8, 64, 16, 20, 52500, 8)]  # 1.05 M elements

PAD_INTERIOR_GEOS = [(2, 5, 7, 1, 1, 7, 9), (3, 4, 6, 2, 0, 8, 9), (1, 1, 1, 3, 3, 7, 7)]  # N H W py px H2 W2
PAD_INTERIOR_C = [4, 64, 3, 6]
PAD_ROWS = [(96 * 11, 33, 40), (5, 8, 8), (3, 1, 8), (7, 21, 24)]

FAN_ND = [1, 2, 3, 4, 5, 7, 9]
FAN_N = [8, 840]
FAN_BIG = 8 * BIG8
ELEMENTWISE_N = [1, 7, 8, 9, 4099, (1 << 21) + 9]

LAYOUT_CCP = [(3, 4), (3, 3), (1, 1), (5, 8), (8, 8)]
LAYOUT_CASES = [(C, Cp, wpad, scale) for C, Cp in LAYOUT_CCP for wpad in (0, 4) for scale in (1.0, 1.0 / 64)]
LAYOUT_NHW = (2, 3, 5)

COPY_ELEMS = [1, 3, 2050]  # bf16: 2, 6 and 4100 bytes


def _multi_cases():
    cases = []
    for C, rows, masked_rows in ((512, [1, 31, 32, 33, 95, 96, 97, 193], [1, 31, 32, 33, 64, 65, 95, 96, 97, 193]),
                                 (8, [1, 255, 256, 257, 2047, 2048, 2049, 6144, 6145], None),
                                 (24, [84, 85, 86, 681], None), (520, [33, 97], []), (4096, [31, 97], [])):
        cases += [(C, r, None) for r in rows]
        cases += [(C, r, "some") for r in (rows if masked_rows is None else masked_rows)]
    return cases + [(512, 97, "all"), (8, 257, "none")]


COLSUM_MULTI = _multi_cases()  # (C, rows, mask kind)
COLSUM_MANY = [COLSUM_MULTI[(i * 7) % len(COLSUM_MULTI)] for i in range(70)]  # 70 segments, masked ones among them
COLSUM_SLICE = [(512, 97), (8, 257), (24, 86)]
COLSUM_NOSPLIT = [(C, r) for C in (520, 4096) for r in (255, 256, 257, 513)]
COLSUM_DET = [(C, r) for C in (8, 24, 512, 520) for r in (1, 511, 512, 513, 1025)]
COLSUM_SCALAR = [(C, r) for C in (3, 20, 1001) for r in (1, 700)]

IMAGE_GENERIC_CCP = [(3, 4), (1, 1), (3, 8), (1, 4)]
IMAGE_GENERIC_HW = [(5, 7), (13, 17), (3, 257), (2, 1)]
# row-padded path (C = Cp = 3): (B, h, w, Wp); groups = B h Wp / 4
IMAGE_ROWPAD = [
    (2, 3, 1, 4),      # 6 groups: a partial wave only
    (2, 2, 3, 4),      # 4 groups
    (2, 32, 4, 4),     # exactly 64: one full wave through LDS
    (5, 13, 4, 4),     # 65: a full wave and a wave of one group
    (2, 4, 5, 8),      # 16 groups
    (3, 5, 7, 8),      # 30 groups
    (3, 5, 13, 16),    # 60 groups, minimal pad
    (3, 5, 13, 20),    # 75 groups: the minimal pad plus 4
    (257, 1, 1, 4),    # 257 = 256 + 1: the second block holds one group
    (2, 3, 227, 228),  # 342 groups: full waves, then a partial one in the second block
]
IMAGE_ROWPAD_TINY = (2, 1, 2, 4)  # npix * 3 = 12 < 16: the generic kernel, which leaves the pad columns alone


# ------------------------------------------------------------------ shared test bodies
# Each runs one case through cxxnet_amd.ops on `dev` -- "cuda": the HIP kernel, "cpu": the CPU
# branch -- into guarded outputs and compares with the references above, so that the CPU and the
# GPU tests assert the same thing of the same inputs.  (cxxnet_amd is imported here only.)
def _sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def check_transpose(case, dev):
    from cxxnet_amd import ops
    B, R, Cc = case
    x = ramp_bf16(B * R * Cc, start=R + 3 * Cc)
    y = flat_guard(B * R * Cc, device=dev)
    ops.transpose(x.to(dev), y.view, B, R, Cc)
    _sync(dev)
    y.check("transpose %s" % (case,))
    assert_bits_equal(y.view, transpose_ref(x, B, R, Cc), "transpose %s" % (case,))


@functools.lru_cache(maxsize=4)
def _channel_copy_inputs(npix, Cs, Cd):
    """(src, dst) shared by the three modes of a case; neither is written to"""
    return rnd_bf16((npix, Cs), 11), relu_out_bf16((npix + 1, Cd), 12)


def check_channel_copy(case, mode, dev):
    from cxxnet_amd import ops
    Cs, soff, Cd, doff, Cc, npix, lead = case
    what = "channel_copy %s mode %d" % (case, mode)
    src, dst0 = _channel_copy_inputs(npix, Cs, Cd)  # (dst0: one guard row behind the pixels)
    if mode == 1:
        dst0 = dst0 - 0.5
    s = flat_guard(npix * Cs, device=dev, lead=lead, fill=src.reshape(-1))
    d = Guarded((npix + 1, Cd), lambda b: b[:npix, doff:doff + Cc], device=dev, fill_buf=dst0)
    ops.channel_copy(s.view.view(npix, Cs), soff, d.buf[:npix], doff, Cc, accumulate=mode == 1, mask_relu=mode == 2)
    _sync(dev)
    d.check(what)  # the channels on both sides of the slice and the row behind
    got = d.buf[:npix].cpu()
    if mode == 2:
        dead = ~(dst0[:npix, doff:doff + Cc] > 0)
        assert bool(dead.any()) and int(torch.count_nonzero(got[:, doff:doff + Cc][dead])) == 0, what + ": masked element not 0"
    assert_bits_equal(got, channel_copy_ref(src, soff, dst0[:npix], doff, Cc, mode), what)


def check_fanout(nd, n, dev):
    from cxxnet_amd import ops
    src = ramp_bf16(n, start=nd)
    outs = [flat_guard(n, device=dev) for _ in range(nd)]
    ops.fanout_copy(src.to(dev), [o.view for o in outs])
    _sync(dev)
    for k, o in enumerate(outs):
        o.check("fanout nd %d n %d dst %d" % (nd, n, k))
        assert_bits_equal(o.view, src, "fanout nd %d n %d dst %d" % (nd, n, k))


def check_sum_into(nd, n, dev, alias=False, mask_relu=False):
    """alias: y is srcs[0]'s own storage.  The kernel chain rounds after each group of 4; the torch
    paths (the CPU branch, and mask_relu with more than 4 sources on the GPU) round once."""
    from cxxnet_amd import ops
    assert not (alias and mask_relu)
    what = "sum_into nd %d n %d alias %d mask %d" % (nd, n, alias, mask_relu)
    srcs = [rnd_bf16((n,), 20 + k) for k in range(nd)]
    y0 = srcs[0] if alias else relu_out_bf16((n,), 19)
    y = flat_guard(n, device=dev, fill=y0)
    devs = [t.to(dev) for t in srcs]
    if alias:
        devs[0] = y.view
    ops.sum_into(y.view, devs, mask_relu=mask_relu)
    _sync(dev)
    y.check(what)
    chained = dev != "cpu" and not (mask_relu and nd > 4)
    got = y.view.cpu()
    if mask_relu:
        dead = ~(y0 > 0)
        assert bool(dead.any()) and int(torch.count_nonzero(got[dead])) == 0, what + ": masked element not 0"
    assert_bits_equal(got, sum_ref(srcs, y0, mask_relu, group=4 if chained else None), what)
    for k, t in enumerate(devs[1:]):
        assert_bits_equal(t, srcs[k + 1], what + ": source %d changed" % (k + 1))


def check_pad_interior(geo, C, dev, lead=0):
    """lead: element offset of both tensors' bases in 1-D buffers (2: 4-byte but not 8-byte aligned)"""
    from cxxnet_amd import ops
    N, H, W, py, px, H2, W2 = geo
    what = "pad_interior %s C %d lead %d" % (geo, C, lead)
    x = rnd_bf16((N, H, W, C), 31)
    n2 = N * H2 * W2 * C
    xs = flat_guard(x.numel(), device=dev, lead=lead, fill=x.reshape(-1))
    xp = Guarded((lead + n2 + H2 * W2 * C,),
                 lambda b: b[lead:lead + n2].view(N, H2, W2, C)[:, py:py + H, px:px + W], device=dev)
    ops.pad_interior(xs.view.view(N, H, W, C), xp.buf[lead:lead + n2].view(N, H2, W2, C), py, px)
    _sync(dev)
    xp.check(what)  # the border and the image behind keep their sentinel
    assert_bits_equal(xp.buf[lead:lead + n2].view(N, H2, W2, C),
                      pad_interior_ref(x, torch.full((N, H2, W2, C), SENTINEL, dtype=BF16), py, px), what)


def check_layout(case, dev):
    """input_to_nhwc then nhwc_to_nchw of what it stored"""
    from cxxnet_amd import ops
    C, Cp, wpad, scale = case
    N, H, W = LAYOUT_NHW
    Wp = W + wpad
    what = "layout C %d Cp %d Wp %d scale %g" % (C, Cp, Wp, scale)
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(41)) * 3
    node = Guarded((N + 1, H, Wp, Cp), lambda b: b[:N, :, :W], device=dev)
    ops.input_to_nhwc(x.to(dev), node.buf[:N], scale)
    _sync(dev)
    if dev == "cpu":  # the CPU branch zeroes the whole node first
        assert int(torch.count_nonzero(node.buf[:N, :, W:])) == 0 and bool((node.buf[N] == SENTINEL).all())
    else:
        node.check(what)  # pad columns and the image behind untouched
    want = input_to_nhwc_ref(x, Cp, scale)
    assert_bits_equal(node.view, want, what)
    assert int(torch.count_nonzero(node.view[..., C:])) == 0
    back = ops.nhwc_to_nchw(node.buf[:N], C, W)
    _sync(dev)
    assert_bits_equal(back, nhwc_to_nchw_ref(want, C, W), what + " back")


def check_nhwc_to_nchw_slice(dev):
    from cxxnet_amd import ops
    N, H, W, Cp, C = 2, 3, 5, 8, 5
    wide = ramp_bf16(N * H * W * 24, start=7).view(N, H, W, 24)
    back = ops.nhwc_to_nchw(wide.to(dev)[..., 8:8 + Cp], C)
    _sync(dev)
    assert_bits_equal(back, nhwc_to_nchw_ref(wide[..., 8:8 + Cp], C, W), "nhwc_to_nchw of a channel slice")


def check_cast_add(n, dev):
    from cxxnet_amd import ops
    x = cast_inputs(n)
    y = flat_guard(n, device=dev)
    ops.cast_to_bf16(x.to(dev), y.view)
    _sync(dev)
    y.check("cast n %d" % n)
    assert_bits_equal(y.view, cast_ref(x), "cast n %d" % n)
    a, b = rnd_bf16((n,), 51), rnd_bf16((n,), 52)
    b[::5] = -a[::5]  # exact cancellation: +0
    z = flat_guard(n, device=dev)
    ops.add(a.to(dev), b.to(dev), z.view)
    _sync(dev)
    z.check("add n %d" % n)
    assert_bits_equal(z.view, add_ref(a, b), "add n %d" % n)


def colsum_case(C, rows, kind, exact, seed=0):
    """(dy, db0, mask, expected): expected is the fp32 integer sum (exact) or (ref, bound)"""
    dy, db0 = (colsum_exact_inputs if exact else colsum_bounded_inputs)(rows, C, seed)
    mask = colsum_mask(rows, C, kind, 4000 + seed)
    return dy, db0, mask, (colsum_exact_ref if exact else colsum_bounded_ref)(dy, db0, mask)


def assert_colsum(db, expected, exact, what):
    """db: a Guarded fp32 [C]; returns the worst d / bound of a bounded case"""
    import bounds
    db.check(what)
    if exact:
        assert_bits_equal(db.view, expected, what)
        return 0.0
    return bounds.assert_within(db.view.cpu(), expected[0], expected[1], what, axes="c")


def check_bias_grad(C, rows, kind, dev, exact=True, multi=False):
    """one bias_grad (or a bias_grad_multi of one item) of a contiguous dy onto a guarded db"""
    from cxxnet_amd import ops
    what = "bias gradient C %d rows %d mask %s %s" % (C, rows, kind, "exact" if exact else "bounded")
    dy, db0, mask, expected = colsum_case(C, rows, kind, exact)
    db = flat_guard(C, torch.float32, dev, fill=db0)
    m = mask.to(dev) if mask is not None else None
    if multi:
        ops.bias_grad_multi([(dy.to(dev), db.view, m)])
    else:
        ops.bias_grad(dy.to(dev), db.view, m)
    _sync(dev)
    return assert_colsum(db, expected, exact, what)


def check_bias_grad_many(cases, dev, exact=True):
    """every (C, rows, kind) of `cases` in one bias_grad_multi call"""
    from cxxnet_amd import ops
    items, dbs = [], []
    for i, (C, rows, kind) in enumerate(cases):
        dy, db0, mask, expected = colsum_case(C, rows, kind, exact, seed=i)
        db = flat_guard(C, torch.float32, dev, fill=db0)
        items.append((dy.to(dev), db.view, mask.to(dev) if mask is not None else None))
        dbs.append((db, expected, "segment %d of %d: C %d rows %d mask %s" % (i, len(cases), C, rows, kind)))
    ops.bias_grad_multi(items)
    _sync(dev)
    return max(assert_colsum(db, expected, exact, what) for db, expected, what in dbs)


def sliced_rows(dy, lo, extra, dev):
    """dy as channels lo .. lo + C of a buffer `extra` channels wider whose other channels hold 1e30"""
    rows, C = dy.shape
    wide = torch.full((rows, C + extra), 1.0e30, dtype=BF16, device=dev)
    wide[:, lo:lo + C] = dy.to(dev)
    return wide[:, lo:lo + C]


def check_bias_grad_slice(C, rows, route, dev, exact=True):
    """bias_grad_multi of a dy that is a channel slice: "slice" at offset 8 of a buffer 16 channels
    wider, "masked-slice" the same with a mask, "odd-stride" at offset 4 of a buffer 4 wider (a row
    stride that is no multiple of 8).  The neighbour channels hold 1e30, which must not enter a sum."""
    from cxxnet_amd import ops
    kind = "some" if route == "masked-slice" else None
    dy, db0, mask, expected = colsum_case(C, rows, kind, exact)
    d = sliced_rows(dy, 8, 16, dev) if route != "odd-stride" else sliced_rows(dy, 4, 4, dev)
    m = mask.to(dev) if mask is not None else None
    if dev != "cpu":
        assert ops.nn.bias_fast_ok(d, m) is (route == "slice")
    db = flat_guard(C, torch.float32, dev, fill=db0)
    ops.bias_grad_multi([(d, db.view, m)])
    _sync(dev)
    return assert_colsum(db, expected, exact, "bias gradient of a channel slice (%s) C %d rows %d" % (route, C, rows))


def check_copy_zero(n, dev):
    from cxxnet_amd import ops
    src = ramp_bf16(n, start=77)
    dst = flat_guard(n, device=dev)
    ops.copy_(dst.view, src.to(dev))
    _sync(dev)
    dst.check("copy_ of %d bytes" % (2 * n))
    assert_bits_equal(dst.view, src, "copy_ of %d bytes" % (2 * n))
    ops.zero_(dst.view)
    _sync(dev)
    dst.check("zero_ of %d bytes" % (2 * n))
    assert int(torch.count_nonzero(bits(dst.view))) == 0, "zero_ of %d bytes" % (2 * n)


def check_image(case, Cp, Wp, dev, pad_cols="zero"):
    """image_to_nhwc of `case` into a guarded [B][h][Wp][Cp] node pre-filled with the sentinel.
    pad_cols: "zero" the pad columns must have been written 0, "untouched" they keep the sentinel.
    Returns the worst d / bound (0 in mode 0, which is compared by equality)."""
    import bounds
    from cxxnet_amd import ops
    from cxxnet_amd.io.data import U8Images
    pix = case["pix"]
    B, h, w, C = pix.shape
    what = "image mode %d %s Cp %d Wp %d" % (case["mode"], tuple(pix.shape), Cp, Wp)
    img = U8Images(pix, case["prm"], case["cm"], case["mean"], case["mode"], case["scale"])
    out = Guarded((B + 1, h, Wp, Cp), lambda b: b[:B], device=dev)
    ops.image_to_nhwc(img, out.view)
    _sync(dev)
    out.check(what)  # the guard image behind the last one
    got = out.view.cpu()
    worst = 0.0
    if case["mode"] == 0:
        assert_bits_equal(got[:, :, :w], image_exact_ref(case, Cp), what)
    else:
        ref, bound = image_bound_ref(case, Cp)
        worst = bounds.assert_within(got[:, :, :w], ref, bound, what, axes="bhwc")
    assert int(torch.count_nonzero(got[:, :, :w, C:])) == 0, what + ": pad channel not 0"
    if Wp > w:
        pad = got[:, :, w:]
        if pad_cols == "zero":
            assert int(torch.count_nonzero(bits(pad))) == 0, what + ": pad column not 0"
        else:
            assert bool((pad == SENTINEL).all()), what + ": pad column written"
    back = ops.nhwc_to_nchw(out.view, C, w)
    _sync(dev)
    assert_bits_equal(back, nhwc_to_nchw_ref(got, C, w), what + " nhwc_to_nchw")
    return worst


def image_cases():
    """(id, mode, B, h, w, C, Cp, Wp, pad_cols): every image case of the CPU and GPU tests; pad_cols
    is what the GPU kernel serving the case does with the pad columns (check_image)."""
    out = []
    for mode in range(4):
        for C, Cp in IMAGE_GENERIC_CCP:
            for h, w in IMAGE_GENERIC_HW:
                out.append(("generic-m%d-c%dp%d-%dx%d" % (mode, C, Cp, h, w), mode, 3, h, w, C, Cp, w, "untouched"))
    for mode in (0, 1):
        out.append(("quads-m%d-4x9x7" % mode, mode, 4, 9, 7, 3, 4, 7, "untouched"))    # 252 pixels, 63 per image
        out.append(("quads-m%d-253px" % mode, mode, 11, 23, 1, 3, 4, 1, "untouched"))  # one more: the generic kernel
        for B, h, w, Wp in IMAGE_ROWPAD:
            out.append(("rowpad-m%d-%dx%dx%d-wp%d" % (mode, B, h, w, Wp), mode, B, h, w, 3, 3, Wp, "zero"))
        B, h, w, Wp = IMAGE_ROWPAD_TINY
        out.append(("rowpad-m%d-tiny" % mode, mode, B, h, w, 3, 3, Wp, "untouched"))
    return out


def image_case_of(entry):
    _, mode, B, h, w, C = entry[:6]
    return image_case(mode, B, h, w, C, seed=17 * mode + 3 * h + w + C, scale=0.02 if (h + w) % 2 else 1.0 / 64)
