"""GPU affine warp stage: the host draws and decodes, the GPU warps.

Reference: src/io/image_augmenter-inl.hpp:74-121 (ImageAugmenter::Process: random shear /
rotation / scale / aspect matrix, cv::warpAffine with INTER_CUBIC and a constant border, then
the crop).  The reference does this on host threads; with ``affine_gpu = 1`` the split is:

  host (runtime/jpeg_decode.h DrawWarp / PlanWarp / DecodeRegion, the native thread pool, GIL
  released): the record's augmentation draws, the forward matrix of io/augment.py _affine
      inverted and folded together with the crop offset and the mirror into one map from an
      output pixel to a source position, and a libjpeg-turbo decode of only the source rows
      and columns that map can touch, into one packed pinned RGB buffer;
  GPU (csrc/kernels/warp_kernels.hip, inside the training step's input stage): the bicubic
      warp of every output pixel straight into the uint8 batch that the image kernel turns
      into the network input (mean, contrast, illumination and scale stay there).

The warp's definition is ``warp_reference`` below, in integer arithmetic: OpenCV's published
fixed-point scheme (coordinates in 1/32 pixel, cubic weights with A = -0.75 scaled to 2^15,
constant border).  The HIP kernel is bit-equal to it (tests/test_warp_stage_gpu.py), and the
CPU consumer path calls it directly, so ``dev = cpu`` and ``dev = gpu`` see the same pixels.
Records libjpeg does not decode to RGB (PNG, CMYK, 12-bit) are decoded in full by Pillow and
appended to the same packed buffer as full-image regions: one warp for every record.
"""
from functools import lru_cache

import numpy as np
import torch

from .data import DevicePrefetch, U8Images

# per-image table: int64 words per row (runtime/jpeg_decode.h WarpTableField)
TABLE = 16
VALID, OFFSET, X0, Y0, RW, RH, IMG_W, IMG_H, M0, FILL = 0, 1, 2, 3, 4, 5, 6, 7, 8, 14
DRAWS = 8  # float64 per row: shear, angle, scale, ratio, crop y, crop x, mirror, 0
MAX_SIDE = 16384  # the kernel's coordinates are 32-bit: image sides up to this
_COORD_LIMIT = float(2 ** 19)  # |source coordinate| the 32-bit fixed-point sums hold


@lru_cache(maxsize=None)
def cubic_table() -> np.ndarray:
    """int32 (32, 32, 16), read-only: for each phase (fy, fx) in 1/32 pixel the 4 x 4 tap weights
    (row-major, tap row j, tap column i), scaled to 2^15 and summing to exactly 32768."""
    f = np.float32
    t = np.arange(32, dtype=np.float32) / f(32)
    A = f(-0.75)

    def inner(u):
        return ((A + f(2)) * u - (A + f(3))) * u * u + f(1)
    c0 = ((A * (t + f(1)) - f(5) * A) * (t + f(1)) + f(8) * A) * (t + f(1)) - f(4) * A
    c1 = inner(t)
    c2 = inner(f(1) - t)
    c3 = f(1) - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], 1).astype(np.float32)  # (32, 4)
    prod = c[:, None, :, None] * c[None, :, None, :]  # (fy, fx, j, i), float32
    tab = np.clip(np.rint(prod * f(32768)), -32768, 32767).astype(np.int32).reshape(32, 32, 16)
    central = (5, 6, 9, 10)  # j, i in {1, 2}, row-major
    for fy in range(32):
        for fx in range(32):
            w = tab[fy, fx]
            diff = int(w.sum()) - 32768
            if diff == 0:
                continue
            cen = [int(w[k]) for k in central]
            k = central[cen.index(max(cen))] if diff < 0 else central[cen.index(min(cen))]
            w[k] -= diff
    tab.setflags(write=False)
    return tab


def warp_one(src: np.ndarray, t: np.ndarray, h: int, w: int, C: int) -> np.ndarray:
    """One table row: (h, w, C) uint8 from the packed buffer."""
    x0, y0, rw, rh, W, H, fill = (int(t[k]) for k in (X0, Y0, RW, RH, IMG_W, IMG_H, FILL))
    m = t[M0:M0 + 6].view(np.float64)
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    ad = np.rint(m[0] * xs * 1024).astype(np.int64)
    bd = np.rint(m[3] * xs * 1024).astype(np.int64)
    X0v = np.rint((m[1] * ys + m[2]) * 1024).astype(np.int64) + 16
    Y0v = np.rint((m[4] * ys + m[5]) * 1024).astype(np.int64) + 16
    X = (X0v[:, None] + ad[None, :]) >> 5
    Y = (Y0v[:, None] + bd[None, :]) >> 5
    ix, iy = (X >> 5) - 1, (Y >> 5) - 1
    wt = cubic_table()[Y & 31, X & 31].astype(np.int64)  # (h, w, 16)
    empty = rw <= 0 or rh <= 0
    reg = None if empty else src[int(t[OFFSET]):int(t[OFFSET]) + rw * rh * 3].reshape(rh, rw, 3).astype(np.int64)
    acc = np.zeros((h, w, 3), np.int64)
    for j in range(4):
        for i in range(4):
            sx, sy = ix + i, iy + j
            inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            if empty:
                tap = np.full((h, w, 3), fill, np.int64)
            else:
                # a tap inside the image is inside the region by construction (clamped like the kernel)
                tap = reg[np.clip(sy - y0, 0, rh - 1), np.clip(sx - x0, 0, rw - 1)]
                tap = np.where(inside[..., None], tap, fill)
            acc += tap * wt[..., j * 4 + i, None]
    return np.clip((acc + 16384) >> 15, 0, 255).astype(np.uint8)[..., :C]


def warp_reference(src, table, r0: int, r1: int, h: int, w: int, C: int) -> np.ndarray:
    """The normative warp in numpy: rows r0..r1 of the batch, (r1 - r0, h, w, C) uint8, from the
    packed uint8 source buffer and the per-image table (zeros for rows with valid = 0)."""
    src = np.asarray(src, dtype=np.uint8).reshape(-1)
    table = np.asarray(table, dtype=np.int64).reshape(-1, TABLE)
    out = np.zeros((r1 - r0, h, w, C), np.uint8)
    for b in range(r0, r1):
        if table[b, VALID]:
            out[b - r0] = warp_one(src, table[b], h, w, C)
    return out


def check_table(table: np.ndarray, nsrc: int, h: int, w: int):
    """Host-side bounds of everything the kernel indexes or holds in 32-bit integers."""
    t = table[table[:, VALID] != 0]
    if not len(t):
        return
    if (t[:, [X0, Y0, RW, RH, OFFSET]] < 0).any() or int(t[:, [RW, RH, IMG_W, IMG_H]].max()) > MAX_SIDE:
        raise ValueError("image_warp: region or image larger than 16384 px a side, or negative")
    if int((t[:, OFFSET] + t[:, RW] * t[:, RH] * 3).max()) > nsrc:
        raise ValueError("image_warp: region outside the packed buffer")
    if (t[:, FILL] < 0).any() or (t[:, FILL] > 255).any():
        raise ValueError("image_warp: fill is a byte")
    m = np.abs(np.ascontiguousarray(t[:, M0:M0 + 6]).view(np.float64))
    reach = np.maximum(m[:, 0] * (w - 1) + m[:, 1] * (h - 1) + m[:, 2], m[:, 3] * (w - 1) + m[:, 4] * (h - 1) + m[:, 5])
    if not np.isfinite(reach).all() or float(reach.max()) >= _COORD_LIMIT:
        raise ValueError("image_warp: map reaches source coordinates beyond 2^19")


class WarpImages:
    """A batch still as packed source regions plus warp maps (rows r0..r1 of the staged batch).
    Duck-types the parts of U8Images the trainer touches (shape, row slices, clone, to_float);
    ``to_u8(device)`` runs the warp (the HIP kernel, or the numpy reference on the CPU)."""

    def __init__(self, src, table, prm, cm, hwc, mean=None, mode=0, scale=1.0, r0=0, r1=None, pf=None):
        self.src, self.table, self.prm_all, self.cm_all, self.hwc = src, table, prm, cm, tuple(hwc)
        self.mean, self.mode, self.scale = mean, mode, float(scale)
        self.r0, self.r1 = r0, table.shape[0] if r1 is None else r1
        self.pf = pf  # DevicePrefetch of (src, table, prm)

    def prefetch(self, dev: torch.device):
        """Issue the batch's host-to-device copies now, on a side stream (the iterator's thread)."""
        self.pf = DevicePrefetch([self.src, self.table, self.prm_all], dev)

    @property
    def shape(self):
        h, w, C = self.hwc
        return (self.r1 - self.r0, C, h, w)

    @property
    def prm(self):
        return self.prm_all[self.r0:self.r1]

    @property
    def cm(self):
        return self.cm_all[self.r0:self.r1]

    def _view(self, r0, r1):
        return WarpImages(self.src, self.table, self.prm_all, self.cm_all, self.hwc, self.mean, self.mode,
                          self.scale, r0, r1, self.pf)

    def __getitem__(self, sl):
        if not isinstance(sl, slice) or sl.step not in (None, 1):
            raise TypeError("WarpImages supports contiguous row slices only")
        lo, hi, _ = sl.indices(self.r1 - self.r0)
        return self._view(self.r0 + lo, self.r0 + max(hi, lo))

    def clone(self):  # the staged buffers are never written after the batch is made
        return self._view(self.r0, self.r1)

    def to_u8(self, device=None) -> U8Images:
        dev = torch.device(device) if device is not None else torch.device("cpu")
        h, w, C = self.hwc
        prm, cm = self.prm, self.cm
        if dev.type == "cuda":
            from .. import ops
            staged = self.pf.take(dev) if self.pf is not None else None
            pix = ops.image_warp(self.src, self.table, self.r0, self.r1, h, w, C, dev,
                                 staged[:2] if staged is not None else None)
            if staged is not None:  # the image kernel's prm on the device too
                prm = staged[2][self.r0:self.r1]
                cm = cm.to(dev, non_blocking=True)
        else:
            pix = torch.from_numpy(warp_reference(self.src.numpy(), self.table.numpy(), self.r0, self.r1, h, w, C))
        return U8Images(pix, prm, cm, self.mean, self.mode, self.scale)

    def to_float(self) -> torch.Tensor:
        return self.to_u8().to_float()


def warp_cfg(aug, mean_mode: int):
    """The native pool's warp settings from an AugmentParam (runtime/bindings.cpp ParseWarpConfig)."""
    C, h, w = aug.shape
    return (h, w, C, aug.rand_crop, aug.rand_mirror, aug.mirror, aug.max_random_contrast,
            aug.max_random_illumination, mean_mode, aug.max_rotate_angle, aug.max_shear_ratio, aug.max_aspect_ratio,
            aug.min_random_scale, aug.max_random_scale, aug.min_img_size, aug.max_img_size, aug.rotate,
            list(aug.rotate_list), aug.fill_value)


def _empty(shape, dtype, pinned):
    return torch.empty(shape, dtype=dtype, pin_memory=pinned)


def stage_batch(pool, items, cfg, B: int, pinned: bool, decode_full, force_full=frozenset()):
    """Run the host half over `items` [(row, payload, seed)]: plan every record, lay the regions
    out in one packed buffer, decode them.  ``decode_full(payload)`` returns the (H, W, 3) uint8
    RGB decode of a record the native decoder does not take (Pillow).  Returns (src, table, prm,
    cm, draws, fallback rows)."""
    table = _empty((B, TABLE), torch.int64, pinned)
    table.numpy().fill(0)  # numpy fills: torch's parallel fill wakes its OpenMP pool
    prm = _empty((B, 4), torch.int32, pinned)
    prm.numpy().fill(0)
    cm = _empty((B, 2), torch.float32, pinned)
    cm.numpy()[:, 0], cm.numpy()[:, 1] = 1.0, 0.0
    draws = np.zeros((B, DRAWS), np.float64)
    tab = table.numpy()
    native_items = [it for it in items if it[0] not in force_full]
    failed, small = pool.plan_warp(native_items, cfg, tab, draws, prm.numpy(), cm.numpy()) if native_items else ([], [])
    fb_rows = sorted(set(failed) | {it[0] for it in items if it[0] in force_full})
    full = {}
    for row, payload, seed in items:
        if row not in fb_rows:
            continue
        img = np.ascontiguousarray(decode_full(payload)[..., :3])
        H, W = img.shape[:2]
        got = type(pool).draw_warp(seed, W, H, cfg)
        if got is None:
            small = list(small) + [row]
            continue
        d, m, _, mirror, contrast, illum = got
        t = tab[row]
        t[:] = 0
        t[VALID], t[RW], t[RH], t[IMG_W], t[IMG_H], t[FILL] = 1, W, H, W, H, cfg[18]
        t[M0:M0 + 6] = np.asarray(m, np.float64).view(np.int64)
        draws[row] = d
        prm[row] = torch.tensor([0, 0, int(mirror), 0], dtype=torch.int32)
        cm[row] = torch.tensor([contrast, illum])
        full[row] = img
    if small:
        raise ValueError("augmented image is smaller than input_shape")
    sizes = tab[:, RW] * tab[:, RH] * 3 * (tab[:, VALID] != 0)
    tab[:, OFFSET] = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    src = _empty((max(total, 1),), torch.uint8, pinned)
    buf = src.numpy()
    for row, img in full.items():
        o = int(tab[row, OFFSET])
        buf[o:o + img.size] = img.reshape(-1)
    again = pool.decode_regions(native_items, tab, buf) if native_items else []
    if again:  # corrupt past the header: decode those records with Pillow instead
        return stage_batch(pool, items, cfg, B, pinned, decode_full, frozenset(force_full) | set(again))
    return src, table, prm, cm, draws, fb_rows

