"""GPU affine warp stage, host half + numpy reference (io/warp_stage.py): the weight table's
invariants, warps whose result is known exactly, and the native staging (draws, map, source
region decode: runtime/jpeg_decode.h DrawWarp / PlanWarp / DecodeRegion)."""
import io
import math

import numpy as np
import pytest
import torch

from cxxnet_amd import native
from cxxnet_amd.io import warp_stage as ws
from cxxnet_amd.io.augment import AugmentParam

from test_jpeg_stage_cpu import _jpeg, _photo

IDENT = (1, 0, 0, 0, 1, 0)


def make_table(rows, B=None):
    """A table from [(row, valid, offset, x0, y0, rw, rh, W, H, m0..m5, fill)]."""
    tab = np.zeros((B if B is not None else len(rows), ws.TABLE), np.int64)
    for row, valid, off, x0, y0, rw, rh, W, H, m, fill in rows:
        tab[row, :8] = (valid, off, x0, y0, rw, rh, W, H)
        tab[row, ws.M0:ws.M0 + 6] = np.asarray(m, np.float64).view(np.int64)
        tab[row, ws.FILL] = fill
    return tab


def _full(img, m, fill=0, row=0, off=0):
    """Table row warping the whole of `img` (H, W, 3) staged at byte offset `off`."""
    H, W = img.shape[:2]
    return (row, 1, off, 0, 0, W, H, W, H, m, fill)


def _warp(img, m, h, w, C=3, fill=0):
    return ws.warp_reference(img.reshape(-1), make_table([_full(img, m, fill)]), 0, 1, h, w, C)[0]


def bowl_aug(shape=(3, 40, 40)):
    """The augmentation keys of examples/kaggle_bowl/bowl.conf."""
    p = AugmentParam()
    for k, v in [("input_shape", ",".join(map(str, shape))), ("rand_mirror", "1"), ("rand_crop", "1"),
                 ("max_rotate_angle", "180"), ("max_aspect_ratio", "0.5"), ("max_shear_ratio", "0.3"),
                 ("min_crop_size", "32"), ("max_crop_size", "48")]:
        p.set_param(k, v)
    return p


def matrix_from_draws(d, W, H, p, h, w):
    """m0..m5 from the raw draws with io/augment.py _affine's formulas (plus crop and mirror)."""
    s, angle, scale, ratio, cy, cx, mirror = d[:7]
    a, b = math.cos(angle / 180.0 * math.pi), math.sin(angle / 180.0 * math.pi)
    hs = 2 * scale / (1 + ratio)
    wsc = ratio * hs
    new_w = int(max(p.min_img_size, min(p.max_img_size, scale * W)))
    new_h = int(max(p.min_img_size, min(p.max_img_size, scale * H)))
    M = np.array([[hs * a - s * b * wsc, hs * b + s * a * wsc, 0], [-b * wsc, a * wsc, 0], [0, 0, 1]], np.float64)
    M[0, 2] = (new_w - (M[0, 0] * W + M[0, 1] * H)) / 2
    M[1, 2] = (new_h - (M[1, 0] * W + M[1, 1] * H)) / 2
    out2warped = np.array([[-1.0 if mirror else 1.0, 0, (w - 1 + cx) if mirror else cx], [0, 1, cy], [0, 0, 1]])
    return (np.linalg.inv(M) @ out2warped)[:2].reshape(-1), (new_w, new_h)


# ------------------------------------------------------------------------------ the table
def test_table_invariants():
    t = ws.cubic_table()
    assert t.shape == (32, 32, 16) and t.dtype == np.int32
    assert (t.sum(-1) == 32768).all()
    assert t.min() == -3638 and t.max() == 32768
    assert np.argwhere(t == 32768).tolist() == [[0, 0, 5]]  # fx = fy = 0, the central tap
    assert np.abs(t.astype(np.int64)).sum(-1).max() <= 61952
    assert (t[0, 0] == np.eye(16, dtype=np.int32)[5] * 32768).all()  # phase 0 copies the pixel


# ------------------------------------------------------------------------------ exact warps
@pytest.mark.parametrize("C", [3, 1])
def test_exact_shift_mirror_rotate(C):
    img = _photo(np.random.default_rng(0), 37, 45)
    h, w = 20, 23
    assert np.array_equal(_warp(img, (1, 0, 5, 0, 1, 7), h, w, C), img[7:7 + h, 5:5 + w, :C])
    assert np.array_equal(_warp(img, (-1, 0, w - 1 + 5, 0, 1, 7), h, w, C), img[7:7 + h, 5:5 + w, :C][:, ::-1])
    # sx = y, sy = x: the transposed source
    assert np.array_equal(_warp(img, (0, 1, 0, 1, 0, 0), 30, 25, C), img[:25, :30, :C].transpose(1, 0, 2))
    # a shifted window past the border reads the fill value there and the image elsewhere
    out = _warp(img, (1, 0, -3, 0, 1, -2), h, w, C, fill=9)
    assert (out[:2] == 9).all() and (out[:, :3] == 9).all() and np.array_equal(out[2:, 3:], img[:h - 2, :w - 3, :C])


def test_constant_outside_and_step():
    const = np.full((31, 29, 3), 77, np.uint8)
    m = (0.83, -0.41, 3.7, 0.36, 1.13, -6.2)
    assert (_warp(const, m, 40, 40, fill=77) == 77).all()
    img = _photo(np.random.default_rng(1), 31, 29)
    assert (_warp(img, (1, 0, 500.25, 0, 1, 0.5), 16, 16, fill=200) == 200).all()  # wholly outside
    assert (_warp(img, (0.7, 0.2, -900, -0.2, 0.7, -70), 16, 16, fill=3) == 3).all()
    # a region with no rows is legal: all fill
    tab = make_table([(0, 1, 0, 0, 0, 0, 0, 29, 31, IDENT, 5)])
    assert (ws.warp_reference(np.zeros(1, np.uint8), tab, 0, 1, 8, 8, 3) == 5).all()
    # a step edge magnified 2x: the cubic's over- and undershoot is clamped, not wrapped
    step = np.zeros((16, 16, 3), np.uint8)
    step[:, 8:] = 255
    out = _warp(step, (0.5, 0, 0, 0, 0.5, 2), 20, 28).astype(int)  # every tap inside the image or left of it
    assert (out[:, :12] == 0).all() and (out[:, 20:] == 255).all() and (np.diff(out, axis=1) >= 0).all()
    assert 0 < out[0, 15, 0] < 255


def test_padding_rows_slices_and_images_type():
    img = _photo(np.random.default_rng(2), 20, 22)
    tab = make_table([_full(img, (1, 0, 1, 0, 1, 2), row=0), _full(img, (0.5, 0, 0, 0, 0.5, 0), row=2)], 4)
    out = ws.warp_reference(img.reshape(-1), tab, 0, 4, 10, 12, 3)
    assert not out[[1, 3]].any() and np.array_equal(out[0], img[2:12, 1:13])
    assert np.array_equal(ws.warp_reference(img.reshape(-1), tab, 1, 3, 10, 12, 3), out[1:3])
    prm = torch.zeros((4, 4), dtype=torch.int32)
    cm = torch.tensor([[1.0, 0.0]] * 4)
    wi = ws.WarpImages(torch.from_numpy(img.reshape(-1).copy()), torch.from_numpy(tab), prm, cm, (10, 12, 3))
    assert tuple(wi.shape) == (4, 3, 10, 12) and tuple(wi[1:3].shape) == (2, 3, 10, 12)
    assert np.array_equal(wi.to_u8().pix.numpy(), out)
    assert np.array_equal(wi[1:3].clone().to_u8().pix.numpy(), out[1:3])
    assert torch.equal(wi.to_float(), torch.from_numpy(out).permute(0, 3, 1, 2).float())
    with pytest.raises(TypeError):
        wi[::2]
    with pytest.raises(ValueError):
        ws.check_table(make_table([(0, 1, 4, 0, 0, 22, 20, 22, 20, IDENT, 0)]), img.size, 10, 12)
    with pytest.raises(ValueError):
        ws.check_table(make_table([_full(img, (1, 0, 2.0 ** 20, 0, 1, 0))]), img.size, 10, 12)


def test_trainer_takes_warp_images():
    """NeuralNet.set_input with a WarpImages batch (row-sliced, as the trainer slices it) fills the
    input node like the float batch of the same pixels."""
    from cxxnet_amd.nnet import NetTrainer
    conf = "netconfig=start\nlayer[+1] = flatten\nlayer[+1] = fullc:f1\n  nhidden = 3\nlayer[+0] = softmax\n" \
           "netconfig=end\ninput_shape = 3,10,12\n"
    tr = NetTrainer()
    for k, v in list(native.rt().parse_config(conf)) + [("batch_size", "3"), ("dev", "cpu"), ("eval_train", "0"),
                                                        ("silent", "1")]:
        tr.set_param(k, v)
    tr.init_model()
    img = _photo(np.random.default_rng(3), 20, 22)
    tab = make_table([_full(img, (0.9, 0.2, 1, -0.2, 0.9, 4), row=r) for r in range(4)])
    mean = torch.tensor([104.0, 117.0, 123.0])
    wi = ws.WarpImages(torch.from_numpy(img.reshape(-1).copy()), torch.from_numpy(tab),
                       torch.zeros((4, 4), dtype=torch.int32), torch.tensor([[1.1, 2.0]] * 4), (10, 12, 3), mean, 1, 0.5)
    nodes = []
    for data in (wi[1:4], wi[1:4].to_float()):
        tr.net.set_input(data)
        nodes.append(tr.net.nodes[0].data[:3].float().clone())
    assert torch.equal(nodes[0], nodes[1]) and nodes[0].std() > 1


# ------------------------------------------------------------------------------ native staging
@pytest.fixture(scope="module")
def pool_cls():
    rt = native.rt()
    if not rt.JpegDecodePool.available():
        pytest.skip("no libjpeg")
    return rt.JpegDecodePool


@pytest.fixture(scope="module")
def small_records():
    """Bowl-sized records (about 50-90 px): 4:2:0, 4:4:4, 4:2:2, grayscale, progressive."""
    rng = np.random.default_rng(11)
    kws = [dict(quality=90, subsampling=2), dict(quality=90, subsampling=0), dict(quality=80, subsampling=1),
           dict(quality=85), dict(quality=90, subsampling=2, progressive=True)]
    recs = []
    for i in range(16):
        h, w = (int(v) for v in rng.integers(50, 91, 2))
        kw = kws[i % len(kws)]
        recs.append(_jpeg(_photo(rng, h, w, gray="subsampling" not in kw), **kw))
    return recs


def _stage(pool, recs, cfg, B, seeds):
    items = [(r, recs[r % len(recs)], seeds[r]) for r in range(B)]
    return ws.stage_batch(pool, items, cfg, B, False, None)


def test_native_draws_and_matrix(pool_cls, small_records):
    p = bowl_aug()
    cfg = ws.warp_cfg(p, 1)
    B = 64
    seeds = [977 * r + 5 for r in range(B)]
    runs = [_stage(pool_cls(nt), small_records, cfg, B, seeds) for nt in (1, 4, 1)]
    for other in runs[1:]:  # deterministic per seed, whatever the thread count
        for a, b in zip(runs[0][:5], other[:5]):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    src, table, prm, cm, draws, fb = runs[0]
    tab = table.numpy()
    assert fb == [] and (tab[:, ws.VALID] == 1).all()
    assert set(prm[:, 2].tolist()) == {0, 1} and (prm[:, [0, 1, 3]] == 0).all()
    assert (np.abs(draws[:, 0]) <= 0.3).all() and draws[:, 1].min() < -90 and draws[:, 1].max() > 90
    assert (draws[:, 1] == np.rint(draws[:, 1])).all() and (np.abs(draws[:, 3] - 1) <= 0.5).all()
    assert (draws[:, 2] == 1).all() and np.array_equal(draws[:, 6], prm[:, 2].numpy())
    for r in range(B):
        W, H = int(tab[r, ws.IMG_W]), int(tab[r, ws.IMG_H])
        want, (nw, nh) = matrix_from_draws(draws[r], W, H, p, 40, 40)
        got = tab[r, ws.M0:ws.M0 + 6].view(np.float64)
        # 1e-9 relative, per entry; an entry that cancels towards zero (cos 90 deg) carries an absolute
        # error of a few ulp of the matrix's largest entry, so that is its scale (measured: 1.3e-14
        # per entry, 5.5e-16 of the largest entry)
        assert np.allclose(got, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), (r, got, want)
        assert 0 <= draws[r, 4] <= nh - 40 and 0 <= draws[r, 5] <= nw - 40
        one = pool_cls.draw_warp(seeds[r], W, H, cfg)  # the Pillow-decode rows' entry point: same draws
        assert list(one[0]) == draws[r].tolist() and list(one[1]) == got.tolist()
        assert one[2] == tuple(tab[r, [ws.X0, ws.Y0, ws.RW, ws.RH]].tolist()) and one[3] == bool(prm[r, 2])
    # a record smaller than the crop after the warp raises the Pillow path's error
    tiny = _jpeg(_photo(np.random.default_rng(0), 30, 30), quality=90)
    with pytest.raises(ValueError, match="smaller than input_shape"):
        ws.stage_batch(pool_cls(1), [(0, tiny, 1)], cfg, 1, False, None)
    assert pool_cls.draw_warp(1, 30, 30, cfg) is None


def test_region_equals_full_decode(pool_cls, small_records, records_large):
    """Warping the staged region equals warping the fully decoded image, bit for bit."""
    pool = pool_cls(3)
    for recs, shape, B in [(small_records, (3, 40, 40), 64), (records_large, (3, 97, 113), 16)]:
        p = bowl_aug(shape)
        cfg = ws.warp_cfg(p, 1)
        C, h, w = shape
        seeds = [31 * r + 2 for r in range(B)]
        src, table, prm, cm, draws, fb = _stage(pool, recs, cfg, B, seeds)
        tab = table.numpy()
        out = ws.warp_reference(src.numpy(), tab, 0, B, h, w, C)
        full = tab.copy()
        full[:, ws.X0] = full[:, ws.Y0] = 0
        full[:, ws.RW], full[:, ws.RH] = full[:, ws.IMG_W], full[:, ws.IMG_H]
        sizes = full[:, ws.RW] * full[:, ws.RH] * 3
        full[:, ws.OFFSET] = np.cumsum(sizes) - sizes
        buf = np.zeros(int(sizes.sum()), np.uint8)
        items = [(r, recs[r % len(recs)], seeds[r]) for r in range(B)]
        assert pool.decode_regions(items, full, buf) == []
        ref = ws.warp_reference(buf, full, 0, B, h, w, C)
        assert np.array_equal(out, ref)
        # the regions are real crops: smaller than the images for a good share of the batch
        assert int((tab[:, ws.RW] * tab[:, ws.RH]).sum()) < int((full[:, ws.RW] * full[:, ws.RH]).sum())
        inside = (tab[:, ws.X0] + tab[:, ws.RW] <= tab[:, ws.IMG_W]) & (tab[:, ws.Y0] + tab[:, ws.RH] <= tab[:, ws.IMG_H])
        assert inside.all() and out.std() > 10


@pytest.fixture(scope="module")
def records_large():
    rng = np.random.default_rng(5)
    return [_jpeg(_photo(rng, 256, 300), quality=90, subsampling=2),
            _jpeg(_photo(rng, 301, 256), quality=90, subsampling=0),
            _jpeg(_photo(rng, 280, 333), quality=80, subsampling=1, progressive=True)]


def test_stage_redecodes_rows_the_native_decoder_drops(pool_cls, small_records):
    """A record whose region decode fails after its header was planned (corrupt data) is staged
    again through the full decode, with the same draws."""
    class Flaky:
        draw_warp = staticmethod(pool_cls.draw_warp)

        def __init__(self):
            self.pool, self.calls = pool_cls(2), 0

        def plan_warp(self, *a):
            return self.pool.plan_warp(*a)

        def decode_regions(self, items, tab, buf):
            self.calls += 1
            return [2] if any(it[0] == 2 for it in items) else self.pool.decode_regions(items, tab, buf)
    cfg = ws.warp_cfg(bowl_aug(), 1)
    items = [(r, small_records[r], 40 + r) for r in range(4)]
    full = []

    def decode_full(payload):
        from cxxnet_amd.io.augment import _decode
        full.append(payload)
        return _decode(payload)
    flaky = Flaky()
    src, table, prm, cm, draws, fb = ws.stage_batch(flaky, items, cfg, 4, False, decode_full)
    ref = ws.stage_batch(pool_cls(1), items, cfg, 4, False, None)
    assert fb == [2] and flaky.calls == 2 and full == [small_records[2]]
    assert np.array_equal(draws, ref[4]) and torch.equal(prm, ref[2]) and torch.equal(cm, ref[3])
    tab = table.numpy()
    assert tab[2, ws.RW] == tab[2, ws.IMG_W] and tab[2, ws.RH] == tab[2, ws.IMG_H]
    # Pillow's decode is bit-identical to the native one (test_image_io.py), so the batch is too
    assert np.array_equal(ws.warp_reference(src.numpy(), tab, 0, 4, 40, 40, 3),
                          ws.warp_reference(ref[0].numpy(), ref[1].numpy(), 0, 4, 40, 40, 3))


def test_decode_regions_checks_bounds(pool_cls, small_records):
    cfg = ws.warp_cfg(bowl_aug(), 1)
    src, table, *_ = _stage(pool_cls(1), small_records, cfg, 2, [1, 2])
    bad = table.numpy().copy()
    bad[1, ws.OFFSET] = src.shape[0]
    bad[1, ws.RW], bad[1, ws.RH] = 8, 8
    with pytest.raises(RuntimeError, match="outside the packed buffer"):
        pool_cls(1).decode_regions([(1, small_records[1], 2)], bad, src.numpy())


def test_iterator_affine_gpu(tmp_path, pool_cls, small_records):
    """iter = img with affine_gpu = 1: WarpImages batches, a PNG and a CMYK record through the
    Pillow decode into the same packed buffer, deterministic per seed; affine_gpu = 0 untouched."""
    from PIL import Image
    from cxxnet_amd.io.data import U8Images
    from cxxnet_amd.io.iterators import create_iterator
    rng = np.random.default_rng(4)
    png, cmyk = io.BytesIO(), io.BytesIO()
    Image.fromarray(_photo(rng, 70, 64)).save(png, format="PNG")
    Image.fromarray(_photo(rng, 66, 80)).convert("CMYK").save(cmyk, format="JPEG")
    recs = list(small_records[:6]) + [png.getvalue(), cmyk.getvalue()]
    lst = []
    for i, r in enumerate(recs):
        (tmp_path / f"{i}.img").write_bytes(r)
        lst.append(f"{i}\t{i % 3}\t{i}.img\n")
    (tmp_path / "a.lst").write_text("".join(lst))

    def batches(affine_gpu, threads=2):
        cfg = [("iter", "img"), ("image_list", str(tmp_path / "a.lst")), ("image_root", str(tmp_path) + "/"),
               ("rand_crop", "1"), ("rand_mirror", "1"), ("max_rotate_angle", "180"), ("max_aspect_ratio", "0.5"),
               ("max_shear_ratio", "0.3"), ("mean_value", "104,117,123"), ("max_random_contrast", "0.2"),
               ("input_shape", "3,40,40"), ("batch_size", "5"), ("round_batch", "0"), ("silent", "1"),
               ("decode_native_threads", str(threads)), ("decode_process", "0"), ("dev", "cpu"),
               ("affine_gpu", str(affine_gpu)), ("iter", "end")]
        it = create_iterator(cfg)
        it.init()
        out = [(b.data, b.num_batch_padd) for b in it]
        it.close()
        return out
    a, b = batches(1), batches(1, threads=1)
    assert len(a) == 2 and a[1][1] == 2
    for (x, _), (y, _) in zip(a, b):
        assert isinstance(x, ws.WarpImages) and tuple(x.shape) == (5, 3, 40, 40)
        assert torch.equal(x.to_u8().pix, y.to_u8().pix) and torch.equal(x.cm, y.cm)
    last = a[1][0]
    tab = last.table.numpy()
    assert tab[:, ws.VALID].tolist() == [1, 1, 1, 0, 0]  # records 5, 6 (PNG), 7 (CMYK), then padding
    for r in (1, 2):  # the Pillow-decoded rows are staged whole
        assert tab[r, ws.RW] == tab[r, ws.IMG_W] and tab[r, ws.RH] == tab[r, ws.IMG_H] and tab[r, ws.X0] == 0
    u8 = last.to_u8()
    assert not u8.pix[3:].any() and u8.pix[:3].float().std() > 10
    assert set(np.unique(a[0][0].cm[:, 0].numpy()).tolist()) != {1.0}  # contrast drawn
    assert torch.equal(last[1:4].to_u8().pix, u8.pix[1:4])
    assert torch.equal(last.to_float(), u8.to_float())
    assert all(isinstance(x, U8Images) for x, _ in batches(0))
