"""GPU affine warp stage (csrc/kernels/warp_kernels.hip via ops.image_warp): the HIP kernel
against the normative numpy warp (io/warp_stage.py warp_reference) -- bit for bit -- and the
iterator's affine_gpu batches through the image kernel into the network input."""
import io

import numpy as np
import pytest
import torch

from cxxnet_amd import ops
from cxxnet_amd.io import warp_stage as ws

from test_jpeg_stage_cpu import _jpeg, _photo
from test_warp_stage_cpu import bowl_aug, make_table, pool_cls, small_records  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


def _png(arr):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG")
    return b.getvalue()


def _decode_full(payload):
    from cxxnet_amd.io.augment import _decode
    return _decode(payload)


def _repack_reversed(src, tab):
    """The same regions laid out in reverse row order: table offsets no longer monotonic."""
    out = np.zeros_like(src)
    o = 0
    for r in range(len(tab) - 1, -1, -1):
        n = int(tab[r, ws.RW] * tab[r, ws.RH] * 3) if tab[r, ws.VALID] else 0
        out[o:o + n] = src[int(tab[r, ws.OFFSET]):int(tab[r, ws.OFFSET]) + n]
        tab[r, ws.OFFSET] = o
        o += n
    return out


@pytest.fixture(scope="module")
def bowl_batch(pool_cls, small_records):  # noqa: F811
    """12 rows, 40 x 40: 7 bowl-like draws over JPEGs and one PNG (Pillow decode), a map with
    negative source coordinates, a 0.5x downscale, a 3 x 5 source (every tap set crosses a
    border), an empty region and a padding row; offsets in non-monotonic order.  Returns (src,
    table, {C: reference})."""
    B, h, w = 12, 40, 40
    rng = np.random.default_rng(8)
    recs = list(small_records[:7]) + [_png(_photo(rng, 61, 77))]
    cfg = ws.warp_cfg(bowl_aug(), 1)
    items = [(r, recs[r], 100 + 13 * r) for r in range(8)]
    src, table, _, _, _, fb = ws.stage_batch(pool_cls(4), items, cfg, B, False, _decode_full)
    assert fb == [7]
    extra = [_photo(rng, 64, 70), _photo(rng, 90, 88), _photo(rng, 5, 3)]
    buf = np.concatenate([src.numpy()] + [e.reshape(-1) for e in extra])
    tab = table.numpy().copy()
    off = int(src.shape[0])
    hand = []
    for row, img, m, fill in [(8, extra[0], (0.9, 0.3, -20.5, -0.3, 0.9, -4.25), 255),  # negative source coordinates
                              (9, extra[1], (2, 0, 3, 0, 2, 5), 17),                    # 0.5x downscale
                              (10, extra[2], (0.11, 0.02, -0.7, -0.03, 0.17, -0.9), 128)]:  # 3 x 5 source
        H, W = img.shape[:2]
        hand.append((row, 1, off, 0, 0, W, H, W, H, m, fill))
        off += img.size
    tab[8:11] = make_table(hand, B)[8:11]
    tab[3, ws.RW] = tab[3, ws.RH] = tab[3, ws.X0] = tab[3, ws.Y0] = 0  # an empty region: all fill
    tab[3, ws.M0 + 2:ws.M0 + 3].view(np.float64)[0] += 5000.0  # (its map is wholly outside the image)
    buf = _repack_reversed(buf, tab)
    assert tab[11, ws.VALID] == 0 and not (np.diff(tab[:11, ws.OFFSET]) >= 0).all()
    refs = {C: ws.warp_reference(buf, tab, 0, B, h, w, C) for C in (3, 1)}
    assert not refs[3][11].any() and (refs[3][3] == 255).all() and refs[3][10].std() > 0
    return torch.from_numpy(buf), torch.from_numpy(tab), refs


@pytest.mark.parametrize("C", [3, 1])
def test_gpu_warp_matches_reference_bowl(bowl_batch, C):
    src, table, refs = bowl_batch
    dev = torch.device("cuda")
    out = ops.image_warp(src, table, 0, 12, 40, 40, C, dev)
    ref = torch.from_numpy(refs[C])
    assert torch.equal(out.cpu(), ref), [r for r in range(12) if not torch.equal(out[r].cpu(), ref[r])]
    part = ops.image_warp(src, table, 3, 11, 40, 40, C, dev)  # a row range is the slice of the full result
    assert torch.equal(part.cpu(), ref[3:11])
    assert ops.image_warp(src, table, 5, 5, 40, 40, C, dev).shape[0] == 0
    staged = [src.to(dev), table.to(dev)]  # prefetched device copies
    assert torch.equal(ops.image_warp(src, table, 0, 12, 40, 40, C, dev, staged).cpu(), ref)


def test_gpu_warp_matches_reference_227(pool_cls):  # noqa: F811
    """4 rows of 227 x 227 (tiles that are no multiple of 16) from 256 x 300 JPEGs, 4:2:0 and 4:4:4."""
    rng = np.random.default_rng(6)
    recs = [_jpeg(_photo(rng, 256, 300), quality=90, subsampling=2), _jpeg(_photo(rng, 256, 300), quality=85, subsampling=0)]
    p = bowl_aug((3, 227, 227))
    p.max_rotate_angle, p.max_shear_ratio, p.max_aspect_ratio = 40, 0.15, 0.1
    cfg = ws.warp_cfg(p, 1)
    items = [(r, recs[r % 2], 7 + 5 * r) for r in range(4)]
    src, table, *_ = ws.stage_batch(pool_cls(2), items, cfg, 4, True, None)
    ref = torch.from_numpy(ws.warp_reference(src.numpy(), table.numpy(), 0, 4, 227, 227, 3))
    out = ops.image_warp(src, table, 0, 4, 227, 227, 3, torch.device("cuda"))
    assert torch.equal(out.cpu(), ref) and ref.float().std() > 10
    assert torch.equal(ops.image_warp(src, table, 1, 3, 227, 227, 3, torch.device("cuda")).cpu(), ref[1:3])


def test_gpu_warp_rejects_bad_tables(bowl_batch):
    src, table, _ = bowl_batch
    dev = torch.device("cuda")
    bad = table.clone()
    bad[0, ws.OFFSET] = src.shape[0] - 5
    with pytest.raises(ValueError, match="outside the packed buffer"):
        ops.image_warp(src, bad, 0, 12, 40, 40, 3, dev)
    bad = table.clone()
    bad[2, ws.IMG_W] = 20000
    with pytest.raises(ValueError, match="16384"):
        ops.image_warp(src, bad, 0, 12, 40, 40, 3, dev)
    with pytest.raises(ValueError, match="inconsistent"):
        ops.image_warp(src, table, 4, 13, 40, 40, 3, dev)


def test_gpu_warp_iterator_end_to_end(tmp_path, small_records):  # noqa: F811
    """affine_gpu = 1 through the trainer's input stage: the GPU warp + image kernel give the same
    bf16 NHWC input as the CPU warp (warp_reference) pushed through the same image kernel, with a
    PNG record (Pillow decode) and a padding row in the batch."""
    from cxxnet_amd.io.iterators import create_iterator
    recs = list(small_records[:7]) + [_png(_photo(np.random.default_rng(1), 66, 71))]
    lst = []
    for i, r in enumerate(recs):
        (tmp_path / f"{i}.img").write_bytes(r)
        lst.append(f"{i}\t{i % 3}\t{i}.img\n")
    (tmp_path / "a.lst").write_text("".join(lst))
    cfg = [("iter", "img"), ("image_list", str(tmp_path / "a.lst")), ("image_root", str(tmp_path) + "/"),
           ("rand_crop", "1"), ("rand_mirror", "1"), ("max_rotate_angle", "180"), ("max_aspect_ratio", "0.5"),
           ("max_shear_ratio", "0.3"), ("min_crop_size", "32"), ("max_crop_size", "48"),
           ("mean_value", "104,117,123"), ("max_random_contrast", "0.2"), ("max_random_illumination", "0.1"),
           ("input_shape", "3,40,40"), ("batch_size", "9"), ("round_batch", "0"), ("silent", "1"),
           ("affine_gpu", "1"), ("iter", "end")]
    it = create_iterator(cfg)
    it.init()
    it.before_first()
    assert it.next()
    batch = it.value()
    it.close()
    d = batch.data
    assert isinstance(d, ws.WarpImages) and batch.num_batch_padd == 1 and d.pf is not None
    node = torch.zeros((9, 40, 40, 4), dtype=torch.bfloat16, device="cuda")
    ops.image_to_nhwc(d, node)
    cpu = d.to_u8()  # warp_reference
    assert cpu.pix[:8].float().std() > 10 and not cpu.pix[8].any()
    node2 = torch.zeros_like(node)
    ops.image_to_nhwc(cpu, node2)
    assert torch.equal(node.float().cpu(), node2.float().cpu())
    assert torch.equal(d.to_u8("cuda").pix.cpu(), cpu.pix)
    assert torch.equal(d[2:9].to_u8("cuda").pix.cpu(), cpu.pix[2:9])


def test_gpu_warp_rate(pool_cls):  # noqa: F811
    """Kernel time of a 256-image AlexNet-size batch (informational; printed)."""
    rng = np.random.default_rng(2)
    recs = [_jpeg(_photo(rng, 256, 300), quality=90, subsampling=2), _jpeg(_photo(rng, 300, 256), quality=90, subsampling=2)]
    p = bowl_aug((3, 227, 227))
    B, h, w = 256, 227, 227
    items = [(r, recs[r % 2], r) for r in range(B)]
    src, table, *_ = ws.stage_batch(pool_cls(8), items, ws.warp_cfg(p, 1), B, True, None)
    dev = torch.device("cuda")
    staged = [src.to(dev), table.to(dev)]
    for _ in range(3):
        ops.image_warp(src, table, 0, B, h, w, 3, dev, staged)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        ops.image_warp(src, table, 0, B, h, w, 3, dev, staged)
    e.record()
    e.synchronize()
    us = s.elapsed_time(e) / 10 * 1e3
    print(f"warp stage: {src.shape[0] / 2 ** 20:.1f} MiB staged, {us:.0f} us per 256-image 227x227 batch "
          f"(kernel + host table check, sources on the device)")
