"""The image input stage (image_u8_to_nhwc_bf16 and its two fast paths, image_u8c3_nhwc4 and
image_u8c3_nhwc3p) element by element against tests/move_refs.py.

Mode 0 is one multiply and one rounding, so it is compared by equality.  Modes 1 to 3 compute
((d - m) * ct + il) * scale, which the compiler may or may not contract to an FMA; they get the
derived bound of move_refs.image_bound_ref (test_move_refs_cpu.py shows that both forms stay inside
it and that a mean read one column off, an ignored mirror, a dropped crop offset or a neighbour's
contrast do not).  The mean is looked up by explicit index arithmetic, not by U8Images.to_float.
Pad channels must be exactly 0; the row-padded kernel must write its pad columns 0 and the generic
kernel must leave them alone; the node is a view into a sentinel-filled buffer with a guard image
behind the last one; and nhwc_to_nchw of the node must return the float of the stored bf16
exactly.  Every batch has at least two images with distinct contrast and illumination."""
import pytest

import move_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda"

IMAGE = mr.image_cases()


def _run(entry):
    name, mode, B, h, w, C, Cp, Wp, pad_cols = entry
    worst = mr.check_image(mr.image_case_of(entry), Cp, Wp, DEV, pad_cols)
    if mode:
        print("image %s: max d/bound %.3f" % (name, worst))


GENERIC = [e for e in IMAGE if e[0].startswith("generic")]
QUADS = [e for e in IMAGE if e[0].startswith("quads")]
ROWPAD = [e for e in IMAGE if e[0].startswith("rowpad")]


@pytest.mark.parametrize("entry", GENERIC, ids=[e[0] for e in GENERIC])
def test_generic_kernel(entry):
    _run(entry)


@pytest.mark.parametrize("entry", QUADS, ids=[e[0] for e in QUADS])
def test_four_pixel_path_and_its_neighbour(entry):
    """252 pixels in quads that straddle the images (63 pixels each), and 253 pixels, which the
    generic kernel must serve with the same result"""
    _, mode, B, h, w, C, Cp, Wp, _ = entry
    assert (C, Cp, Wp) == (3, 4, w) and B * h * w in (252, 253)
    _run(entry)


@pytest.mark.parametrize("entry", ROWPAD, ids=[e[0] for e in ROWPAD])
def test_row_padded_path(entry):
    _, mode, B, h, w, C, Cp, Wp, pad_cols = entry
    assert (C, Cp) == (3, 3) and Wp % 4 == 0 and Wp >= w
    assert (pad_cols == "zero") == (B * h * w * 3 >= 16)
    _run(entry)
