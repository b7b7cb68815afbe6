"""tests/orient_reference.py against its definition: PIL's Image.transpose and ImageOps.exif_transpose are the table of
include/compeg_hip.h ("Oriented tensor output"); `preimage` maps a rectangle of the upright slot onto the rectangle of T
that `orient` brings there."""
import io

import numpy as np
import pytest

import orient_reference as orf

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageOps  # noqa: E402

A = (np.arange(5 * 7, dtype=np.uint8) * 7 + 3).reshape(5, 7)   # non-square, every element distinct


def test_orientation_1_is_the_identity():
    assert np.array_equal(orf.orient(A, 1), A)


@pytest.mark.parametrize("o", range(2, 9))
def test_orient_is_pils_transpose(o):
    want = np.asarray(Image.fromarray(A).transpose(getattr(Image.Transpose, orf.PIL_TRANSPOSE[o])))
    got = orf.orient(A, o)
    assert got.shape == want.shape == ((7, 5) if o >= 5 else (5, 7))
    assert np.array_equal(got, want)
    # ... and with planes in front, every plane alike
    planes = np.stack([A, A + 1, A + 2])
    assert all(np.array_equal(orf.orient(planes, o)[c], orf.orient(planes[c], o)) for c in range(3))


@pytest.mark.parametrize("o", orf.ORIENTATIONS)
def test_orient_is_exif_transpose_of_a_file_with_that_tag(o):
    image = Image.fromarray(A)
    exif = Image.Exif()
    exif[0x0112] = o
    raw = io.BytesIO()
    image.save(raw, format="PNG", exif=exif)   # (lossless: the elements survive)
    stored = Image.open(io.BytesIO(raw.getvalue()))
    assert stored.getexif().get(0x0112) == o
    assert np.array_equal(np.asarray(ImageOps.exif_transpose(stored)), orf.orient(A, o))


@pytest.mark.parametrize("o", orf.ORIENTATIONS)
@pytest.mark.parametrize("rect", [(2, 4, 20, 6), (23, 19, 1, 1), (0, 0, 24, 20), (7, 0, 9, 20)])
def test_preimage_maps_a_rectangles_ones_onto_its_images_ones(rect, o):
    ow, oh = orf.SLOT
    tw, th = orf.slot_extent(orf.SLOT, o)
    assert (tw, th) == ((oh, ow) if o >= 5 else (ow, oh))
    x, y, w, h = orf.preimage(rect, o, orf.SLOT)
    t = np.zeros((th, tw), np.uint8)
    t[y:y + h, x:x + w] = 1
    u = np.zeros((oh, ow), np.uint8)
    u[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = 1
    assert np.array_equal(orf.orient(t, o), u)


def test_expected_at_orientation_1_is_the_filtered_reference():
    fr = orf.fr
    rgba = fr.frame(50, 26, seed=5)[1]
    scale, bias = fr.params("f16")
    a = orf.expected(rgba, (24, 20), 1, "f16", scale, bias, "rgb", "bicubic", (3, 1, 45, 21), (0, 3, 24, 11), (114, 114, 114), o=1)
    b = fr.expected(rgba, (24, 20), 1, "f16", scale, bias, "rgb", "bicubic", (3, 1, 45, 21), (0, 3, 24, 11), (114, 114, 114))
    assert fr.same(a, b, "f16")


def test_the_resampling_runs_along_the_stored_axes():
    """Orientation 6 of a crop into the upright (13, 31) is the filtered (31, 13) slot turned, not a filtered (13, 31) one."""
    fr = orf.fr
    rgba = fr.frame(330, 70, seed=3)[1]
    scale, bias = fr.params("f32")
    got = orf.expected(rgba, (13, 31), 1, "f32", scale, bias, o=6)
    t = fr.expected(rgba, (31, 13), 1, "f32", scale, bias)
    assert got.shape == (3, 31, 13) and np.array_equal(got, np.rot90(t, -1, (1, 2)))
