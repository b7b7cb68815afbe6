"""tests/luma_reference.py against what "L" means elsewhere, and against mutants of itself.  The integer formula with the
BT.601 weights is PIL's Image.convert("L") byte for byte, in RGB and RGBA mode; R = G = B gives that value under every
preset; the f32 expectation is PIL's convert("L") taken to mode F and resized, within test_filter_reference's own cap.
Each mutant -- the rounding constant dropped, the weights applied to block sums, BT.709 for BT.601, float weights rounded
-- changes a named case's expectation.  CPU only."""
import numpy as np
import pytest

import luma_reference as lr
import tensor_reference as tr
from test_filter_reference import _cap

fr = lr.fr
NOISY = tr.frame(330, 70)[1]   # the noisy 330 x 70 frame


def _grid():
    """[n, 1, 3]: every 4th value of each channel with the extremes (65^3 colours), then the other grid: every 5th of R
    and B against all of G's."""
    a = np.array(sorted(set(range(0, 256, 4)) | {255}), np.uint8)
    b = np.array(sorted(set(range(0, 256, 5)) | {255}), np.uint8)
    g = np.arange(256, dtype=np.uint8)
    one = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    two = np.stack(np.meshgrid(b, g, b[::2], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([one, two])[:, None, :]


@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_bt601_is_pils_convert_l_byte_for_byte(mode):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    grid = _grid()
    assert {0, 255} <= set(np.unique(grid)) and len(grid) > 300000
    for rgb in (noise, grid, np.ascontiguousarray(NOISY[..., :3])):
        a = rgb if mode == "RGB" else np.concatenate([rgb, rng.integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)], -1)
        want = np.asarray(Image.fromarray(a, mode).convert("L"))
        got = lr.luma(a, lr.BT601)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} pixels differ"


@pytest.mark.parametrize("weights", list(lr.PRESETS))
def test_a_grey_pixel_keeps_its_value_under_every_preset(weights):
    assert sum(lr.PRESETS[weights]) == 65536
    y = np.arange(256, dtype=np.uint8)
    grey = np.stack([y, y, y, np.full(256, 255, np.uint8)], -1)[None]
    assert np.array_equal(lr.luma(grey, weights)[0], y)


def test_white_is_255_and_its_block_sum_at_8_is_16320():
    white = np.full((16, 24, 4), 255, np.uint8)
    for weights in lr.PRESETS:
        l = lr.luma(white, weights)
        assert (l == 255).all()
        assert int(l[:8, :8].astype(np.uint32).sum()) == 16320 == 64 * 255
        # ... and the slot of the means is 255 exactly: 16320 / 64
        assert (lr.expected(white, (3, 2), 8, "f32", 1.0, 0.0, weights, "box") == np.float32(255)).all()


def test_single_channel_presets_pick_that_channel():
    for c, weights in enumerate(("r", "g", "b")):
        assert np.array_equal(lr.luma(NOISY, weights), NOISY[..., c])


@pytest.mark.parametrize("w, h, size", [(330, 70, (31, 13)), (330, 70, (224, 224)), (50, 26, (5, 3)), (17, 9, (16, 8))])
@pytest.mark.parametrize("kernel", fr.KERNELS)
def test_agrees_with_pil_convert_l_then_resize_in_mode_f(kernel, w, h, size):
    Image = pytest.importorskip("PIL.Image")
    resample = {"box": Image.Resampling.BOX, "triangle": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
                "lanczos3": Image.Resampling.LANCZOS}[kernel]
    rgba = tr.frame(w, h)[1]
    grey = Image.fromarray(np.ascontiguousarray(rgba[..., :3])).convert("L")
    want = np.asarray(grey.convert("F").resize(size, resample), dtype=np.float64)
    got = lr.expected(rgba, size, 1, "f32", 1.0, 0.0, "bt601", kernel)
    p = np.asarray(grey, dtype=np.float32)[None]
    worst, cap = float(np.abs(got.astype(np.float64) - want).max()), _cap(kernel, p, size)
    print(f"{kernel} {w}x{h} -> {size}: max |difference to PIL| {worst:.3e}, cap {cap:.3e}")
    assert got.shape == (size[1], size[0]) and worst <= cap


# ---- mutants: what the reference would be if it were wrong in one of the ways an implementation may be ----------------

def _no_rounding(rgba):
    p = rgba.astype(np.uint32)
    return ((p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471) >> 16).astype(np.uint8)


def _float_weights(rgba):
    p = rgba.astype(np.float64)
    return np.rint(0.299 * p[..., 0] + 0.587 * p[..., 1] + 0.114 * p[..., 2]).astype(np.uint8)


# the named case: the noisy frame into the letterbox slot's extent, bicubic, u8 and f32
CASE = dict(size=(48, 40), k=1, scale=1.0, bias=0.0, kernel="bicubic", dst=(0, 15, 48, 10))


@pytest.mark.parametrize("name, mutant", [("no + 32768", _no_rounding), ("BT.709 for BT.601", lambda a: lr.luma(a, lr.BT709)),
                                          ("float weights 0.299 / 0.587 / 0.114 rounded", _float_weights)])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_a_mutant_of_the_pixel_formula_changes_the_letterbox_case(name, mutant, dtype):
    want = lr.expected(NOISY, dtype=dtype, **CASE)
    got = lr.expected_of(mutant(NOISY), dtype=dtype, **CASE)
    pixels = int((mutant(NOISY) != lr.luma(NOISY)).sum())
    changed = int((got != want).sum())
    print(f"{name}, {dtype}: {pixels} of {NOISY.shape[0] * NOISY.shape[1]} source pixels and {changed} of {want.size} elements change")
    assert pixels > 0 and changed > 0


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_weights_on_the_block_sums_change_the_k2_case(dtype):
    """The mutant takes the 2 x 2 sums of R, G and B first and weighs those: its prefiltered sample is
    float((wR SR + wG SG + wB SB + 32768) >> 16) / 4, one rounding a block where the contract has one a pixel.  Case: the
    noisy frame at k = 2 with box at the prefiltered extent, which is the prefiltered plane itself."""
    h, w = NOISY.shape[0] // 2, NOISY.shape[1] // 2
    want = lr.expected(NOISY, (w, h), 2, dtype, 1.0, 0.0, "bt601", "box")
    sums = NOISY[:h * 2, :w * 2, :3].astype(np.uint32).reshape(h, 2, w, 2, 3).sum(axis=(1, 3), dtype=np.uint32)
    weighed = (sums[..., 0] * np.uint32(19595) + sums[..., 1] * np.uint32(38470) + sums[..., 2] * np.uint32(7471) + np.uint32(32768)) >> np.uint32(16)
    mutant = fr.store((weighed.astype(np.float32) * np.float32(0.25))[None], dtype)[0]
    # (the case is what it is said to be: the per-pixel L, summed and divided)
    block = lr.luma(NOISY)[:h * 2, :w * 2].astype(np.uint32).reshape(h, 2, w, 2).sum(axis=(1, 3), dtype=np.uint32)
    assert np.array_equal(want, fr.store((block.astype(np.float32) * np.float32(0.25))[None], dtype)[0])
    changed = int((mutant != want).sum())
    print(f"weights on block sums, k = 2, {dtype}: {changed} of {want.size} elements change")
    assert changed > 0
