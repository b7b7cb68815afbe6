"""The numpy contract of the filtered tensor output (tests/filter_reference.py) against references from outside: PIL's
Image.resize in mode F for all four kernels, torch's interpolate(antialias=True) in float64 for bicubic and triangle;
and the three properties the header states, with array equality: triangle where both axes shrink is the antialiased
bilinear reference, box at 1/2, 1/4, 1/8 is the block mean, box, triangle and bicubic at the source extent are the
identity."""
import numpy as np
import pytest

import antialias_reference as ar
import filter_reference as fr
import resize_reference as rr
import tensor_reference as tr

# (w, h, size = (ow, oh)): shrinking both ways; 330x70 into 224x224 shrinks on x and grows on y; near the identity; down to
# one element; 96x64 into 40x100 shrinks on x and grows on y, 64x96 into 100x40 the other way round
SHAPES = [(330, 70, (31, 13)), (330, 70, (224, 224)), (50, 26, (5, 3)), (17, 9, (16, 8)), (17, 9, (1, 1)), (96, 64, (40, 100)),
          (64, 96, (100, 40))]


def _source(w, h):
    return rr.prefilter(tr.frame(w, h)[1], 1)


def _cap(kernel, p, size):
    """255 * L * 2^-23 * (Tx + Ty + 4) on the 0..255 scale: one rounding per accumulated tap and 4 for the weights' own
    rounding to f32 on both axes (the antialiased bilinear test's bound), scaled by L, the product over the two axes of the
    largest sum of |w_t| in the reference's own tables: with negative lobes the partial sums a rounding acts on are
    that much larger than the pixel scale."""
    ph, pw = p.shape[1:]
    big = fr.abs_weight_sum(kernel, size[0], pw) * fr.abs_weight_sum(kernel, size[1], ph)
    return 255 * big * 2.0 ** -23 * (fr.taps(kernel, size[0], pw) + fr.taps(kernel, size[1], ph) + 4)


@pytest.mark.parametrize("w, h, size", SHAPES)
@pytest.mark.parametrize("kernel", fr.KERNELS)
def test_agrees_with_pil_within_rounding(kernel, w, h, size):
    Image = pytest.importorskip("PIL.Image")
    resample = {"box": Image.Resampling.BOX, "triangle": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
                "lanczos3": Image.Resampling.LANCZOS}[kernel]
    p = _source(w, h)
    want = np.stack([np.asarray(Image.fromarray(plane, mode="F").resize(size, resample), dtype=np.float64) for plane in p])
    worst = float(np.abs(fr.resample(p, size, kernel).astype(np.float64) - want).max())
    cap = _cap(kernel, p, size)
    print(f"{kernel} {w}x{h} -> {size}: max |difference to PIL| {worst:.3e}, cap {cap:.3e}")
    assert worst <= cap


@pytest.mark.parametrize("w, h, size", SHAPES)
@pytest.mark.parametrize("kernel, mode", [("triangle", "bilinear"), ("bicubic", "bicubic")])
def test_agrees_with_torch_antialias_within_rounding(kernel, mode, w, h, size):
    torch = pytest.importorskip("torch")
    p = _source(w, h)
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None].double(), size=(size[1], size[0]), mode=mode, align_corners=False,
                                           antialias=True)[0].numpy()
    worst = float(np.abs(fr.resample(p, size, kernel).astype(np.float64) - want).max())
    cap = _cap(kernel, p, size)
    print(f"{kernel} {w}x{h} -> {size}: max |difference to torch| {worst:.3e}, cap {cap:.3e}")
    assert worst <= cap


@pytest.mark.parametrize("w, h, k, size, crop", [(330, 70, 1, (31, 13), None), (330, 70, 2, (31, 13), None), (50, 26, 1, (5, 3), None),
                                                 (17, 9, 1, (16, 8), None), (330, 70, 1, (24, 11), (3, 1, 245, 61)), (640, 360, 1, (224, 224), None)])
def test_triangle_where_both_axes_shrink_is_the_antialiased_bilinear(w, h, k, size, crop):
    rgba = tr.frame(w, h)[1]
    p = rr.prefilter(rgba, k, crop)
    assert np.array_equal(fr.resample(p, size, "triangle"), ar.resample(p, size))
    for n, dtype in enumerate(tr.DTYPES):
        scale, bias = rr.params(dtype)
        order = ("rgb", "bgr")[n % 2]
        assert np.array_equal(fr.inner(rgba, size, k, dtype, scale, bias, order, "triangle", crop), ar.expected(rgba, size, k, dtype, scale, bias, order, crop))


@pytest.mark.parametrize("factor", (2, 4, 8))
def test_box_at_a_divisor_is_the_block_mean(factor):
    rgba, crop = tr.frame(330, 70)[1], (2, 6, 320, 64)
    for n, dtype in enumerate(tr.DTYPES):
        scale, bias = rr.params(dtype)
        order = ("rgb", "bgr")[n % 2]
        want = tr.expected(rgba[6:70, 2:322], factor, dtype, scale, bias, order)
        got = fr.inner(rgba, (320 // factor, 64 // factor), 1, dtype, scale, bias, order, "box", crop)
        assert np.array_equal(got, want), dtype


@pytest.mark.parametrize("kernel", ("box", "triangle", "bicubic"))
def test_the_source_extent_is_the_identity(kernel):
    rgba, crop = tr.frame(50, 26)[1], (3, 1, 45, 21)
    for k in (1, 2):
        for n, dtype in enumerate(tr.DTYPES):
            scale, bias = rr.params(dtype)
            order = ("rgb", "bgr")[n % 2]
            want = tr.expected(rgba[1:22, 3:48], k, dtype, scale, bias, order)
            got = fr.inner(rgba, (45 // k, 21 // k), k, dtype, scale, bias, order, kernel, crop)
            assert np.array_equal(got, want), (k, dtype)


def test_tap_counts_stay_within_the_limit():
    for kernel in fr.KERNELS:
        s2 = fr.TWICE_SUPPORT[kernel]
        for n_out in (1, 2, 3, 10, 31):
            n_in = 128 * n_out // s2   # the largest extent the kernel takes
            assert fr.axis_ok(kernel, n_in, n_out) and not fr.axis_ok(kernel, n_in + 1, n_out)
            first, count, w = fr.axis_table(kernel, n_out, n_in)
            assert count.min() >= 1 and count.max() <= 129
            assert first.min() >= 0 and (first + count).max() <= n_in
            assert np.abs(w.astype(np.float64).sum(axis=0) - 1).max() < 1e-5
        for n_in, n_out in ((330, 31), (70, 224), (9, 8), (17, 17), (5, 64)):
            first, count, w = fr.axis_table(kernel, n_out, n_in)
            assert count.min() >= 1 and first.min() >= 0 and (first + count).max() <= n_in
            assert np.all(np.diff(first) >= 0) and np.all(np.diff(first + count) >= 0)   # (what the band's one walk leans on)
