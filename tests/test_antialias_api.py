"""The antialias flag of the resized tensor output where no device is needed (include/compeg_hip.h, "Antialiased
bilinear"): compeg_resized_tensor_shape with the flag, the rejections the flag adds and those it must leave alone,
through the C ABI and the Python mirror; and the numpy reference (tests/antialias_reference.py) against plain bilinear,
against torch's interpolate(antialias=True) on the CPU, and against a mutant of itself with a fused accumulate."""
import ctypes as C

import numpy as np
import pytest

import antialias_reference as ar
import compeg_amd as ca
import resize_reference as rr
import tensor_reference as tr
from compeg_amd._lib import Rect, ResizeSpec, TensorSpec, lib

U8, F16, BF16, F32 = 0, 1, 2, 3
NEAREST, BILINEAR, ANTIALIAS = 0, 1, 0x100
# the f32 contraction shape (the GPU test packs the same): 330x70 noisy -> 31x13, ImageNet scale and bias
CONTRACTION = (330, 70, 1, (31, 13))


def _spec(dtype=F16, order=0, downscale=1, reserved=0):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = (1, 1, 1)
    s.bias[:] = (0, 0, 0)
    return s


def _resize(ow=5, oh=3, filter=BILINEAR | ANTIALIAS, reserved=0):
    return ResizeSpec(ow, oh, filter, reserved)


def _shape(spec, resize, w, h, crop=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_resized_tensor_shape(C.byref(spec) if spec is not None else None, C.byref(resize) if resize is not None else None, w, h,
                                         C.byref(Rect(*crop)) if crop is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_shape_and_byte_count_with_the_flag():
    assert _shape(_spec(F16, downscale=2), _resize(24, 20), 50, 26, (3, 1, 45, 21)) == (0, 22, 10, 3 * 20 * 24 * 2)
    assert _shape(_spec(U8, downscale=8), _resize(5, 3), 16, 8) == (0, 2, 1, 45)
    assert _shape(_spec(F32), _resize(224, 224), 3840, 2160) == (0, 3840, 2160, 3 * 224 * 224 * 4)
    assert _shape(_spec(BF16, downscale=4), _resize(1, 1), 330, 70, (326, 66, 4, 4)) == (0, 1, 1, 6)
    # exactly 64 times either way is taken
    assert _shape(_spec(F16), _resize(5, 1), 320, 64) == (0, 320, 64, 30)


@pytest.mark.parametrize("spec, resize, w, h, crop, words", [
    (_spec(), _resize(filter=NEAREST | ANTIALIAS), 16, 8, None, ("antialias",)),
    (_spec(), _resize(filter=BILINEAR | 0x200), 16, 8, None, ("filter 513",)),
    (_spec(), _resize(filter=BILINEAR | ANTIALIAS | 0x200), 16, 8, None, ("filter 769",)),
    (_spec(), _resize(filter=BILINEAR | 0x80000000), 16, 8, None, ("filter",)),
    (_spec(), _resize(filter=2 | ANTIALIAS), 16, 8, None, ("filter 258",)),
    (_spec(), _resize(5, 3), 330, 70, None, ("antialias", "330x70", "5x3", "downscale")),              # 66 times on x
    (_spec(), _resize(224, 1), 330, 70, None, ("antialias", "330x70", "224x1", "downscale")),          # 70 times on y alone
    (_spec(), _resize(5, 3), 330, 70, (0, 0, 321, 70), ("antialias", "321x70", "5x3", "downscale")),
    (_spec(downscale=2), _resize(2, 3), 330, 70, None, ("antialias", "165x35", "2x3", "downscale")),
    # what is rejected without the flag stays rejected with it, with the same words
    (_spec(dtype=4), _resize(), 16, 8, None, ("dtype 4",)),
    (_spec(order=2), _resize(), 16, 8, None, ("order 2",)),
    (_spec(downscale=3), _resize(), 16, 8, None, ("downscale 3",)),
    (_spec(reserved=1), _resize(), 16, 8, None, ("reserved",)),
    (_spec(), _resize(ow=0), 16, 8, None, ("output size",)),
    (_spec(), _resize(oh=65536), 16, 8, None, ("output size",)),
    (_spec(), _resize(reserved=1), 16, 8, None, ("reserved",)),
    (_spec(), _resize(), 16, 8, (1, 0, 16, 8), ("crop",)),
    (_spec(), _resize(), 16, 8, (0xffffffff, 0, 2, 2), ("crop",)),
    (_spec(downscale=8), _resize(), 7, 5, None, ("7x5",)),
    # ... and so do the filters that never existed
    (_spec(), _resize(filter=2), 16, 8, None, ("filter 2 is neither 0 (nearest) nor 1 (bilinear)",)),
    (_spec(), _resize(filter=5), 16, 8, None, ("filter 5 is neither 0 (nearest) nor 1 (bilinear)",)),
    (_spec(), _resize(filter=9), 16, 8, None, ("filter 9 is neither 0 (nearest) nor 1 (bilinear)",)),
], ids=lambda v: v[0] if isinstance(v, tuple) and v and isinstance(v[0], str) else None)
def test_rejections_carry_a_message(spec, resize, w, h, crop, words):
    rc, pw, ph, n = _shape(spec, resize, w, h, crop)
    assert rc == ca.E_INVALID_ARG
    assert (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message   # (values, not macro names)


def test_ratio_limit_yields_to_a_larger_downscale():
    assert _shape(_spec(), _resize(5, 3), 330, 70)[0] == ca.E_INVALID_ARG
    assert _shape(_spec(), _resize(5, 3, filter=BILINEAR), 330, 70)[0] == 0   # (the limit is the flag's)
    assert _shape(_spec(downscale=2), _resize(5, 3), 330, 70) == (0, 165, 35, 90)
    # 4K to 32 x 32: 120 times at k = 1, 60 at k = 2
    assert _shape(_spec(), _resize(32, 32), 3840, 2160)[0] == ca.E_INVALID_ARG
    assert _shape(_spec(downscale=2), _resize(32, 32), 3840, 2160)[0] == 0


def test_python_keyword():
    assert ca.resized_tensor_shape(50, 26, (24, 20), dtype="f16", downscale=2, crop=(3, 1, 45, 21), antialias=True) == ((3, 20, 24), 2880, (10, 22))
    assert ca.resized_tensor_shape(3840, 2160, (224, 224), antialias=True) == ((3, 224, 224), 3 * 224 * 224 * 2, (2160, 3840))
    assert ca.resized_tensor_shape(330, 70, (5, 3), antialias=False)[2] == (70, 330)
    assert ca.resized_tensor_shape(330, 70, (5, 3), downscale=2, antialias=True)[2] == (35, 165)
    with pytest.raises(ca.Error) as e:
        ca.resized_tensor_shape(330, 70, (5, 3), antialias=True)
    assert e.value.code == ca.E_INVALID_ARG and "antialias" in str(e.value) and "downscale" in str(e.value)
    with pytest.raises(ca.Error) as e:
        ca.resized_tensor_shape(16, 8, (5, 3), filter="nearest", antialias=True)
    assert e.value.code == ca.E_INVALID_ARG and "antialias" in str(e.value)
    assert ca.RESIZE_FILTERS == {"nearest": 0, "bilinear": 1}
    import inspect
    for fn in (ca.resized_tensor_shape, ca.Decoder.pack_tensor_resized, ca.Batch.pack_tensor_resized):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "antialias" and last.default is False
    assert C.sizeof(ca.ResizeSpec) == 16


# ---- the reference itself ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("w, h, size", [(17, 9, (64, 64)), (16, 8, (24, 20)), (50, 26, (50, 26)), (50, 26, (64, 26))])
def test_with_neither_axis_shrinking_it_is_plain_bilinear(w, h, size):
    rgba = tr.frame(w, h)[1]
    p = rr.prefilter(rgba, 1)
    assert np.array_equal(ar.resample(p, size), rr.resample(p, size, "bilinear"))
    for n, dtype in enumerate(tr.DTYPES):
        scale, bias = rr.params(dtype)
        order = ("rgb", "bgr")[n % 2]
        assert rr.same(ar.expected(rgba, size, 1, dtype, scale, bias, order), rr.expected(rgba, size, 1, dtype, scale, bias, order, "bilinear"), dtype)


def test_identity_extent_is_pack_tensor_of_the_crop():
    rgba, crop = tr.frame(50, 26)[1], (3, 1, 45, 21)
    for n, dtype in enumerate(tr.DTYPES):
        scale, bias = rr.params(dtype)
        want = tr.expected(rgba[1:22, 3:48], 2, dtype, scale, bias, ("rgb", "bgr")[n % 2])
        assert tr.same(ar.expected(rgba, (22, 10), 2, dtype, scale, bias, ("rgb", "bgr")[n % 2], crop), want, dtype)


def _source(w, h, k):
    if (w, h) == (3840, 2160):   # random P: no frame of this size is decoded for a test
        return np.random.default_rng(1).integers(0, 256, (3, h, w)).astype(np.float32)
    return rr.prefilter(tr.frame(w, h)[1], k)


@pytest.mark.parametrize("w, h, k, size", [(330, 70, 1, (224, 224)), (330, 70, 1, (31, 13)), (330, 70, 2, (31, 13)), (50, 26, 1, (5, 3)),
                                           (17, 9, 1, (16, 8)), (17, 9, 1, (1, 1)), (640, 360, 1, (224, 224)), (3840, 2160, 1, (224, 224))])
def test_agrees_with_torch_antialias_within_rounding(w, h, k, size):
    """The cap on the largest difference, 0..255 scale: 255 * 2^-23 * (B + Tx + Ty + 4).  B, the largest prefiltered extent
    among the axes that do not shrink (0 if none), is what the f32 rounding of a coordinate can do there (the plain
    bilinear test's term); Tx and Ty, the largest tap counts, one rounding per accumulated tap; 4 for the weights' own
    rounding to f32 on both axes.  torch runs in float64."""
    torch = pytest.importorskip("torch")
    p = _source(w, h, k)
    ph, pw = p.shape[1:]
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None].double(), size=(size[1], size[0]), mode="bilinear", align_corners=False,
                                           antialias=True)[0].numpy()
    worst = float(np.abs(ar.resample(p, size).astype(np.float64) - want).max())
    b = max([n for n, o in ((pw, size[0]), (ph, size[1])) if n <= o] or [0])
    cap = 255 * 2.0 ** -23 * (b + ar.taps(size[0], pw) + ar.taps(size[1], ph) + 4)
    print(f"{w}x{h} k={k} -> {size}: max |difference| {worst:.6f}, cap {cap:.6f}")
    assert worst <= cap


def test_tap_counts_stay_within_the_ratio_limit():
    for n_in, n_out in ((64, 1), (640, 10), (4096, 64), (65535, 1024), (330, 31), (129, 2), (8191, 4000)):
        first, count, w = ar.axis_table(n_out, n_in)
        assert count.min() >= 1 and count.max() <= 2 * ar.MAX_RATIO + 1
        assert first.min() >= 0 and (first + count).max() <= n_in   # (the clamp never binds on a shrinking axis)
        assert np.abs(w.astype(np.float64).sum(axis=0) - 1).max() < 1e-5


def test_a_fused_accumulate_shows():
    """h + (P * w) is what a compiler contracts into an fma; the contract forbids it, and on this shape it changes elements."""
    w, h, k, size = CONTRACTION
    rgba = tr.frame(w, h)[1]
    want = ar.expected(rgba, size, k, "f32", rr.IMAGENET_SCALE, rr.IMAGENET_BIAS)
    mutant = ar.expected(rgba, size, k, "f32", rr.IMAGENET_SCALE, rr.IMAGENET_BIAS, fused=True)
    differing = int((want != mutant).sum())
    print(f"{w}x{h} -> {size}: {differing} of {want.size} elements differ under a fused accumulate")
    assert differing >= 1
