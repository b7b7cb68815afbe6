"""The resized-tensor entry points that need no device (include/compeg_hip.h, "Resized tensor output"):
compeg_resized_tensor_shape and the rejections it shares with the pack calls, through the C ABI and through the
Python mirror; and the numpy reference (tests/resize_reference.py) against tensor_reference and torch on the CPU."""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import resize_reference as rr
import tensor_reference as tr
from compeg_amd._lib import Rect, ResizeSpec, TensorSpec, lib

U8, F16, BF16, F32 = 0, 1, 2, 3
NEAREST, BILINEAR = 0, 1


def _spec(dtype=F16, order=0, downscale=1, reserved=0):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = (1, 1, 1)
    s.bias[:] = (0, 0, 0)
    return s


def _resize(ow=5, oh=3, filter=BILINEAR, reserved=0):
    return ResizeSpec(ow, oh, filter, reserved)


def _shape(spec, resize, w, h, crop=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_resized_tensor_shape(C.byref(spec) if spec is not None else None, C.byref(resize) if resize is not None else None, w, h,
                                         C.byref(Rect(*crop)) if crop is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_shape_and_byte_count():
    assert _shape(_spec(F16, downscale=2), _resize(24, 20), 50, 26, (3, 1, 45, 21)) == (0, 22, 10, 3 * 20 * 24 * 2)
    assert _shape(_spec(U8, downscale=8), _resize(5, 3), 16, 8) == (0, 2, 1, 45)
    assert _shape(_spec(F32, downscale=1), _resize(224, 224, NEAREST), 330, 70) == (0, 330, 70, 3 * 224 * 224 * 4)
    assert _shape(_spec(BF16, downscale=4), _resize(1, 1), 330, 70, (326, 66, 4, 4)) == (0, 1, 1, 6)


def test_byte_count_does_not_wrap_at_32_bits():
    rc, pw, ph, n = _shape(_spec(F32), _resize(65535, 65535), 16, 8)
    assert (rc, pw, ph) == (0, 16, 8)
    assert n == 3 * 65535 ** 2 * 4 and n > 2 ** 32


def test_outputs_are_optional():
    assert lib.compeg_resized_tensor_shape(C.byref(_spec()), C.byref(_resize()), 16, 8, None, None, None, None) == 0


@pytest.mark.parametrize("spec, resize, w, h, crop, words", [
    (None, _resize(), 16, 8, None, "NULL"),
    (_spec(), None, 16, 8, None, "NULL"),
    (_spec(dtype=4), _resize(), 16, 8, None, "dtype 4"),
    (_spec(order=2), _resize(), 16, 8, None, "order 2"),
    (_spec(downscale=3), _resize(), 16, 8, None, "downscale 3"),
    (_spec(reserved=1), _resize(), 16, 8, None, "reserved"),
    (_spec(), _resize(ow=0), 16, 8, None, "output size"),
    (_spec(), _resize(oh=0), 16, 8, None, "output size"),
    (_spec(), _resize(ow=65536), 16, 8, None, "output size"),
    (_spec(), _resize(oh=70000), 16, 8, None, "output size"),
    (_spec(), _resize(filter=2), 16, 8, None, "filter"),
    (_spec(), _resize(filter=9), 16, 8, None, "filter"),
    (_spec(), _resize(reserved=1), 16, 8, None, "reserved"),
    (_spec(), _resize(), 16, 8, (0, 0, 0, 8), "crop"),
    (_spec(), _resize(), 16, 8, (0, 0, 16, 0), "crop"),
    (_spec(), _resize(), 16, 8, (1, 0, 16, 8), "crop"),
    (_spec(), _resize(), 16, 8, (0, 1, 16, 8), "crop"),
    (_spec(), _resize(), 16, 8, (16, 0, 1, 1), "crop"),
    (_spec(), _resize(), 16, 8, (0xffffffff, 0, 2, 2), "crop"),      # x + width wraps to 1
    (_spec(), _resize(), 16, 8, (0, 0xfffffffe, 2, 4), "crop"),
    (_spec(), _resize(), 16, 8, (8, 0, 0xfffffff9, 2), "crop"),      # ... wraps to 1 as well
    (_spec(downscale=4), _resize(), 16, 8, (2, 2, 3, 6), "3x6"),
    (_spec(downscale=8), _resize(), 16, 8, (0, 0, 16, 7), "16x7"),
    (_spec(downscale=8), _resize(), 7, 5, None, "7x5"),
    (_spec(), _resize(), 0, 9, None, "0x9"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_rejections_carry_a_message(spec, resize, w, h, crop, words):
    rc, pw, ph, n = _shape(spec, resize, w, h, crop)
    assert rc == ca.E_INVALID_ARG
    assert (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and words in message, message
    assert "COMPEG_" not in message   # (values, not macro names: test_shipped_library_has_no_laboratory_switches)


def test_pack_calls_reject_null_handles_and_specs():
    spec, resize = _spec(), _resize()
    for fn in (lib.compeg_decoder_pack_tensor_resized, lib.compeg_batch_pack_tensor_resized):
        assert fn(None, C.byref(spec), C.byref(resize), None, C.c_void_p(256), 1 << 20, None) == ca.E_INVALID_ARG
        assert lib.compeg_last_error().decode()


def test_python_mirror_and_crop_forms():
    assert ca.resized_tensor_shape(50, 26, (24, 20), dtype="f16", downscale=2, crop=(3, 1, 45, 21)) == ((3, 20, 24), 2880, (10, 22))
    assert ca.resized_tensor_shape(16, 8, (5, 3), dtype="u8", downscale=8) == ((3, 3, 5), 45, (1, 2))
    assert ca.resized_tensor_shape(3840, 2160, (224, 224)) == ((3, 224, 224), 3 * 224 * 224 * 2, (2160, 3840))
    assert ca.resized_tensor_shape(330, 70, (64, 64), filter="nearest", crop=[329, 69, 1, 1])[2] == (1, 1)
    assert ca.RESIZE_FILTERS == {"nearest": 0, "bilinear": 1} and "RESIZE_FILTERS" in ca.__all__
    for kwargs in (dict(filter="bicubic"), dict(filter=5), dict(crop=(0, 0, 17, 8)), dict(dtype="f64"), dict(downscale=16)):
        with pytest.raises(ca.Error) as e:
            ca.resized_tensor_shape(16, 8, (5, 3), **kwargs)
        assert str(e.value)
    with pytest.raises(ca.Error) as e:
        ca.resized_tensor_shape(16, 8, (0, 3))
    assert e.value.code == ca.E_INVALID_ARG and "output size" in str(e.value)
    assert hasattr(ca.Decoder, "pack_tensor_resized") and hasattr(ca.Batch, "pack_tensor_resized")
    assert C.sizeof(ca.ResizeSpec) == 16 and C.sizeof(ca.Rect) == 16


# ---- the reference itself ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", rr.FILTERS)
@pytest.mark.parametrize("w, h, k, crop", [(50, 26, 1, None), (50, 26, 2, (3, 1, 45, 21)), (330, 70, 4, (1, 3, 329, 67)), (17, 9, 8, None),
                                           (17, 9, 1, (16, 8, 1, 1))])
def test_identity_extent_is_pack_tensor_of_the_crop(filter, w, h, k, crop):
    rgba = tr.frame(w, h)[1]
    cx, cy, cw, ch = crop or (0, 0, w, h)
    cropped = rgba[cy:cy + ch, cx:cx + cw]
    pw, ph = rr.pre_extent(w, h, k, crop)
    for n, dtype in enumerate(tr.DTYPES):
        scale, bias = rr.params(dtype)
        order = ("rgb", "bgr")[n % 2]
        want = tr.expected(cropped, k, dtype, scale, bias, order)
        got = rr.expected(rgba, (pw, ph), k, dtype, scale, bias, order, filter, crop)
        assert tr.same(got, want, dtype)


def _torch_p(p):
    torch = pytest.importorskip("torch")
    return torch, torch.from_numpy(p)[None]


@pytest.mark.parametrize("w, h, k, size", [(330, 70, 1, (224, 224)), (330, 70, 2, (64, 64)), (17, 9, 1, (64, 64)), (640, 360, 1, (224, 224)),
                                           (50, 26, 2, (5, 3)), (16, 8, 8, (33, 7))])
def test_nearest_is_torch_nearest_exact(w, h, k, size):
    p = rr.prefilter(tr.frame(w, h)[1], k)
    torch, t = _torch_p(p)
    want = torch.nn.functional.interpolate(t, size=(size[1], size[0]), mode="nearest-exact")[0].numpy()
    assert np.array_equal(rr.resample(p, size, "nearest"), want)


@pytest.mark.parametrize("w, h, k, size", [(640, 360, 1, (224, 224)), (330, 70, 1, (224, 224)), (17, 9, 1, (64, 64)), (330, 70, 2, (31, 13)),
                                           (50, 26, 1, (64, 64))])
def test_bilinear_agrees_with_torch_within_coordinate_rounding(w, h, k, size):
    """0.01 on the 0..255 scale caps what the rounding of a coordinate can do (255 * pw * 2^-23, pw <= 640); torch computes
    its ratio and weights in another order of operations."""
    p = rr.prefilter(tr.frame(w, h)[1], k)
    torch, t = _torch_p(p)
    want = torch.nn.functional.interpolate(t, size=(size[1], size[0]), mode="bilinear", align_corners=False, antialias=False)[0].numpy()
    worst = float(np.abs(rr.resample(p, size, "bilinear") - want).max())
    print(f"{w}x{h} k={k} -> {size}: max |difference| {worst:.6f}")
    assert worst <= 0.01


def _floor_stays_inside(n_in, n_out):
    f32 = np.float32
    b = (np.arange(n_out, dtype=np.uint32).astype(f32) + f32(0.5)) * rr.ratio(n_in, n_out)
    s = np.maximum(b - f32(0.5), f32(0))
    return np.floor(b).max() <= n_in - 1 and np.floor(s).max() <= n_in - 1


def test_floor_never_leaves_the_axis():
    """(the clamps to pw - 1 in the formula never bind on floor(b) or floor(s): small extents pairwise, and the largest)"""
    for n_in in range(1, 201, 7):
        for n_out in range(1, 201):
            assert _floor_stays_inside(n_in, n_out), (n_in, n_out)
    for n_in in (8191, 65528, 65535):
        for n_out in (1, 7, 224, 4000, 8191, 65528, 65535):
            assert _floor_stays_inside(n_in, n_out), (n_in, n_out)
