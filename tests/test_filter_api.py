"""The filtered tensor output where no device is needed (include/compeg_hip.h, "Filtered tensor output"):
compeg_filtered_tensor_shape through the C ABI -- shapes, byte counts, every rejection with its message, the tap limit
met and passed by one sample for each kernel --, what the pack calls reject before they look at their object, and the
Python mirror."""
import ctypes as C

import pytest

import compeg_amd as ca
from compeg_amd._lib import FilterSpec, Rect, Region, TensorSpec, lib

U8, F16, BF16, F32 = 0, 1, 2, 3
BOX, TRIANGLE, BICUBIC, LANCZOS3 = 0, 1, 2, 3
# kernel -> (2S, the largest reduction in whole numbers)
LIMITS = {BOX: (1, 128), TRIANGLE: (2, 64), BICUBIC: (4, 32), LANCZOS3: (6, 21)}
NAMES = {BOX: "box", TRIANGLE: "triangle", BICUBIC: "bicubic", LANCZOS3: "lanczos3"}


def _spec(dtype=F16, order=0, downscale=1, reserved=0):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = (1, 1, 1)
    s.bias[:] = (0, 0, 0)
    return s


def _filter(ow=5, oh=3, kernel=BICUBIC, reserved=0):
    return FilterSpec(ow, oh, kernel, reserved)


def _region(image=0, src=(0, 0, 0, 0), dst=(0, 0, 0, 0), reserved=0):
    return Region(image, reserved, Rect(*src), Rect(*dst))


def _shape(spec, filter, w, h, region=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_filtered_tensor_shape(C.byref(spec) if spec is not None else None, C.byref(filter) if filter is not None else None, w, h,
                                          C.byref(region) if region is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_struct_sizes():
    assert C.sizeof(FilterSpec) == 16 and C.sizeof(Region) == 40 and C.sizeof(TensorSpec) == 40 and C.sizeof(Rect) == 16
    assert C.sizeof(ca.FilterSpec) == 16


def test_shapes_and_byte_counts():
    assert _shape(_spec(F16, downscale=2), _filter(24, 20), 50, 26, _region(src=(3, 1, 45, 21))) == (0, 22, 10, 3 * 20 * 24 * 2)
    assert _shape(_spec(U8, downscale=8), _filter(5, 3, BOX), 16, 8) == (0, 2, 1, 45)
    assert _shape(_spec(F32), _filter(224, 224, LANCZOS3), 3840, 2160) == (0, 3840, 2160, 3 * 224 * 224 * 4)
    assert _shape(_spec(BF16, downscale=4), _filter(1, 1, TRIANGLE), 330, 70, _region(src=(326, 66, 4, 4))) == (0, 1, 1, 6)
    # the slot's bytes are the output's, not the inner rectangle's; growing is taken
    assert _shape(_spec(F32), _filter(48, 40), 330, 70, _region(dst=(0, 15, 48, 10))) == (0, 330, 70, 3 * 40 * 48 * 4)
    assert _shape(_spec(U8), _filter(640, 360, BICUBIC), 17, 9) == (0, 17, 9, 3 * 360 * 640)
    # the outputs are optional
    assert lib.compeg_filtered_tensor_shape(C.byref(_spec()), C.byref(_filter()), 16, 8, None, None, None, None) == 0


@pytest.mark.parametrize("kernel", LIMITS)
def test_the_tap_limit_is_met_and_one_sample_more_is_not(kernel):
    twice_support, most = LIMITS[kernel]
    for o in (1, 2, 3, 7):
        n = 128 * o // twice_support   # the largest n with n * 2S <= 128 * o
        assert n * twice_support <= 128 * o < (n + 1) * twice_support
        # ... on x alone, on y alone, against the whole output and against an inner rectangle
        assert _shape(_spec(), _filter(o, 9, kernel), n, 9)[:3] == (0, n, 9)
        assert _shape(_spec(), _filter(9, o, kernel), 9, n)[:3] == (0, 9, n)
        assert _shape(_spec(), _filter(20, 20, kernel), n, 9, _region(dst=(3, 5, o, 9)))[0] == 0
        assert _shape(_spec(downscale=2), _filter(o, 9, kernel), 2 * n + 1, 18)[:3] == (0, n, 9)
        for args, extents in (((_spec(), _filter(o, 9, kernel), n + 1, 9), (f"{n + 1}x9", f"{o}x9")),
                              ((_spec(), _filter(9, o, kernel), 9, n + 1), (f"9x{n + 1}", f"9x{o}")),
                              ((_spec(), _filter(20, 20, kernel), n + 1, 9, _region(dst=(3, 5, o, 9))), (f"{n + 1}x9", f"{o}x9")),
                              ((_spec(downscale=2), _filter(o, 9, kernel), 2 * n + 2, 18), (f"{n + 1}x9", f"{o}x9"))):
            rc, pw, ph, nbytes = _shape(*args)
            message = lib.compeg_last_error().decode()
            assert rc == ca.E_INVALID_ARG and (pw, ph, nbytes) == (0xdead, 0xdead, 0xdead)
            assert all(w in message for w in extents + (NAMES[kernel], f"by {most} at the most", "downscale")), message
            assert "COMPEG_" not in message


def test_the_tap_limit_yields_to_a_larger_downscale():
    # 4K to 64 x 64: 60 times at k = 1 is box's and triangle's, 30 at k = 2 bicubic's, 15 at k = 4 Lanczos'
    for kernel, k in ((BOX, 1), (TRIANGLE, 1), (BICUBIC, 2), (LANCZOS3, 4)):
        assert _shape(_spec(downscale=k), _filter(64, 64, kernel), 3840, 2160)[0] == 0
        if k > 1:
            assert _shape(_spec(downscale=k // 2), _filter(64, 64, kernel), 3840, 2160)[0] == ca.E_INVALID_ARG


@pytest.mark.parametrize("spec, filter, w, h, region, words", [
    (_spec(), _filter(kernel=4), 16, 8, None, ("kernel 4 is none of 0 (box), 1 (triangle), 2 (bicubic), 3 (lanczos3)",)),
    (_spec(), _filter(kernel=7), 16, 8, None, ("kernel 7 is none of 0 (box), 1 (triangle), 2 (bicubic), 3 (lanczos3)",)),
    (_spec(), _filter(kernel=0x101), 16, 8, None, ("kernel 257",)),
    (_spec(), _filter(kernel=0x80000002), 16, 8, None, ("kernel",)),
    (_spec(), _filter(reserved=1), 16, 8, None, ("filter", "reserved")),
    (_spec(), _filter(ow=0), 16, 8, None, ("output size 0x3",)),
    (_spec(), _filter(oh=65536), 16, 8, None, ("output size 5x65536",)),
    (None, _filter(), 16, 8, None, ("spec is NULL",)),
    (_spec(), None, 16, 8, None, ("filter is NULL",)),
    # the tensor spec's
    (_spec(dtype=4), _filter(), 16, 8, None, ("dtype 4",)),
    (_spec(order=2), _filter(), 16, 8, None, ("order 2",)),
    (_spec(downscale=3), _filter(), 16, 8, None, ("downscale 3",)),
    (_spec(reserved=1), _filter(), 16, 8, None, ("tensor spec", "reserved")),
    # what compeg_region_tensor_shape rejects of a region
    (_spec(), _filter(), 16, 8, _region(reserved=1), ("reserved",)),
    (_spec(), _filter(), 16, 8, _region(src=(1, 0, 16, 8)), ("crop 16x8", "leaves", "16x8 image")),
    (_spec(), _filter(), 16, 8, _region(src=(0xffffffff, 0, 2, 2)), ("crop", "leaves")),
    (_spec(), _filter(), 16, 8, _region(src=(3, 3, 0, 5)), ("crop", "side of 0")),
    (_spec(), _filter(), 16, 8, _region(dst=(0, 0, 5, 0)), ("dst", "side of 0")),
    (_spec(), _filter(), 16, 8, _region(dst=(1, 0, 5, 3)), ("dst 5x3", "leaves", "5x3 output")),
    (_spec(), _filter(), 16, 8, _region(dst=(0, 0xffffffff, 5, 3)), ("dst", "leaves")),
    (_spec(downscale=8), _filter(), 7, 5, None, ("7x5", "downscale factor 8")),
    (_spec(downscale=4), _filter(), 16, 8, _region(src=(0, 0, 4, 3)), ("4x3", "downscale factor 4")),
], ids=lambda v: v[0] if isinstance(v, tuple) and v and isinstance(v[0], str) else None)
def test_rejections_carry_a_message(spec, filter, w, h, region, words):
    rc, pw, ph, n = _shape(spec, filter, w, h, region)
    assert rc == ca.E_INVALID_ARG
    assert (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message   # (values, not macro names)


@pytest.mark.parametrize("call", ("compeg_decoder_pack_tensor_filtered", "compeg_batch_pack_tensor_filtered"))
def test_the_pack_calls_check_their_arguments_before_their_object(call):
    """With no decoder or batch at all -- the object is NULL --, what does not depend on it is rejected first, with its own
    message; only a call that got past all that says that the object is missing."""
    fn = getattr(lib, call)
    one = (Region * 1)(_region())
    pad = (C.c_float * 3)(0, 0, 0)

    def said(spec, filter, regions, count, pad_):
        rc = fn(None, C.byref(spec), C.byref(filter) if filter is not None else None, regions, count, pad_, None, 0, None)
        assert rc == ca.E_INVALID_ARG
        return lib.compeg_last_error().decode()
    assert "kernel 9 is none of 0 (box), 1 (triangle), 2 (bicubic), 3 (lanczos3)" in said(_spec(), _filter(kernel=9), one, 1, pad)
    assert "reserved" in said(_spec(), _filter(reserved=2), one, 1, pad)
    assert "output size" in said(_spec(), _filter(ow=0), one, 1, pad)
    assert "dtype 5" in said(_spec(dtype=5), _filter(), one, 1, pad)
    assert "filter is NULL" in said(_spec(), None, one, 1, pad)
    assert "regions is NULL" in said(_spec(), _filter(), None, 1, pad)
    assert "region count of 0" in said(_spec(), _filter(), one, 0, pad)
    for c, bad in enumerate((float("inf"), float("nan"), float("-inf"))):
        values = [0.0, 0.0, 0.0]
        values[c] = bad
        message = said(_spec(), _filter(), one, 1, (C.c_float * 3)(*values))
        assert "pad" in message and f"channel {c}" in message and "finite" in message, message
    assert "NULL" in said(_spec(), _filter(), one, 1, pad)   # (the object, at last)
    assert "NULL" in said(_spec(), _filter(), one, 1, None)   # (pad NULL is zeros, not an error)


def test_python_mirror():
    assert ca.FILTER_KERNELS == {"box": 0, "triangle": 1, "bicubic": 2, "lanczos3": 3}
    assert ca.RESIZE_FILTERS == {"nearest": 0, "bilinear": 1}
    for name in ("FILTER_KERNELS", "FilterSpec", "filtered_tensor_shape"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert ca.filtered_tensor_shape(50, 26, (24, 20), (0, (3, 1, 45, 21), None), dtype="f16", downscale=2) == ((3, 20, 24), 2880, (10, 22))
    assert ca.filtered_tensor_shape(3840, 2160, (224, 224), kernel="lanczos3") == ((3, 224, 224), 3 * 224 * 224 * 2, (2160, 3840))
    assert ca.filtered_tensor_shape(330, 70, (48, 40), (0, None, ca.region_fit((330, 70), (48, 40))), kernel="box", dtype="u8")[1] == 3 * 40 * 48
    assert ca.filtered_tensor_shape(16, 8, (5, 3), kernel=3)[2] == (8, 16)   # (the header's number)
    with pytest.raises(ca.Error) as e:
        ca.filtered_tensor_shape(330, 70, (5, 3))   # bicubic: 66 times on x
    assert e.value.code == ca.E_INVALID_ARG and all(w in str(e.value) for w in ("bicubic", "330x70", "5x3", "downscale"))
    assert ca.filtered_tensor_shape(330, 70, (5, 3), kernel="box")[2] == (70, 330)
    assert ca.filtered_tensor_shape(330, 70, (5, 3), downscale=4)[2] == (17, 82)
    with pytest.raises(ca.Error) as e:
        ca.filtered_tensor_shape(16, 8, (5, 3), kernel="lanczos")
    assert "unknown filter kernel" in str(e.value) and "lanczos3" in str(e.value)
    with pytest.raises(ca.Error) as e:
        ca.filtered_tensor_shape(16, 8, (5, 3), kernel=4)
    assert "kernel 4" in str(e.value)
    import inspect
    for fn in (ca.Decoder.pack_tensor_filtered, ca.Batch.pack_tensor_filtered):
        p = inspect.signature(fn).parameters
        assert list(p)[:4] == ["self", "dst", "size", "regions"] and p["regions"].default is None
        assert p["kernel"].default == "bicubic" and p["pad"].default == (0, 0, 0) and p["hip_stream"].default == 0
