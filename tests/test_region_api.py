"""The region tensor output where no device is needed (include/compeg_hip.h, "Region tensor output"): compeg_region_fit
against Python integers, compeg_region_tensor_shape against compeg_resized_tensor_shape, every rejection that needs no
decode with its message words, the struct's size, the Python mirror, and the numpy reference (tests/region_reference.py)
against the resized references where dst is the whole output."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import compeg_amd as ca
import region_reference as gr
from compeg_amd._lib import Rect, Region, ResizeSpec, TensorSpec, lib
from conftest import ROOT

U8, F16, BF16, F32 = 0, 1, 2, 3
NEAREST, BILINEAR, ANTIALIAS = 0, 1, 0x100
CENTER, TOP_LEFT = 0, 1


def _spec(dtype=F16, order=0, downscale=1, reserved=0, scale=(1, 1, 1), bias=(0, 0, 0)):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = scale
    s.bias[:] = bias
    return s


def _resize(ow=24, oh=20, filter=BILINEAR, reserved=0):
    return ResizeSpec(ow, oh, filter, reserved)


def _region(image=0, src=None, dst=None, reserved=0):
    return Region(image, reserved, Rect(*(src or (0, 0, 0, 0))), Rect(*(dst or (0, 0, 0, 0))))


def _fit(sw, sh, ow, oh, align=CENTER):
    r = Rect(0xdead, 0xdead, 0xdead, 0xdead)
    rc = lib.compeg_region_fit(sw, sh, ow, oh, align, C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


def _shape(spec, resize, w, h, region=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_region_tensor_shape(C.byref(spec) if spec is not None else None, C.byref(resize) if resize is not None else None, w, h,
                                        C.byref(region) if region is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def _resized_shape(spec, resize, w, h, crop=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_resized_tensor_shape(C.byref(spec), C.byref(resize), w, h, C.byref(Rect(*crop)) if crop is not None else None, C.byref(pw),
                                         C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def _message():
    return lib.compeg_last_error().decode()


# ---- compeg_region_fit ---------------------------------------------------------------------------------------------

def test_fit_examples_of_the_header():
    assert _fit(3840, 2160, 640, 640) == (0, (0, 140, 640, 360))
    assert _fit(330, 70, 48, 40) == (0, (0, 15, 48, 10))
    assert _fit(330, 70, 48, 40, TOP_LEFT) == (0, (0, 0, 48, 10))
    assert _fit(2160, 3840, 640, 640) == (0, (140, 0, 360, 640))
    assert _fit(64, 64, 7, 7) == (0, (0, 0, 7, 7))


def _check_fit(sw, sh, ow, oh):
    for align, name in ((CENTER, "center"), (TOP_LEFT, "top_left")):
        want = gr.fit((sw, sh), (ow, oh), name)
        assert _fit(sw, sh, ow, oh, align) == (0, want), (sw, sh, ow, oh, name)
        dx, dy, dw, dh = want
        assert 1 <= dw <= ow and 1 <= dh <= oh and dx + dw <= ow and dy + dh <= oh and (dw == ow or dh == oh)


def test_fit_against_python_integers_over_all_extents_1_to_64(tmp_path):
    """Every source extent 1..64 each way into every output extent 1..64 each way, both placements: 2 x 16.8 million
    calls of the library, made by a C99 program (tests/emul_region/fit_driver.c, built here and linked with the library
    like tests/c_consumer) against a table computed here in 64-bit integers by the header's formula; the table itself is
    region_reference.fit's Python integers wherever it is looked at."""
    n = np.arange(1, 65, dtype=np.int64)
    sw, sh, ow, oh = np.meshgrid(n, n, n, n, indexing="ij")
    wide = ow * sh <= oh * sw
    dh = np.where(wide, np.clip((2 * sh * ow + sw) // (2 * sw), 1, oh), oh)
    dw = np.where(wide, ow, np.clip((2 * sw * oh + sh) // (2 * sh), 1, ow))
    table = np.stack([(ow - dw) // 2, (oh - dh) // 2, dw, dh], axis=-1).astype(np.uint8)
    rng = np.random.default_rng(5)
    for a, b, c, d in [(1, 1, 1, 1), (64, 64, 64, 64), (1, 64, 64, 1), (64, 1, 1, 64), (33, 7, 48, 40)] + rng.integers(1, 65, (2000, 4)).tolist():
        assert tuple(int(v) for v in table[a - 1, b - 1, c - 1, d - 1]) == gr.fit((a, b), (c, d)), (a, b, c, d)
    (tmp_path / "table.bin").write_bytes(table.tobytes())
    exe, libdir = str(tmp_path / "fit_driver"), os.path.dirname(ca.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "emul_region", "fit_driver.c"), "-o", exe, "-L", libdir, "-l:libcompeg_hip.so",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "64", str(tmp_path / "table.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"calls {2 * 64 ** 4} wrong 0" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]


def test_fit_at_the_largest_extents_and_at_strips():
    big = (1, 2, 63, 64, 65534, 65535)
    for sw in big:
        for sh in big:
            for ow in big:
                for oh in big:
                    _check_fit(sw, sh, ow, oh)
    for n in (1, 2, 3, 5, 64, 1000, 65535):
        for o in ((1, 1), (640, 640), (65535, 1), (1, 65535), (48, 40)):
            _check_fit(1, n, *o)
            _check_fit(n, 1, *o)
    _check_fit(0xffffffff, 1, 65535, 65535)
    _check_fit(1, 0xffffffff, 65535, 65535)
    _check_fit(0xffffffff, 0xffffffff, 65535, 65534)
    _check_fit(0xffffffff, 0xfffffffe, 65535, 65535)


@pytest.mark.parametrize("args, words", [
    ((0, 8, 4, 4, CENTER), ("source", "0x8")),
    ((8, 0, 4, 4, CENTER), ("source", "8x0")),
    ((8, 8, 0, 4, CENTER), ("output size", "0x4")),
    ((8, 8, 4, 65536, CENTER), ("output size", "4x65536")),
    ((8, 8, 4, 4, 2), ("align 2",)),
])
def test_fit_rejections(args, words):
    rc, rect = _fit(*args)
    assert rc == ca.E_INVALID_ARG and rect == (0xdead,) * 4
    assert all(w in _message() for w in words), _message()
    assert lib.compeg_region_fit(8, 8, 4, 4, CENTER, None) == ca.E_INVALID_ARG and "dst" in _message()


# ---- compeg_region_tensor_shape ------------------------------------------------------------------------------------

def test_struct_sizes():
    assert C.sizeof(Region) == 40 and C.sizeof(Rect) == 16 and C.sizeof(ResizeSpec) == 16 and C.sizeof(TensorSpec) == 40
    assert (Region.image.offset, Region.reserved.offset, Region.src.offset, Region.dst.offset) == (0, 4, 8, 24)
    assert ca.Region is Region


@pytest.mark.parametrize("flag", (0, ANTIALIAS))
def test_shape_is_the_resized_shape_of_the_crop_at_the_inner_extent(flag):
    for spec, size, w, h, src, dst in ((_spec(F16, downscale=2), (24, 20), 50, 26, (3, 1, 45, 21), None),
                                       (_spec(U8, downscale=8), (5, 3), 16, 8, None, None),
                                       (_spec(F32), (640, 640), 3840, 2160, None, (0, 140, 640, 360)),
                                       (_spec(BF16, downscale=4), (33, 17), 330, 70, (326, 66, 4, 4), (32, 16, 1, 1)),
                                       (_spec(F16), (48, 40), 330, 70, None, (0, 15, 48, 10))):
        resize = _resize(*size, filter=BILINEAR | flag)
        inner = _resize(*(dst[2:] if dst else size), filter=BILINEAR | flag)
        rc, pw, ph, _ = _resized_shape(spec, inner, w, h, src)
        slot = 3 * size[1] * size[0] * (1, 2, 2, 4)[spec.dtype]
        assert rc == 0
        assert _shape(spec, resize, w, h, _region(0, src, dst)) == (0, pw, ph, slot)
    # NULL: the whole image into the whole output; the image index is not this call's to check
    assert _shape(_spec(F16), _resize(24, 20), 50, 26, None) == (0, 50, 26, 3 * 20 * 24 * 2)
    assert _shape(_spec(F16), _resize(24, 20), 50, 26, _region(image=7)) == (0, 50, 26, 3 * 20 * 24 * 2)


def test_antialias_limit_is_taken_against_the_inner_extent():
    aa = BILINEAR | ANTIALIAS
    assert _shape(_spec(), _resize(64, 64, aa), 330, 70, _region(dst=(0, 0, 6, 2)))[0] == 0          # 55 and 35 times
    assert _shape(_spec(), _resize(64, 64, aa), 330, 70, _region(dst=(0, 0, 5, 2)))[0] == ca.E_INVALID_ARG   # 66 times on x
    assert all(w in _message() for w in ("antialias", "330x70", "5x2", "downscale"))
    assert _shape(_spec(downscale=2), _resize(64, 64, aa), 330, 70, _region(dst=(0, 0, 5, 2))) == (0, 165, 35, 3 * 64 * 64 * 2)
    assert _shape(_spec(), _resize(64, 64, aa), 330, 70, _region(dst=(3, 3, 40, 1)))[0] == ca.E_INVALID_ARG  # 70 times on y
    assert _shape(_spec(), _resize(64, 64, BILINEAR), 330, 70, _region(dst=(0, 0, 5, 2)))[0] == 0     # (the limit is the flag's)
    assert _shape(_spec(), _resize(5, 2, aa), 330, 70, _region(src=(0, 0, 320, 70)))[0] == 0          # exactly 64 times is taken


@pytest.mark.parametrize("spec, resize, w, h, region, words", [
    # everything compeg_resized_tensor_shape rejects, with its words
    (_spec(dtype=4), _resize(), 16, 8, _region(), ("dtype 4",)),
    (_spec(order=2), _resize(), 16, 8, _region(), ("order 2",)),
    (_spec(downscale=3), _resize(), 16, 8, _region(), ("downscale 3",)),
    (_spec(reserved=1), _resize(), 16, 8, _region(), ("tensor spec", "reserved")),
    (_spec(scale=(1, float("inf"), 1)), _resize(), 16, 8, _region(), ("plane 1", "finite")),
    (_spec(bias=(0, 0, float("nan"))), _resize(), 16, 8, _region(), ("plane 2", "finite")),
    (_spec(), _resize(ow=0), 16, 8, _region(), ("output size",)),
    (_spec(), _resize(oh=65536), 16, 8, _region(), ("output size",)),
    (_spec(), _resize(reserved=1), 16, 8, _region(), ("resize", "reserved")),
    (_spec(), _resize(filter=2), 16, 8, _region(), ("filter 2",)),
    (_spec(), _resize(filter=NEAREST | ANTIALIAS), 16, 8, _region(), ("antialias",)),
    (_spec(), _resize(filter=BILINEAR | 0x200), 16, 8, _region(), ("filter 513",)),
    (_spec(downscale=8), _resize(), 7, 5, _region(), ("7x5", "downscale factor 8")),
    # the region's own
    (_spec(), _resize(), 16, 8, _region(reserved=1), ("reserved",)),
    (_spec(), _resize(), 16, 8, _region(src=(1, 0, 16, 8)), ("crop", "leaves", "16x8")),
    (_spec(), _resize(), 16, 8, _region(src=(0xffffffff, 0, 2, 2)), ("crop", "leaves")),
    (_spec(), _resize(), 16, 8, _region(src=(0, 0, 0, 8)), ("crop", "side of 0")),
    (_spec(), _resize(), 16, 8, _region(src=(3, 0, 0, 0)), ("crop", "side of 0")),
    (_spec(), _resize(), 16, 8, _region(src=(0, 0, 4, 0)), ("crop", "side of 0")),
    (_spec(downscale=4), _resize(), 16, 8, _region(src=(2, 2, 8, 3)), ("8x3", "downscale factor 4")),
    (_spec(), _resize(), 16, 8, _region(dst=(0, 0, 0, 5)), ("dst", "side of 0")),
    (_spec(), _resize(), 16, 8, _region(dst=(1, 1, 0, 0)), ("dst", "side of 0")),
    (_spec(), _resize(), 16, 8, _region(dst=(1, 0, 24, 20)), ("dst 24x20", "(1, 0)", "leaves", "24x20 output")),
    (_spec(), _resize(), 16, 8, _region(dst=(0, 19, 5, 2)), ("dst 5x2", "leaves")),
    (_spec(), _resize(), 16, 8, _region(dst=(0xffffffff, 0, 2, 2)), ("dst", "leaves")),
    (_spec(), _resize(64, 64, BILINEAR | ANTIALIAS), 330, 70, _region(dst=(8, 8, 5, 3)), ("antialias", "330x70", "5x3", "downscale")),
], ids=lambda v: "-".join(v) if isinstance(v, tuple) and v and isinstance(v[0], str) else None)
def test_shape_rejections_carry_a_message(spec, resize, w, h, region, words):
    rc, pw, ph, n = _shape(spec, resize, w, h, region)
    assert rc == ca.E_INVALID_ARG
    assert (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = _message()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message   # (values, not macro names)


def test_null_specs():
    assert _shape(None, _resize(), 16, 8)[0] == ca.E_INVALID_ARG and "spec" in _message()
    assert _shape(_spec(), None, 16, 8)[0] == ca.E_INVALID_ARG and "resize" in _message()


# ---- the pack calls, as far as they go without an object -----------------------------------------------------------

@pytest.mark.parametrize("call", ("compeg_decoder_pack_tensor_regions", "compeg_batch_pack_tensor_regions"))
def test_pack_rejections_that_need_no_object(call):
    fn = getattr(lib, call)
    regions, pad = (Region * 2)(_region(), _region()), (C.c_float * 3)(114, 114, 114)
    spec, resize = _spec(), _resize()

    def run(spec=spec, resize=resize, regions=regions, count=2, pad=pad):
        rc = fn(None, C.byref(spec) if spec is not None else None, C.byref(resize) if resize is not None else None, regions, count, pad, None, 0, None)
        assert rc == ca.E_INVALID_ARG
        return _message()
    assert "spec" in run(spec=None)
    assert "dtype 9" in run(spec=_spec(dtype=9))
    assert "resize" in run(resize=None)
    assert "filter 7" in run(resize=_resize(filter=7))
    assert "regions is NULL" in run(regions=None)
    assert "count of 0" in run(count=0)
    for c, bad in enumerate((float("inf"), float("-inf"), float("nan"))):
        p = (C.c_float * 3)(114, 114, 114)
        p[c] = bad
        m = run(pad=p)
        assert "pad" in m and f"channel {c}" in m and "finite" in m
    assert "is NULL" in run() and "regions" not in run()   # all of that in order: the object is what is missing


# ---- the Python mirror ---------------------------------------------------------------------------------------------

def test_python_mirror():
    assert ca.region_fit((3840, 2160), (640, 640)) == (0, 140, 640, 360)
    assert ca.region_fit((330, 70), (48, 40)) == (0, 15, 48, 10)
    assert ca.region_fit((330, 70), (48, 40), align="top_left") == (0, 0, 48, 10)
    assert ca.region_fit((330, 70), (48, 40), align=1) == (0, 0, 48, 10)
    with pytest.raises(ca.Error):
        ca.region_fit((330, 70), (48, 40), align="bottom")
    with pytest.raises(ca.Error) as e:
        ca.region_fit((0, 70), (48, 40))
    assert e.value.code == ca.E_INVALID_ARG
    assert ca.FIT_ALIGNS == {"center": 0, "top_left": 1}
    assert ca.region_tensor_shape(330, 70, (48, 40), (0, None, (0, 15, 48, 10)), antialias=True) == ((3, 40, 48), 3 * 40 * 48 * 2, (70, 330))
    assert ca.region_tensor_shape(50, 26, (24, 20), (0, (3, 1, 45, 21), None), dtype="f32", downscale=2) == ((3, 20, 24), 3 * 20 * 24 * 4, (10, 22))
    assert ca.region_tensor_shape(50, 26, (24, 20)) == ((3, 20, 24), 2880, (26, 50))
    assert ca.region_tensor_shape(50, 26, (24, 20), Region(0, 0, Rect(0, 0, 0, 0), Rect(1, 1, 2, 2)), dtype="u8")[1] == 1440
    with pytest.raises(ca.Error) as e:
        ca.region_tensor_shape(330, 70, (48, 40), (0, None, (0, 0, 5, 40)), antialias=True)
    assert e.value.code == ca.E_INVALID_ARG and "antialias" in str(e.value)
    for name in ("Region", "region_fit", "region_tensor_shape", "FIT_ALIGNS"):
        assert name in ca.__all__
    assert ca.RESIZE_FILTERS == {"nearest": 0, "bilinear": 1}
    for fn in (ca.Decoder.pack_tensor_regions, ca.Batch.pack_tensor_regions):
        names = list(inspect.signature(fn).parameters)
        assert names == ["self", "dst", "size", "regions", "pad", "filter", "dtype", "downscale", "scale", "bias", "order", "hip_stream", "antialias"]
        p = inspect.signature(fn).parameters
        assert p["pad"].default == (0, 0, 0) and p["antialias"].default is False and p["hip_stream"].default == 0


# ---- the reference itself ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", gr.FILTERS)
@pytest.mark.parametrize("dtype", gr.DTYPES)
def test_reference_with_dst_whole_is_the_resized_reference(filter, dtype):
    rgba = gr.frame(50, 26)[1]
    scale, bias = gr.params(dtype)
    for k, size, src, order in ((1, (24, 20), None, "rgb"), (2, (7, 3), (3, 1, 45, 21), "bgr")):
        want = gr.inner(rgba, size, k, dtype, scale, bias, order, filter, src)
        for dst in (None, (0, 0) + size):
            got = gr.expected(rgba, size, k, dtype, scale, bias, order, filter, src, dst, pad=(1, 2, 3))
            assert got.dtype == want.dtype and got.shape == want.shape and gr.same(got, want, dtype)


def test_reference_places_the_inner_rectangle_and_pads_by_source_channel():
    rgba = gr.frame(50, 26)[1]
    scale, bias, pad = (2.0, 3.0, 4.0), (0.5, 0.25, 0.125), (10.0, 20.0, 30.0)
    for order, planes in (("rgb", (20.5, 60.25, 120.125)), ("bgr", (60.5, 60.25, 40.125))):
        got = gr.expected(rgba, (12, 9), 1, "f32", scale, bias, order, "bilinear", None, (2, 3, 7, 4), pad)
        inner = gr.inner(rgba, (7, 4), 1, "f32", scale, bias, order, "bilinear")
        assert np.array_equal(got[:, 3:7, 2:9], inner)
        mask = np.ones((9, 12), bool)
        mask[3:7, 2:9] = False
        for c in range(3):
            assert (got[c][mask] == np.float32(planes[c])).all()
    # the u8 ties and clamps, an f16 overflow
    assert gr.pad_values((0.5, 1.5, 2.5), "u8", *gr.IDENTITY).tolist() == [0, 2, 2]
    assert gr.pad_values((-3.0, 300.0, 254.5), "u8", *gr.IDENTITY).tolist() == [0, 255, 254]
    f16 = gr.pad_values((70000.0, -70000.0, 65519.0), "f16", *gr.IDENTITY)
    assert np.isposinf(f16[0]) and np.isneginf(f16[1]) and f16[2] == np.float16(65504)
