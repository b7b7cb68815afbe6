"""The oriented tensor output where no device is needed (include/compeg_hip.h, "Oriented tensor output"):
compeg_oriented_tensor_shape against compeg_filtered_tensor_shape of (dst', T), every rejection with its words,
compeg_orient_rect against tests/orient_reference.py, compeg_image_orientation on synthetic frames with a hand-built
APP1 behind SOI -- against PIL where the segment is well formed -- and that the segment never changes what the parser
returns or says."""
import ctypes as C
import glob
import io
import os

import pytest

import compeg_amd as ca
import orient_reference as orf
from compeg_amd._lib import FilterSpec, OrientedRegion, Rect, Region, TensorSpec, lib
from conftest import ROOT
from tools import synth

U8, F16, BF16, F32 = 0, 1, 2, 3
BOX, TRIANGLE, BICUBIC, LANCZOS3 = 0, 1, 2, 3


def _spec(dtype=F16, order=0, downscale=1, reserved=0):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = (1, 1, 1)
    s.bias[:] = (0, 0, 0)
    return s


def _filter(ow=24, oh=20, kernel=BICUBIC, reserved=0):
    return FilterSpec(ow, oh, kernel, reserved)


def _oriented(o=1, src=(0, 0, 0, 0), dst=(0, 0, 0, 0), image=0, reserved=0, inner_reserved=0):
    return OrientedRegion(Region(image, inner_reserved, Rect(*src), Rect(*dst)), o, reserved)


def _shape(spec, filter, w, h, region=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_oriented_tensor_shape(C.byref(spec), C.byref(filter), w, h, C.byref(region) if region is not None else None, C.byref(pw),
                                          C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def _filtered_shape(spec, filter, w, h, region):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_filtered_tensor_shape(C.byref(spec), C.byref(filter), w, h, C.byref(region), C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_struct_sizes():
    assert C.sizeof(OrientedRegion) == 48 and C.sizeof(ca.OrientedRegion) == 48 and C.sizeof(Region) == 40
    assert OrientedRegion.orientation.offset == 40 and OrientedRegion.reserved.offset == 44


@pytest.mark.parametrize("o", orf.ORIENTATIONS)
def test_the_shape_is_the_filtered_shape_of_the_turned_rectangle_in_t(o):
    """... accepted or rejected alike, for regions on both sides of the tap limit."""
    for (w, h), src, dst, kernel, k in (((330, 70), (101, 3, 64, 60), (2, 4, 20, 6), BICUBIC, 1), ((330, 70), (101, 3, 200, 64), (2, 4, 20, 6), BICUBIC, 1),
                                        ((330, 70), (101, 3, 200, 64), (2, 4, 20, 6), BICUBIC, 2), ((50, 26), (3, 1, 45, 21), (1, 3, 11, 13), LANCZOS3, 1),
                                        ((66, 26), (2, 0, 20, 16), (23, 19, 1, 1), BOX, 1), ((16, 8), (0, 0, 16, 8), (0, 0, 24, 20), TRIANGLE, 4)):
        tw, th = orf.slot_extent((24, 20), o)
        turned = Region(0, 0, Rect(*src), Rect(*orf.preimage(dst, o, (24, 20))))
        want = _filtered_shape(_spec(F32, downscale=k), _filter(tw, th, kernel), w, h, turned)
        got = _shape(_spec(F32, downscale=k), _filter(24, 20, kernel), w, h, _oriented(o, src, dst))
        assert got == want, (o, src, dst)
        if want[0] == 0:
            assert got[3] == 3 * 20 * 24 * 4
    # the all-zero rectangles are the whole image into the whole upright slot; no region at all is that at orientation 1
    assert _shape(_spec(U8), _filter(13, 31), 330, 70, _oriented(o)) == (0, 330, 70, 3 * 31 * 13)
    assert _shape(_spec(U8), _filter(13, 31), 330, 70) == (0, 330, 70, 3 * 31 * 13)
    # the image's own tag: there is no image here, 0 counts as 1
    assert _shape(_spec(), _filter(), 330, 70, _oriented(0, (101, 3, 200, 64), (2, 4, 20, 6)))[0] == 0


def test_the_tap_limit_is_taken_against_ts_axes():
    # 200 samples into 20 outputs at orientation 1; into 6 at orientation 6: 200 * 4 > 128 * 6
    assert _shape(_spec(), _filter(), 330, 70, _oriented(1, (101, 3, 200, 64), (2, 4, 20, 6)))[0] == 0
    for o in (5, 6, 7, 8):
        rc = _shape(_spec(), _filter(), 330, 70, _oriented(o, (101, 3, 200, 64), (2, 4, 20, 6)))
        message = lib.compeg_last_error().decode()
        assert rc == (ca.E_INVALID_ARG, 0xdead, 0xdead, 0xdead)
        assert all(w in message for w in ("bicubic", "200x64", "6x20", f"orientation {o} transposes", "downscale")), message
    # ... and the other way round: 64 rows into 6 at orientation 1 is within, 120 columns into 6 at orientation 6 too
    assert _shape(_spec(), _filter(), 330, 70, _oriented(6, (101, 3, 120, 64), (2, 4, 20, 6)))[0] == 0
    message_free = _shape(_spec(), _filter(), 330, 70, _oriented(2, (101, 3, 200, 64), (2, 4, 4, 6)))
    assert message_free[0] == ca.E_INVALID_ARG and "transposes" not in lib.compeg_last_error().decode()


@pytest.mark.parametrize("region, words", [
    (_oriented(9), ("orientation 9", "1 .. 8")),
    (_oriented(0xffffffff), ("orientation 4294967295",)),
    (_oriented(6, reserved=1), ("reserved must be 0",)),
    (_oriented(1, inner_reserved=1), ("reserved must be 0",)),
    (_oriented(6, dst=(0, 0, 5, 0)), ("dst 5x0", "side of 0")),
    (_oriented(6, dst=(5, 0, 20, 20)), ("dst 20x20 at (5, 0)", "leaves", "24x20 output")),
    (_oriented(5, dst=(0, 0, 20, 24)), ("dst 20x24", "leaves", "24x20 output")),   # (it would fit T: the slot is upright)
    (_oriented(3, dst=(0, 0xffffffff, 5, 3)), ("dst", "leaves")),
    (_oriented(7, src=(1, 0, 330, 70)), ("crop 330x70", "leaves", "330x70 image")),
    (_oriented(8, src=(3, 3, 0, 5)), ("crop", "side of 0")),
], ids=lambda v: None)
def test_rejections_carry_a_message(region, words):
    rc, pw, ph, n = _shape(_spec(), _filter(), 330, 70, region)
    assert rc == ca.E_INVALID_ARG and (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message


def test_what_the_filtered_shape_rejects_of_the_specs_is_rejected_here():
    for spec, filter, words in ((_spec(dtype=4), _filter(), ("dtype 4",)), (_spec(downscale=3), _filter(), ("downscale 3",)),
                                (_spec(), _filter(kernel=4), ("kernel 4",)), (_spec(), _filter(reserved=1), ("filter", "reserved")),
                                (_spec(), _filter(ow=0), ("output size 0x20",)), (_spec(downscale=8), _filter(), ("downscale factor 8",))):
        rc = _shape(spec, filter, 7, 5, _oriented(6))
        message = lib.compeg_last_error().decode()
        assert rc[0] == ca.E_INVALID_ARG and all(w in message for w in words), message


@pytest.mark.parametrize("call", ("compeg_decoder_pack_tensor_oriented", "compeg_batch_pack_tensor_oriented"))
def test_the_pack_calls_check_their_arguments_before_their_object(call):
    fn = getattr(lib, call)
    one = (OrientedRegion * 1)(_oriented(6))
    pad = (C.c_float * 3)(0, 0, 0)

    def said(spec, filter, regions, count, pad_):
        rc = fn(None, C.byref(spec), C.byref(filter) if filter is not None else None, regions, count, pad_, None, 0, None)
        assert rc == ca.E_INVALID_ARG
        return lib.compeg_last_error().decode()
    assert "kernel 9" in said(_spec(), _filter(kernel=9), one, 1, pad)
    assert "dtype 5" in said(_spec(dtype=5), _filter(), one, 1, pad)
    assert "filter is NULL" in said(_spec(), None, one, 1, pad)
    assert "regions is NULL" in said(_spec(), _filter(), None, 1, pad)
    assert "region count of 0" in said(_spec(), _filter(), one, 0, pad)
    message = said(_spec(), _filter(), one, 1, (C.c_float * 3)(0, float("nan"), 0))
    assert "pad" in message and "channel 1" in message
    assert "NULL" in said(_spec(), _filter(), one, 1, pad)   # (the object, at last)


RECTS = ((2, 4, 20, 6), (23, 19, 1, 1), (0, 0, 24, 20), (7, 0, 9, 20), (0, 5, 3, 2), (21, 5, 3, 2), (5, 0, 2, 3), (5, 17, 2, 3))


@pytest.mark.parametrize("o", orf.ORIENTATIONS)
def test_orient_rect_is_the_references_preimage(o):
    for rect in RECTS:   # (one that touches each edge among them)
        stored = Rect()
        assert lib.compeg_orient_rect(24, 20, o, C.byref(Rect(*rect)), C.byref(stored)) == 0
        assert (stored.x, stored.y, stored.width, stored.height) == orf.preimage(rect, o, (24, 20))
        assert ca.orient_rect((24, 20), o, rect) == orf.preimage(rect, o, (24, 20))
    # 64-bit integers: the largest extents do not wrap
    big = ca.orient_rect((0xffffffff, 0xfffffffe), o, (0xfffffff0, 7, 15, 0xfffffff0))
    assert big == orf.preimage((0xfffffff0, 7, 15, 0xfffffff0), o, (0xffffffff, 0xfffffffe))


def test_orient_rect_rejections():
    stored = Rect(1, 2, 3, 4)
    for args, words in (((24, 20, 0, Rect(0, 0, 1, 1)), ("orientation 0",)), ((24, 20, 9, Rect(0, 0, 1, 1)), ("orientation 9",)),
                        ((24, 20, 6, Rect(5, 0, 20, 20)), ("20x20 at (5, 0)", "leaves", "24x20")),
                        ((24, 20, 6, Rect(0xffffffff, 0, 2, 2)), ("leaves",)), ((24, 20, 2, Rect(0, 19, 1, 2)), ("leaves",))):
        assert lib.compeg_orient_rect(*args[:3], C.byref(args[3]), C.byref(stored)) == ca.E_INVALID_ARG
        message = lib.compeg_last_error().decode()
        assert all(w in message for w in words), message
        assert (stored.x, stored.y, stored.width, stored.height) == (1, 2, 3, 4)
    assert lib.compeg_orient_rect(24, 20, 1, None, C.byref(stored)) == ca.E_INVALID_ARG
    assert lib.compeg_orient_rect(24, 20, 1, C.byref(Rect(0, 0, 1, 1)), None) == ca.E_INVALID_ARG


# ---- the tag ------------------------------------------------------------------------------------------------------------

FRAME = synth.make_jpeg(48, 32, seed=11)


def _parse(jpeg):
    """(return code, message or None, orientation or None)"""
    h = C.c_void_p()
    raw = bytes(jpeg)
    rc = lib.compeg_image_parse(raw, len(raw), 1, C.byref(h))
    if rc != 0:
        return rc, lib.compeg_last_error().decode(), None
    o = lib.compeg_image_orientation(h)
    lib.compeg_image_free(h)
    return rc, None, o


def _pil_orientation(jpeg):
    from PIL import Image
    return Image.open(io.BytesIO(jpeg)).getexif().get(0x0112, 1)


def test_a_frame_without_the_segment_has_orientation_1():
    assert _parse(FRAME) == (0, None, 1)
    assert ca.ImageData(FRAME).orientation == 1
    assert lib.compeg_image_orientation(None) == 1


@pytest.mark.parametrize("little", (True, False), ids=("II", "MM"))
@pytest.mark.parametrize("where", ("only", "first", "last"))
def test_the_tag_in_both_byte_orders_wherever_it_stands_in_ifd0(little, where):
    pytest.importorskip("PIL")
    for o in orf.ORIENTATIONS:
        jpeg = orf.splice(FRAME, orf.exif_app1(o, little, where))
        assert _parse(jpeg) == (0, None, o)
        assert _pil_orientation(jpeg) == o
        assert ca.ImageData(jpeg).orientation == o


@pytest.mark.parametrize("little", (True, False), ids=("II", "MM"))
def test_what_is_not_a_usable_tag_gives_1(little):
    for segment in (orf.exif_app1(6, little, "absent"), orf.exif_app1(6, little, kind=4), orf.exif_app1(6, little, count=2),
                    orf.exif_app1(0, little), orf.exif_app1(9, little), orf.exif_app1(0x0600, little), orf.exif_app1(6, little, tag=0x0113)):
        assert _parse(orf.splice(FRAME, segment)) == (0, None, 1)
    # the absent tag is PIL's 1 too
    pytest.importorskip("PIL")
    assert _pil_orientation(orf.splice(FRAME, orf.exif_app1(6, little, "absent"))) == 1


def test_only_the_first_exif_segment_in_front_of_the_scan_counts():
    first, second = orf.exif_app1(6), orf.exif_app1(3, little=False)
    assert _parse(orf.splice(FRAME, first + second))[2] == 6
    assert _parse(orf.splice(FRAME, second + first))[2] == 3
    # a first one without the tag is still the first; an APP1 that is not "Exif" (XMP) is none
    assert _parse(orf.splice(FRAME, orf.exif_app1(6, where="absent") + second))[2] == 1
    xmp = b"\xff\xe1" + (2 + 29 + 4).to_bytes(2, "big") + b"http://ns.adobe.com/xap/1.0/\0" + b"<x/>"
    assert _parse(orf.splice(FRAME, xmp + first))[2] == 6
    # behind the scan's data it is not in front of SOS
    assert FRAME[-2:] == b"\xff\xd9"
    assert _parse(FRAME[:-2] + first + FRAME[-2:])[:2] == _parse(FRAME)[:2]
    assert _parse(FRAME[:-2] + first + FRAME[-2:])[2] == 1


def test_the_segment_cut_at_every_length_gives_1():
    """The APP1's own length says less than the IFD needs, at every length down to none: whatever reads beyond it is a bug."""
    whole = orf.exif_app1(6, where="last")
    payload = whole[4:]
    at = payload.index(b"\x12\x01") + 12   # the end of the orientation's 12-byte entry in the payload
    assert _parse(orf.splice(FRAME, whole))[2] == 6
    for n in range(len(payload)):
        cut = b"\xff\xe1" + (n + 2).to_bytes(2, "big") + payload[:n]
        want = 6 if n >= at else 1
        assert _parse(orf.splice(FRAME, cut)) == (0, None, want), n


def test_an_offset_outside_the_segment_gives_1():
    for little in (True, False):
        whole = bytearray(orf.exif_app1(6, little))
        for offset in (len(whole), 0xffffffff, 0xfffffff8, len(whole) - 4 - 6 - 1):
            whole[4 + 6 + 4:4 + 6 + 8] = offset.to_bytes(4, "little" if little else "big")
            assert _parse(orf.splice(FRAME, bytes(whole))) == (0, None, 1), offset
        for header in (b"II*\1", b"MM*\0", b"IM\0*", b"\0\0\0\0"):
            whole[4 + 6:4 + 6 + 4] = header
            assert _parse(orf.splice(FRAME, bytes(whole)))[2] == 1


def test_golden_files_without_exif_have_orientation_1():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "parser", "*.jpg")))
    assert files
    seen = 0
    for path in files:
        raw = open(path, "rb").read()
        if b"Exif\0\0" in raw:
            continue
        rc, _, o = _parse(raw)
        if rc == 0:
            seen += 1
            assert o == 1, path
    assert seen > 0


def test_the_segment_never_changes_what_the_parser_returns_or_says():
    """Every spliced file of this module, and the golden parser files with a segment spliced in, parse to the same return
    code and message as without it."""
    segments = [orf.exif_app1(o, little, where) for o in (1, 6, 9) for little in (True, False) for where in ("only", "first", "last", "absent")]
    segments += [orf.exif_app1(6, kind=4), orf.exif_app1(6, count=2), b"\xff\xe1\x00\x02", b"\xff\xe1\x00\x08Exif\0\0", b"\xff\xe1\x00\x0aExif\0\0II"]
    frames = [FRAME, synth.make_jpeg(17, 9, seed=2), FRAME[:len(FRAME) // 2], FRAME[:200]]
    frames += [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "parser", "*.jpg")))]
    for frame in frames:
        if frame[:2] != b"\xff\xd8":
            continue
        want = _parse(frame)[:2]
        for segment in segments:
            assert _parse(orf.splice(frame, segment))[:2] == want


def test_python_mirror():
    assert ca.ORIENTATIONS == {"normal": 1, "mirror": 2, "rotate180": 3, "flip": 4, "transpose": 5, "rotate90": 6, "transverse": 7, "rotate270": 8}
    for name in ("ORIENTATIONS", "OrientedRegion", "orient_rect", "oriented_tensor_shape"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert ca.oriented_tensor_shape(330, 70, (24, 20), (0, (101, 3, 120, 64), (2, 4, 20, 6), "rotate90")) == ((3, 20, 24), 2880, (64, 120))
    assert ca.oriented_tensor_shape(330, 70, (24, 20), (0, (101, 3, 120, 64), (2, 4, 20, 6)), orientation=6)[2] == (64, 120)
    assert ca.oriented_tensor_shape(330, 70, (13, 31), orientation="exif", dtype="u8")[1] == 3 * 31 * 13
    with pytest.raises(ca.Error) as e:
        ca.oriented_tensor_shape(330, 70, (24, 20), (0, (101, 3, 200, 64), (2, 4, 20, 6)), orientation="rotate270")
    assert e.value.code == ca.E_INVALID_ARG and "orientation 8 transposes" in str(e.value)
    with pytest.raises(ca.Error) as e:
        ca.oriented_tensor_shape(330, 70, (24, 20), orientation="upright")
    assert "unknown orientation" in str(e.value) and "rotate90" in str(e.value)
    with pytest.raises(ca.Error) as e:
        ca.orient_rect((24, 20), 9, (0, 0, 1, 1))
    assert "orientation 9" in str(e.value)
    assert ca.orient_rect((70, 330), "rotate90", (0, 0, 70, 330)) == (0, 0, 330, 70)
    import inspect
    for fn in (ca.Decoder.pack_tensor_oriented, ca.Batch.pack_tensor_oriented):
        p = inspect.signature(fn).parameters
        assert list(p)[:5] == ["self", "dst", "size", "regions", "orientation"] and p["regions"].default is None
        assert p["orientation"].default == "exif" and p["kernel"].default == "bicubic" and p["hip_stream"].default == 0
