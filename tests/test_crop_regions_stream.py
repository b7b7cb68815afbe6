"""The cropped decode of a region list where no device is needed (include/compeg_hip.h, "Cropped decode of a region list").

compeg_crop_regions_shape and compeg_crop_region_check against their restatements (tests/crop_regions_stream.py), every
refusal that needs no decoder or batch by what its message says, the struct sizes, the Python argument forms, __all__, and
the expectation module pinned to tests/crop_stream.py's: a one-region list whose slot is its rectangle is the one-rectangle
decode's destination, and a region laid into a larger slot is that rectangle moved, the rest of the slot untouched.  The
mixed batch the other files share is checked here too.  (What needs a decoder or a batch needs a device:
tests/test_gpu_crop_regions.py.)"""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import crop_regions_stream as rgs
import crop_stream as crs
import planes_stream as ps
from compeg_amd._lib import CropRegion, CropRegionsSpec, lib


def _spec(slot, format=0, pitch=0, reserved=(0, 0, 0, 0)):
    s = CropRegionsSpec()
    s.slot_width, s.slot_height = slot
    s.format, s.pitch = format, pitch
    for i, v in enumerate(reserved):
        s.reserved[i] = v
    return s


def _region(image, rect, place=(0, 0), reserved=0):
    r = CropRegion()
    r.image = image
    r.x, r.y, r.width, r.height = rect
    r.dst_x, r.dst_y = place
    r.reserved = reserved
    return r


def test_struct_sizes_and_names():
    assert C.sizeof(CropRegion) == 32 and C.sizeof(CropRegionsSpec) == 32
    for name in ("CropRegion", "CropRegionsSpec", "crop_regions_shape"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert hasattr(ca.Decoder, "decode_cropped_regions") and hasattr(ca.Batch, "decode_cropped_regions")
    # no new kernel id: the name tuples are what they were
    assert ca.LAST_KERNEL_NAMES[11] == "cropped" and len(ca.LAST_KERNEL_NAMES) == 14 and len(ca.ALL_KERNEL_NAMES) == 12


def test_shape_against_the_restatement():
    for slot in ((1, 1), (8, 8), (17, 9), (224, 224), (325, 71), (65535, 1), (1, 65535), (65535, 65535)):
        for format in rgs.FORMATS:
            assert ca.crop_regions_shape(slot, format) == rgs.shape(slot, format), (slot, format)
        for extra in (0, 4, 64):
            pitch = 4 * slot[0] + extra
            assert ca.crop_regions_shape(slot, "rgba", pitch) == rgs.shape(slot, "rgba", pitch), (slot, pitch)
    assert ca.crop_regions_shape((224, 224)) == (896, 200704)
    assert ca.crop_regions_shape((224, 224), "rgb_planar") == (224, 150528)
    # (either output may be NULL)
    assert lib.compeg_crop_regions_shape(C.byref(_spec((3, 4))), None, None) == 0


def _shape_refused(spec, *words):
    pt, total = C.c_uint32(0xdddddddd), C.c_uint64(0xdddddddddddddddd)
    rc = lib.compeg_crop_regions_shape(C.byref(spec) if spec is not None else None, C.byref(pt), C.byref(total))
    text = lib.compeg_last_error().decode()
    assert rc == ca.E_INVALID_ARG and all(x in text for x in words) and "COMPEG_" not in text, (rc, text)
    assert (pt.value, total.value) == (0xdddddddd, 0xdddddddddddddddd), "an output was written on failure"


def _region_refused(spec, w, h, region, *words):
    rc = lib.compeg_crop_region_check(C.byref(spec) if spec is not None else None, w, h, C.byref(region) if region is not None else None)
    text = lib.compeg_last_error().decode()
    assert rc == ca.E_INVALID_ARG and all(x in text for x in words) and "COMPEG_" not in text, (rc, text)


def test_spec_refusals_that_need_no_device():
    _shape_refused(None, "spec is NULL")
    _shape_refused(_spec((8, 8), format=2), "format 2")
    _shape_refused(_spec((8, 8), reserved=(0, 0, 7, 0)), "reserved[2]", "is 7", "must be 0")
    _shape_refused(_spec((8, 8), reserved=(1, 0, 0, 0)), "reserved[0]", "is 1")
    _shape_refused(_spec((0, 8)), "0x8", "no pixels")
    _shape_refused(_spec((8, 0)), "8x0", "no pixels")
    _shape_refused(_spec((65536, 8)), "65536x8", "65535")
    _shape_refused(_spec((41, 9), pitch=160), "pitch 160", "164")   # (below 4 slot_width)
    _shape_refused(_spec((41, 9), pitch=166), "pitch 166", "multiple of 4")
    _shape_refused(_spec((8, 8), format=1, pitch=8), "pitch 8", "planar")
    with pytest.raises(ca.Error, match="unknown crop format"):
        ca.crop_regions_shape((8, 8), "bgr")
    with pytest.raises(ca.Error, match="pitch 166"):
        ca.crop_regions_shape((41, 9), pitch=166)


def test_region_check_against_the_restatement():
    slot = (20, 12)
    spec = _spec(slot)
    n = {True: 0, False: 0}
    for w, h in ((16, 16), (33, 9), (1, 1)):
        for rect in ((0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (3, 2, 8, 5), (w, 0, 1, 1), (0, 0, 0, 1), (0, 0, 21, 1), (2, 2, 14, 11)):
            for place in ((0, 0), (1, 1), (19, 11), (slot[0] - rect[2], slot[1] - rect[3]), (20, 0)):
                if min(place) < 0:
                    continue
                want = rgs.fits(slot, w, h, (0, rect, place))
                rc = lib.compeg_crop_region_check(C.byref(spec), w, h, C.byref(_region(0, rect, place)))
                assert (rc == 0) == want, (w, h, rect, place, rc, lib.compeg_last_error().decode())
                n[want] += 1
    assert n[True] > 10 and n[False] > 10


def test_region_refusals_that_need_no_device():
    spec = _spec((20, 12))
    _region_refused(None, 16, 16, _region(0, (0, 0, 8, 8)), "spec is NULL")
    _region_refused(spec, 16, 16, None, "region is NULL")
    _region_refused(_spec((20, 12), format=3), 16, 16, _region(0, (0, 0, 8, 8)), "format 3")
    _region_refused(spec, 0, 16, _region(0, (0, 0, 8, 8)), "no pixels")
    _region_refused(spec, 16, 16, _region(0, (0, 0, 8, 8), reserved=5), "reserved is 5", "must be 0")
    _region_refused(spec, 16, 16, _region(0, (3, 4, 0, 8)), "0x8 at (3, 4)", "empty")
    _region_refused(spec, 16, 16, _region(0, (3, 4, 8, 0)), "8x0 at (3, 4)", "empty")
    _region_refused(spec, 16, 16, _region(2, (9, 0, 8, 8)), "8x8 at (9, 0)", "beyond image 2's 16x16")
    _region_refused(spec, 16, 16, _region(0, (0, 9, 8, 8)), "8x8 at (0, 9)", "beyond", "16x16")
    _region_refused(spec, 16, 16, _region(0, (0xffffffff, 0, 2, 1)), "beyond")   # (x + width wraps in 32 bits)
    _region_refused(spec, 16, 16, _region(0, (0, 0, 8, 8), (13, 0)), "8x8 at (0, 0)", "placed at (13, 0)", "slot's 20x12")
    _region_refused(spec, 16, 16, _region(0, (0, 0, 8, 8), (0, 5)), "placed at (0, 5)", "20x12")
    _region_refused(spec, 16, 16, _region(0, (0, 0, 2, 1), (0xffffffff, 0)), "slot")   # (dst_x + width wraps in 32 bits)
    assert lib.compeg_crop_region_check(C.byref(spec), 16, 16, C.byref(_region(9, (8, 8, 8, 8), (12, 4)))) == 0   # (image is not looked at)


def test_entry_points_refuse_null_owners():
    spec, region = _spec((8, 8)), _region(0, (0, 0, 8, 8))
    for rc in (lib.compeg_batch_decode_cropped_regions(None, C.byref(spec), C.byref(region), 1, C.c_void_p(16), 256, None),
               lib.compeg_decoder_decode_cropped_regions(None, None, C.byref(spec), C.byref(region), 1, C.c_void_p(16), 256, None),
               lib.compeg_decoder_decode_cropped_regions_blocking(None, None, C.byref(spec), C.byref(region), 1, C.c_void_p(16), 256)):
        assert rc == ca.E_INVALID_ARG and "NULL" in lib.compeg_last_error().decode()


def test_python_argument_forms():
    spec, array, count = ca._crop_regions_args([(2, (3, 4, 5, 6)), (0, (1, 2, 3, 4), (7, 8)), _region(1, (0, 0, 9, 2), (1, 0))], None, "rgb_planar", None)
    assert count == 3 and (spec.slot_width, spec.slot_height, spec.format, spec.pitch) == (10, 12, 1, 0)
    got = [(r.image, (r.x, r.y, r.width, r.height), (r.dst_x, r.dst_y), r.reserved) for r in array]
    assert got == [(2, (3, 4, 5, 6), (0, 0), 0), (0, (1, 2, 3, 4), (7, 8), 0), (1, (0, 0, 9, 2), (1, 0), 0)]
    assert rgs.slot_of([(2, (3, 4, 5, 6)), (0, (1, 2, 3, 4), (7, 8)), (1, (0, 0, 9, 2), (1, 0))]) == (10, 12)
    spec, array, count = ca._crop_regions_args([(0, (0, 0, 2, 2))], (30, 20), "rgba", 128)
    assert count == 1 and (spec.slot_width, spec.slot_height, spec.format, spec.pitch) == (30, 20, 0, 128)
    assert ca._crop_regions_args([], None, "rgba", None)[2] == 0
    for bad in ((0,), (0, (1, 2, 3)), (0, (1, 2, 3, 4), (1,)), "region", 7):
        with pytest.raises(ca.Error, match="crop regions"):
            ca._crop_regions_args([bad], None, "rgba", None)
    with pytest.raises(ca.Error, match="unknown crop format"):
        ca._crop_regions_args([(0, (0, 0, 2, 2))], None, "bgr", None)


# ---- the expectation module ------------------------------------------------------------------------------------------

def test_one_region_whose_slot_is_its_rectangle_is_the_one_rectangle_destination():
    f = ps.sized("420", 324, 70, 5, seed=4)
    full = crs.frame_rgba(f)
    for n, rect in enumerate(crs.RECTS):
        for format in rgs.FORMATS:
            pitch = 4 * rect[2] + 8 * (n % 3) if format == "rgba" else None
            assert rgs.shape(rect[2:], format, pitch) == crs.shape(324, 70, rect, format, pitch)
            before = np.full(crs.shape(324, 70, rect, format, pitch)[1], 0xA5, dtype=np.uint8)
            want = crs.destination(full[0], full[1], rect, format, pitch, before=before)
            assert np.array_equal(rgs.destination([full], [(0, rect)], rect[2:], format, pitch, before=before), want), (rect, format)


def test_a_region_in_a_larger_slot_is_the_rectangle_moved():
    f = ps.sized("422", 48, 23, 4, seed=2, short=3)
    full = crs.frame_rgba(f, ca=ca)
    rect, slot = (30, 14, 18, 9), (25, 12)
    m = full[1][14:23, 30:48]
    assert m.any() and not m.all()
    for place in ((0, 0), (1, 2), (7, 3)):
        for format in rgs.FORMATS:
            pt, slot_bytes = rgs.shape(slot, format, 112 if format == "rgba" else None)
            before = np.full(2 * slot_bytes, 0xA5, dtype=np.uint8)
            out = rgs.destination([full], [(0, (0, 0, 1, 1)), (0, rect, place)], slot, format, 112 if format == "rgba" else None, before=before)
            one = out[slot_bytes:]
            if format == "rgba":
                px = np.stack([one[r * pt:r * pt + 4 * slot[0]].reshape(slot[0], 4) for r in range(slot[1])])
            else:
                px = one.reshape(3, slot[1], slot[0]).transpose(1, 2, 0)
            inside = np.zeros((slot[1], slot[0]), dtype=bool)
            inside[place[1]:place[1] + 9, place[0]:place[0] + 18] = m
            c = 4 if format == "rgba" else 3
            assert np.array_equal(px[place[1]:place[1] + 9, place[0]:place[0] + 18][m], full[0][14:23, 30:48][m][:, :c])
            assert (px[~inside] == 0xA5).all(), "the rest of the slot and the undecoded MCU's pixels keep what was there"
            if format == "rgba":
                assert all((one[r * pt + 4 * slot[0]:(r + 1) * pt] == 0xA5).all() for r in range(slot[1])), "the pitch's padding"
            assert (out[:slot_bytes] != 0xA5).sum() <= c and (out[:slot_bytes] != 0xA5).any(), "slot 0 holds its one pixel"


def test_the_grouping_restated():
    layouts = ["422", "gray", "420", "422", "444"]
    regions = [(1, (0, 0, 1, 1)), (0, (0, 0, 1, 1)), (4, (0, 0, 1, 1)), (3, (0, 0, 1, 1)), (1, (0, 0, 1, 1)), (0, (0, 0, 1, 1)), (3, (0, 0, 1, 1))]
    assert rgs.launches(layouts, regions) == [("422", [1, 3, 5, 6]), ("444", [2]), ("gray", [0, 4])]
    assert rgs.launches(layouts, regions, chunk=3) == [("422", [1, 3, 5]), ("422", [6]), ("444", [2]), ("gray", [0, 4])]
    assert rgs.launches(layouts, regions, chunk=1)[:2] == [("422", [1]), ("422", [3])]
    assert rgs.launches(layouts, []) == []
    many = [(0, (0, 0, 1, 1))] * 70000
    assert [len(ks) for _, ks in rgs.launches(layouts, many)] == [65535, 70000 - 65535]


def test_the_mixed_batch_and_its_region_list():
    frames = rgs.mixed_batch()
    fulls = rgs.mixed_fulls(frames, ca)   # (asserts the masks)
    assert [lay for _, lay in frames[:5]] == list(rgs.GROUPS) and [f.standard for f, _ in frames[:5]] == [False, True, False, True, False]
    assert any(f.interval == 0 or f.intervals == 1 for f, _ in frames[:5]), "one of the five has no DRI"
    regions = rgs.mixed_regions()
    spec = _spec(rgs.SLOT)
    for image, rect, place in regions:
        f = frames[image][0]
        assert rgs.fits(rgs.SLOT, f.w, f.h, (image, rect, place))
        assert lib.compeg_crop_region_check(C.byref(spec), f.w, f.h, C.byref(_region(image, rect, place))) == 0
    places = [p for _, _, p in regions]
    assert (0, 0) in places and any(p[0] == 1 for p in places) and any(p[1] == 1 for p in places)
    assert any(p[0] + r[2] == rgs.SLOT[0] for _, r, p in regions) and any(p[1] + r[3] == rgs.SLOT[1] for _, r, p in regions)
    images = [r[0] for r in regions]
    lays = [frames[i][1] for i in images]
    assert images != sorted(images) and lays != sorted(lays, key=rgs.GROUPS.index), "neither images nor samplings come in order"
    # the region inside the undecoded MCU writes nothing; every other region writes something
    before = np.full(len(regions) * rgs.shape(rgs.SLOT)[1], 0xA5, dtype=np.uint8)
    out = rgs.destination(fulls, regions, rgs.SLOT, before=before).reshape(len(regions), -1)
    untouched = [k for k in range(len(regions)) if (out[k] == 0xA5).all()]
    assert untouched == [k for k, r in enumerate(regions) if r[0] == rgs.SHORT and r[1] == (33, 17, 14, 5)] and len(untouched) == 1
    groups = rgs.launches([lay for _, lay in frames], regions)
    assert [g for g, _ in groups] == list(rgs.GROUPS) and sorted(k for _, ks in groups for k in ks) == list(range(len(regions)))
