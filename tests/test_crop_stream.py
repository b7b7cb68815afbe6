"""The cropped decode where no device is needed (include/compeg_hip.h, "Cropped decode").

The expectation itself (tests/crop_stream.py) is pinned to the oracle: for the sized frames the card's tests are made of and
for the golden files, the destination it gives for a rectangle is the slice of orc.ImageData(...).decode() -- the crop of the
full decode, which is the definition.  Grayscale, which the oracle's colour step does not take, is pinned to
gs.expectation.  Then compeg_crop_shape against its restatement, the refusals that need no decoder or batch, the
full-frame rectangle, a C99 consumer of the new declarations, and the kernel's name.  (What needs a decoder or a batch needs
a device: tests/test_gpu_crop.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compeg_amd as ca
import crop_stream as crs
import gray_stream as gs
import planes_stream as ps
from compeg_amd._lib import CropSpec, lib
from conftest import GOLDEN, ROOT
from oracle import oracle as orc


def _slices_equal(rgba, mask, want, what, rects):
    h, w = mask.shape
    for n, rect in enumerate(rects):
        x, y, rw, rh = rect
        for format in crs.FORMATS:
            pitch = 4 * rw + 8 * (n % 3) if format == "rgba" else None
            pt, total = crs.shape(w, h, rect, format, pitch)
            got = crs.view(crs.destination(rgba, mask, rect, format, pitch), rect, format, pitch)
            assert np.array_equal(got, want[y:y + rh, x:x + rw]), f"{what}: {rect}, {format}"
            if format == "rgba" and pt > 4 * rw:   # the padding of a pitch keeps what was there
                raw = crs.destination(rgba, mask, rect, format, pitch, before=np.full(total, 0xA5, dtype=np.uint8))
                assert all((raw[r * pt + 4 * rw:(r + 1) * pt] == 0xA5).all() for r in range(rh))


@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_expectation_is_the_slice_of_the_oracles_decode(layout):
    w, h = crs.SIZE
    for i, ri in enumerate(crs.DRIS[layout]):
        f = ps.sized(layout, w, h, ri, standard=i % 2 == 1, seed=3 + i)
        rgba, mask = crs.frame_rgba(f)
        assert mask.all() and rgba.shape == (h, w, 4)
        want = gs.expectation(f) if layout == "gray" else orc.ImageData(f.jpeg(), **f.image_kw()).decode()
        assert np.array_equal(rgba, want), f"{f.name}: the full frame"
        _slices_equal(rgba, mask, want, f.name, crs.RECTS)


def test_expectation_of_a_frame_with_an_undecoded_tail():
    f = ps.sized("422", 48, 23, 4, seed=2, short=3)
    rgba, mask = crs.frame_rgba(f, ca=ca)
    want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    assert not mask.all() and (rgba[~mask] == 0).all()
    assert np.array_equal(rgba[mask], want[mask])
    rect = (30, 14, 18, 9)   # partly over the MCU no interval covers
    before = np.full(crs.shape(48, 23, rect)[1], 0xA5, dtype=np.uint8)
    got = crs.view(crs.destination(rgba, mask, rect, before=before), rect)
    m = mask[14:23, 30:48]
    assert np.array_equal(got[m], want[14:23, 30:48][m]) and (got[~m] == 0xA5).all() and (~m).any() and m.any()


def test_expectation_of_the_golden_files_is_the_slice_of_the_oracles_decode():
    files = ps.golden_files(ca, GOLDEN)
    samplings = set()
    for name, j, kw in files:
        rgba, mask, (w, h, comps, hs, vs) = crs.file_rgba(ca, j, **kw)
        samplings.add((comps, hs, vs))
        if comps == 1:
            continue   # (the oracle's colour step takes three components; the card's own RGBA is compared in tests/test_gpu_crop.py)
        want = orc.ImageData(j, **{k: v for k, v in kw.items() if k != "allow_grayscale"}).decode()
        assert np.array_equal(rgba[mask], want[mask]), name
        rects = [(0, 0, w, h), (w // 3, h // 4, max(1, w // 2), max(1, h // 3)), (w - 1, h - 1, 1, 1)]
        if mask.all():
            _slices_equal(rgba, mask, want, name, rects)
    assert {(3, 2, 1), (3, 1, 1)} <= samplings, samplings


def test_full_frame_rectangle_is_the_tight_rgba():
    f = ps.sized("420", 324, 70, 5, seed=4)
    rgba, mask = crs.frame_rgba(f)
    assert np.array_equal(crs.destination(rgba, mask, (0, 0, 324, 70)), rgba.ravel())
    planar = crs.destination(rgba, mask, (0, 0, 324, 70), "rgb_planar")
    assert np.array_equal(planar.reshape(3, 70, 324), rgba[..., :3].transpose(2, 0, 1))
    assert ca.crop_shape(324, 70, (0, 0, 324, 70)) == (4 * 324, 4 * 324 * 70)


# ---- the shape call --------------------------------------------------------------------------------------------------

def _spec(rect, format=0, pitch=0, reserved=(0, 0)):
    s = CropSpec()
    s.x, s.y, s.width, s.height = rect
    s.format, s.pitch = format, pitch
    s.reserved[0], s.reserved[1] = reserved
    return s


def _shape(spec, w, h):
    pt, total = C.c_uint32(0xdddddddd), C.c_uint64(0xdddddddddddddddd)
    rc = lib.compeg_crop_shape(C.byref(spec) if spec is not None else None, w, h, C.byref(pt), C.byref(total))
    return rc, (pt.value, total.value)


def test_struct_size_and_names():
    assert C.sizeof(CropSpec) == 32
    assert ca.CROP_FORMATS == {"rgba": 0, "rgb_planar": 1} and crs.FORMATS == tuple(ca.CROP_FORMATS)
    assert ca.ALL_KERNEL_NAMES[11] == "cropped" and ca.ALL_KERNEL_NAMES[10] == "reduced" and ca.ALL_KERNEL_NAMES[:10] == ca.KERNEL_NAMES
    assert len(ca.ALL_KERNEL_NAMES) == 12
    for name in ("CropSpec", "CROP_FORMATS", "crop_shape"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert hasattr(ca.Decoder, "decode_cropped") and hasattr(ca.Batch, "decode_cropped")


def test_shape_against_the_restatement():
    for w, h in ((1, 1), (8, 8), (17, 9), (324, 70), (3840, 2160), (65535, 1), (1, 65535)):
        rects = {(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w // 2, h // 3, w - w // 2, h - h // 3), (w // 4, 0, max(1, w // 3), h)}
        for rect in rects:
            for format in crs.FORMATS:
                assert ca.crop_shape(w, h, rect, format) == crs.shape(w, h, rect, format), (w, h, rect, format)
            for extra in (0, 4, 64):
                pitch = 4 * rect[2] + extra
                assert ca.crop_shape(w, h, rect, "rgba", pitch) == crs.shape(w, h, rect, "rgba", pitch), (w, h, rect, pitch)
    assert ca.crop_shape(3840, 2160, (1808, 968, 224, 224)) == (896, 200704)
    assert ca.crop_shape(3840, 2160, (1808, 968, 224, 224), "rgb_planar") == (224, 150528)
    # (either output may be NULL)
    assert lib.compeg_crop_shape(C.byref(_spec((1, 2, 3, 4))), 17, 9, None, None) == 0


def _refused(spec, w, h, *words):
    rc, out = _shape(spec, w, h)
    text = lib.compeg_last_error().decode()
    assert rc == ca.E_INVALID_ARG and all(x in text for x in words) and "COMPEG_" not in text, (rc, text)
    assert out == (0xdddddddd, 0xdddddddddddddddd), "an output was written on failure"


def test_refusals_that_need_no_device():
    _refused(None, 16, 16, "spec is NULL")
    _refused(_spec((0, 0, 8, 8), format=2), 16, 16, "format 2")
    _refused(_spec((0, 0, 8, 8), reserved=(0, 7)), 16, 16, "reserved", "0, 7", "must be 0")
    _refused(_spec((0, 0, 8, 8), reserved=(1, 0)), 16, 16, "reserved", "1, 0")
    _refused(_spec((0, 0, 8, 8)), 0, 16, "no pixels")
    _refused(_spec((0, 0, 8, 8)), 16, 0, "no pixels")
    _refused(_spec((3, 4, 0, 8)), 16, 16, "0x8 at (3, 4)", "empty")
    _refused(_spec((3, 4, 8, 0)), 16, 16, "8x0 at (3, 4)", "empty")
    _refused(_spec((9, 0, 8, 8)), 16, 16, "8x8 at (9, 0)", "beyond", "16x16")
    _refused(_spec((0, 9, 8, 8)), 16, 16, "8x8 at (0, 9)", "beyond", "16x16")
    _refused(_spec((16, 0, 1, 1)), 16, 16, "1x1 at (16, 0)", "beyond")
    _refused(_spec((0xffffffff, 0, 2, 1)), 16, 16, "beyond")   # (x + width wraps in 32 bits)
    _refused(_spec((0, 0, 0xffffffff, 0xffffffff)), 65535, 65535, "beyond")
    _refused(_spec((0, 0, 41, 9), pitch=160), 324, 70, "pitch 160", "164")   # (below 4 width)
    _refused(_spec((0, 0, 41, 9), pitch=166), 324, 70, "pitch 166", "multiple of 4")
    _refused(_spec((0, 0, 8, 8), format=1, pitch=8), 16, 16, "pitch 8", "planar")
    with pytest.raises(ca.Error, match="unknown crop format"):
        ca.crop_shape(16, 16, (0, 0, 8, 8), "bgr")
    with pytest.raises(ca.Error, match="beyond"):
        ca.crop_shape(16, 16, (8, 8, 9, 8))


def test_a_plain_c_consumer_of_the_new_declarations(tmp_path):
    exe = str(tmp_path / "crop_consumer")
    libdir = os.path.dirname(ca.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_consumer", "crop_consumer.c"), "-o", exe,
                           "-L", libdir, "-l:libcompeg_hip.so", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, "3840", "2160", "1808", "968", "224", "224", "0", "1024"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["shape", "1024", str(1024 * 224)], r.stdout + r.stderr
    r = subprocess.run([exe, "3840", "2160", "3700", "968", "224", "224", "1", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith(f"refused {ca.E_INVALID_ARG}: ") and "224x224 at (3700, 968)" in r.stdout, r.stdout + r.stderr
