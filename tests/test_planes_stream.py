"""The planes decode where no device is needed (include/compeg_hip.h, "Planar YCbCr output").

The expectation itself (tests/planes_stream.py) is pinned to what "bit-exact" already means here: for every frame of the
coefficient families, colour and grayscale, and for every real file of the golden set the front end accepts, the expected
planar planes, put through the integer colour step with nearest-neighbour chroma, equal the oracle's RGBA decode.  Then
compeg_planes_shape against a table written out here and against the restated layout, every refusal the shape call makes
with its words, ImageData.sampling(), and the C99 consumer compiled against the header.  (What needs a batch or a decoder
-- a short destination, batches of two sizes or two samplings -- needs a device: tests/test_gpu_planes.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compeg_amd as ca
import coef_stream as cs
import gray_stream as gs
import planes_stream as ps
from compeg_amd._lib import PlanesLayout, PlanesSpec, lib
from conftest import GOLDEN, ROOT
from oracle import oracle as orc


# ---- the expectation is the oracle's ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f.name for f in cs.cases()] + [f.name for f in gs.cases()])
def test_expected_planes_through_the_colour_step_are_the_oracles_rgba(name):
    gray = "/gray/" in name
    f = gs.case(name) if gray else cs.case(name)
    comps, hs, vs = ps.sampling_of(f)
    y, cb, cr, (my, _) = ps.frame_planes(f)
    got = ps.colour(y, cb, cr, hs, vs, f.w, f.h, my)
    if gray:
        # (the oracle rejects one component: its decode of the 4:4:4 twin where the twin can serve, else the restatement
        # tests/test_gray_stream.py pins)
        want = gs.expectation(f)
    else:
        want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    assert np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"


def test_expected_planes_of_the_golden_files_are_the_oracles_rgba():
    files = ps.golden_files(ca, GOLDEN)
    samplings = set()
    for name, j, kw in files:
        planes, (w, h, comps, hs, vs) = ps.file_planes(ca, j, **kw)
        samplings.add((comps, hs, vs))
        got = ps.colour(planes[0], planes[1], planes[2], hs, vs, w, h, planes[3][0])
        if comps == 1:
            continue   # (no oracle decode of one component; the card's own RGBA is compared in tests/test_gpu_planes.py)
        want = orc.ImageData(j, allow_sampling=True).decode()
        assert np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"
    assert {(3, 2, 1), (3, 1, 1)} <= samplings, samplings


def test_sized_frames_decode_like_the_oracle():
    """The frames the card's tests are made of (ps.sized): odd extents in every sampling, both entropy modes."""
    for layout in ("422", "444", "440", "420"):
        hs, vs = ps.SAMPLINGS[layout]
        for (w, h, ri, std) in ((8 * hs + 1, 8 * vs + 1, 2, False), (24 * hs - 1, 24 * vs - 1, 3, True), (8 * hs, 8 * vs, 0, False)):
            f = ps.sized(layout, w, h, ri, standard=std, seed=3)
            y, cb, cr, (my, _) = ps.frame_planes(f)
            want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
            assert want.shape[:2] == (h, w)
            assert np.array_equal(ps.colour(y, cb, cr, hs, vs, w, h, my), want), f.name


# ---- the shape call --------------------------------------------------------------------------------------------------

def _shape(spec, w, h, comps, hs, vs):
    lay = PlanesLayout()
    C.memset(C.byref(lay), 0xdd, C.sizeof(lay))
    rc = lib.compeg_planes_shape(C.byref(spec) if spec is not None else None, w, h, comps, hs, vs, C.byref(lay))
    return rc, lay


def _spec(format=0, chroma=0, luma_pitch=0, chroma_pitch=0, reserved=(0, 0, 0, 0)):
    return PlanesSpec(format, chroma, luma_pitch, chroma_pitch, (C.c_uint32 * 4)(*reserved))


def test_struct_sizes_and_names():
    assert C.sizeof(PlanesSpec) == 32 and C.sizeof(PlanesLayout) == 88
    assert ca.PLANES_FORMATS == {"planar": 0, "semiplanar": 1, "yuyv": 2, "uyvy": 3} and ca.PLANES_CHROMA == {"coded": 0, "420": 1}
    assert ca.KERNEL_NAMES[9] == "planes" and len(ca.KERNEL_NAMES) == 10


# (w, h, sampling, format, chroma, pitch) -> ([(offset, pitch, row bytes, width, height)], total), written out by hand
TABLE = [
    ((1, 1, "422", "planar", "coded", None), ([(0, 1, 1, 1, 1), (1, 1, 1, 1, 1), (2, 1, 1, 1, 1)], 3)),
    ((1, 1, "422", "yuyv", "coded", None), ([(0, 4, 4, 1, 1)], 4)),
    ((1, 1, "420", "semiplanar", "coded", None), ([(0, 1, 1, 1, 1), (1, 2, 2, 1, 1)], 3)),
    ((1, 1, "gray", "planar", "coded", None), ([(0, 1, 1, 1, 1)], 1)),
    ((17, 9, "422", "planar", "coded", None), ([(0, 17, 17, 17, 9), (153, 9, 9, 9, 9), (234, 9, 9, 9, 9)], 315)),
    ((17, 9, "422", "semiplanar", "coded", None), ([(0, 17, 17, 17, 9), (153, 18, 18, 9, 9)], 315)),
    ((17, 9, "422", "planar", "420", None), ([(0, 17, 17, 17, 9), (153, 9, 9, 9, 5), (198, 9, 9, 9, 5)], 243)),
    ((17, 9, "422", "semiplanar", "420", None), ([(0, 17, 17, 17, 9), (153, 18, 18, 9, 5)], 243)),
    ((17, 9, "422", "uyvy", "coded", None), ([(0, 36, 36, 17, 9)], 324)),
    ((17, 9, "444", "planar", "coded", None), ([(0, 17, 17, 17, 9), (153, 17, 17, 17, 9), (306, 17, 17, 17, 9)], 459)),
    ((17, 9, "444", "semiplanar", "coded", None), ([(0, 17, 17, 17, 9), (153, 34, 34, 17, 9)], 459)),
    ((17, 9, "440", "planar", "coded", None), ([(0, 17, 17, 17, 9), (153, 17, 17, 17, 5), (238, 17, 17, 17, 5)], 323)),
    ((17, 9, "420", "planar", "coded", None), ([(0, 17, 17, 17, 9), (153, 9, 9, 9, 5), (198, 9, 9, 9, 5)], 243)),
    ((17, 9, "420", "semiplanar", "coded", None), ([(0, 17, 17, 17, 9), (153, 18, 18, 9, 5)], 243)),
    ((17, 9, "gray", "semiplanar", "coded", None), ([(0, 17, 17, 17, 9)], 153)),
    ((1000, 1, "422", "planar", "coded", None), ([(0, 1000, 1000, 1000, 1), (1000, 500, 500, 500, 1), (1500, 500, 500, 500, 1)], 2000)),
    ((1000, 1, "422", "yuyv", "coded", None), ([(0, 2000, 2000, 1000, 1)], 2000)),
    ((1000, 1, "420", "planar", "coded", None), ([(0, 1000, 1000, 1000, 1), (1000, 500, 500, 500, 1), (1500, 500, 500, 500, 1)], 2000)),
    ((1000, 1, "440", "semiplanar", "coded", None), ([(0, 1000, 1000, 1000, 1), (1000, 2000, 2000, 1000, 1)], 3000)),
    ((33, 31, "422", "planar", "coded", (48, 32)), ([(0, 48, 33, 33, 31), (1488, 32, 17, 17, 31), (2480, 32, 17, 17, 31)], 3472)),
    ((33, 31, "422", "semiplanar", "420", (0, 64)), ([(0, 33, 33, 33, 31), (1023, 64, 34, 17, 16)], 2047)),
    ((33, 31, "420", "planar", "coded", None), ([(0, 33, 33, 33, 31), (1023, 17, 17, 17, 16), (1295, 17, 17, 17, 16)], 1567)),
    ((33, 31, "420", "semiplanar", "coded", (64, 0)), ([(0, 64, 33, 33, 31), (1984, 34, 34, 17, 16)], 2528)),
    ((33, 31, "gray", "planar", "coded", (40, 0)), ([(0, 40, 33, 33, 31)], 1240)),
    ((1920, 1080, "422", "semiplanar", "420", None), ([(0, 1920, 1920, 1920, 1080), (2073600, 1920, 1920, 960, 540)], 3110400)),   # NV12
    ((1920, 1080, "422", "yuyv", "coded", None), ([(0, 3840, 3840, 1920, 1080)], 4147200)),                                          # YUY2
]


@pytest.mark.parametrize("case, want", TABLE, ids=lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) and len(v) == 6 else "")
def test_shape_against_the_table(case, want):
    w, h, sampling, format, chroma, pitch = case
    hs, vs = ps.SAMPLINGS[sampling]
    comps = 1 if sampling == "gray" else 3
    spec = ca._planes_spec(format, chroma, pitch)
    rc, lay = _shape(spec, w, h, comps, hs, vs)
    assert rc == 0, lib.compeg_last_error()
    got = [(lay.offset[p], lay.pitch[p], lay.row_bytes[p], lay.width[p], lay.height[p]) for p in range(lay.planes)]
    assert (got, lay.total_bytes) == want and lay.reserved == 0
    assert all((lay.offset[p], lay.pitch[p], lay.row_bytes[p], lay.width[p], lay.height[p]) == (0, 0, 0, 0, 0) for p in range(lay.planes, 3))
    assert ps.layout(w, h, comps, hs, vs, format, chroma, pitch) == want          # (the restatement the other tests lay their bytes out by)
    planes, total = ca.planes_shape(w, h, (hs, vs), comps, format, chroma, pitch)   # (and the Python mirror)
    assert total == want[1] and [(p["offset"], p["pitch"], p["row_bytes"], p["width"], p["height"]) for p in planes] == want[0]


@pytest.mark.parametrize("args, code, words", [
    ((_spec(2), 16, 8, 3, 1, 1), ca.E_UNSUPPORTED, ("yuyv", "4:2:2 files only", "4:4:4")),
    ((_spec(3), 16, 8, 3, 2, 2), ca.E_UNSUPPORTED, ("uyvy", "4:2:2 files only", "4:2:0")),
    ((_spec(2), 16, 8, 1, 1, 1), ca.E_UNSUPPORTED, ("4:2:2 files only", "grayscale")),
    ((_spec(0, 1), 16, 8, 3, 1, 2), ca.E_UNSUPPORTED, ("chroma 1 (4:2:0)", "from 4:2:2 files only", "4:4:0")),
    ((_spec(1, 1), 16, 8, 3, 2, 2), ca.E_UNSUPPORTED, ("chroma 1 (4:2:0)", "from 4:2:2 files only", "4:2:0")),
    ((_spec(2, 1), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("chroma 1 (4:2:0)", "planar and semiplanar", "packed")),
    ((_spec(0, 0, 15), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("luma_pitch 15", "below", "16 bytes")),
    ((_spec(0, 0, 0, 7), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("chroma_pitch 7", "below", "8 bytes")),
    ((_spec(1, 0, 0, 15), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("chroma_pitch 15", "16 bytes")),
    ((_spec(2, 0, 31), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("luma_pitch 31", "32 bytes")),
    ((_spec(reserved=(0, 0, 0, 1)), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("reserved must be 0",)),
    ((_spec(reserved=(7, 0, 0, 0)), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("reserved must be 0",)),
    ((_spec(4), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("format 4",)),
    ((_spec(0, 2), 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("chroma 2",)),
    ((_spec(), 0, 8, 3, 2, 1), ca.E_INVALID_ARG, ("no pixels",)),
    ((_spec(), 16, 8, 2, 2, 1), ca.E_INVALID_ARG, ("2 components",)),
    ((_spec(), 16, 8, 3, 4, 1), ca.E_INVALID_ARG, ("luma sampling 4x1",)),
    ((None, 16, 8, 3, 2, 1), ca.E_INVALID_ARG, ("spec is NULL",)),
], ids=lambda v: None)
def test_refusals_with_their_messages(args, code, words):
    rc, lay = _shape(*args)
    assert rc == code
    assert bytes(lay) == b"\xdd" * C.sizeof(lay)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message


def test_python_names_are_checked():
    with pytest.raises(ca.Error, match="unknown planes format"):
        ca.planes_shape(16, 8, format="nv12")
    with pytest.raises(ca.Error, match="unknown planes chroma"):
        ca.planes_shape(16, 8, chroma="411")


def test_image_sampling():
    assert ca.ImageData(cs.case("texture/edge/422/reference/dri4").jpeg()).sampling() == (2, 1)
    for lay in ("444", "440", "420"):
        assert ca.ImageData(cs.case(f"texture/edge/{lay}/reference/dri4").jpeg(), allow_sampling=True).sampling() == ps.SAMPLINGS[lay]
    g = ca.ImageData(gs.cases()[0].jpeg(), allow_grayscale=True)
    assert g.sampling() == (1, 1) and g.components() == 1
    hs = C.c_uint32(9)
    assert lib.compeg_image_sampling(None, C.byref(hs), None) == ca.E_INVALID_ARG and hs.value == 9


def test_c99_consumer_compiles_against_the_header(tmp_path):
    """tests/c_consumer includes the header as C99; so does this unit, which also touches the new declarations."""
    src = tmp_path / "planes_c99.c"
    src.write_text('#include "compeg_hip.h"\n'
                   "int main(void) {\n"
                   "    compeg_planes_spec spec = {COMPEG_PLANES_SEMIPLANAR, COMPEG_CHROMA_420, 0, 0, {0, 0, 0, 0}};\n"
                   "    compeg_planes_layout lay;\n"
                   "    uint32_t hs = 0, vs = 0;\n"
                   "    (void)compeg_image_sampling(0, &hs, &vs);\n"
                   "    if (compeg_planes_shape(&spec, 1920, 1080, 3, 2, 1, &lay) != 0) return 1;\n"
                   "    return lay.total_bytes == 3110400u && sizeof spec == 32 && sizeof lay == 88 && COMPEG_KERNEL_PLANES == 9 ? 0 : 1;\n"
                   "}\n")
    for unit in (str(src), os.path.join(ROOT, "tests", "c_consumer", "consumer.c")):
        subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), unit])
    exe = tmp_path / "planes_c99"
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           ca.LIB_PATH, "-Wl,-rpath," + os.path.dirname(ca.LIB_PATH)])
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
