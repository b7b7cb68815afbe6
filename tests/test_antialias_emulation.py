"""The resize_tensor_antialias kernels' lane body (compeg_amd/csrc/antialias_body.h) on the CPU:
tests/emul_antialias/antialias_driver.cpp, compiled with g++ -fsanitize=address,undefined and the flags of
tests/test_resize_emulation.py, plans every launch with the library's planner -- records and axis tables -- and runs
its grid lane by lane over RGBA images laid out as the runtime allocates them: rows and pitch padded to 16 pixels, the
padding filled with 0xA5 so that a padding byte that leaks into a tap shows, every image and the tables heap blocks of
their own so that a load outside them is the sanitizer's to report.  The destination lies one element into a larger
buffer between sentinel bytes that must survive.  Every element is compared with tests/antialias_reference.py.

Of the shapes the CPU reference is checked on, two are thinned out here because the grid runs lane by lane under the
sanitizers: 640x360 -> 224x224 runs once (f16, rgb) rather than in every element type and order, and 3840x2160 ->
224x224 (35 million taps, and a 4K frame to encode and decode first) does not run at all; its tap counts, 35 on x and 20
on y, are below those of 50x26 -> 1x1 (50 and 26), which does run, and the card runs the shape itself in the probe
(tools/resize_probe.py --antialias compares slot 0 with the reference)."""
import os
import struct
import subprocess

import pytest

import numpy as np

import antialias_reference as ar
from conftest import ROOT

FILTER = 0x101   # bilinear | antialias
SENTINEL = 0x5C
PAD = 0xA5
# (w, h, k, (ow, oh)): both axes shrink; one axis on each road; neither shrinks; the identity extent
SHAPES = ((330, 70, 1, (31, 13)), (330, 70, 2, (31, 13)), (50, 26, 1, (5, 3)), (17, 9, 1, (16, 8)), (17, 9, 1, (1, 1)), (50, 26, 1, (1, 1)),
          (330, 70, 1, (224, 224)), (17, 9, 1, (64, 64)), (16, 8, 1, (24, 20)), (50, 26, 1, (50, 26)), (50, 26, 1, (64, 26)))
FIVE = ((16, 8, 3, (1, 1, 15, 7)), (17, 9, 4, (0, 0, 17, 9)), (50, 26, 5, (3, 1, 45, 21)), (66, 26, 6, (2, 0, 64, 26)), (330, 70, 7, (101, 3, 200, 64)))


def _case(images, size, k, dtype, order, offset=None, axes=None):
    """images: ((w, h, seed, crop or None), ...); axes: how many axis tables the launch must build (None: not checked)"""
    scale, bias = ar.params(dtype)
    return dict(images=tuple(images), size=size, k=k, dtype=dtype, order=order, scale=scale, bias=bias, axes=axes,
                offset=64 + ar.ELEM_BYTES[dtype] if offset is None else offset)


def _cases():
    cases, n = [], 0
    for w, h, k, size in SHAPES:
        n += 1
        for d, dtype in enumerate(ar.DTYPES):
            cases.append(_case(((w, h, 3, None),), size, k, dtype, ("rgb", "bgr")[(n + d) % 2], axes=2))
    cases.append(_case(((640, 360, 3, None),), (224, 224), 1, "f16", "rgb", offset=64))
    # crops on 330x70: flush with the right and bottom edges, an odd origin, exactly k x k in the far corner, 1 x 1
    for k in (1, 2, 8):
        for crop in ((330 - 97, 70 - 33, 97, 33), (5, 3, 201, 45), (330 - k, 70 - k, k, k)):
            for size in ((17, 9), (64, 64), (40, 3)):
                n += 1
                cases.append(_case(((330, 70, 3, crop),), size, k, ar.DTYPES[n % 4], ("rgb", "bgr")[n // 4 % 2]))
    cases.append(_case(((330, 70, 3, (129, 30, 1, 1)),), (5, 3), 1, "f16", "rgb"))
    cases.append(_case(((330, 70, 3, (329, 69, 1, 1)),), (1, 1), 1, "u8", "bgr"))
    # k = 8 down to one element: the longest lanes here
    cases.append(_case(((330, 70, 3, None),), (1, 1), 8, "f32", "rgb"))
    cases.append(_case(((330, 70, 3, None),), (7, 2), 4, "bf16", "bgr"))
    # one launch of five images of five sizes with a crop each: some shrink, some grow, each has its own tables
    for d, dtype in enumerate(ar.DTYPES):
        cases.append(_case(FIVE, (24, 20), 1, dtype, ("rgb", "bgr")[d % 2], axes=10))
    cases.append(_case(FIVE, (24, 20), 4, "f16", "bgr"))
    # three images of one size: two tables, not six; planes with an odd element count (35 x 13 = 455)
    for dtype in ar.DTYPES:
        cases.append(_case(tuple((50, 26, 3 + i, None) for i in range(3)), (35, 13), 1, dtype, "rgb", axes=2))
    # at an aligned address
    for dtype in ar.DTYPES:
        cases.append(_case(((330, 70, 3, None), (330, 70, 4, None)), (48, 16), 1, dtype, "bgr", offset=64, axes=2))
    # a square source and a square output: one table serves both axes
    cases.append(_case(((330, 70, 3, (0, 0, 64, 64)),), (24, 24), 1, "f16", "rgb", axes=1))
    return cases


CASES = _cases()


def _id(c):
    images = "+".join(f"{w}x{h}" + ("" if crop is None else "c%d.%d.%d.%d" % crop) for w, h, seed, crop in c["images"])
    return f"{images}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['dtype']}-{c['order']}-at{c['offset']}"


_frames = {}


def _rgba(w, h, seed):
    if (w, h, seed) not in _frames:
        _frames[(w, h, seed)] = ar.frame(w, h, seed=seed)[1]
    return _frames[(w, h, seed)]


def _allocation(w, h, seed):
    """(pitch, rows, bytes) of one image as the runtime allocates it."""
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    alloc = np.full((rows, pitch), PAD, dtype=np.uint8)
    alloc[:h, :w * 4] = _rgba(w, h, seed).reshape(h, w * 4)
    return pitch, rows, alloc.tobytes()


def _needed(c):
    return len(c["images"]) * 3 * c["size"][1] * c["size"][0] * ar.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through one run of the driver: case index -> (the destination buffer afterwards, axis tables built)."""
    tmp = tmp_path_factory.mktemp("emul_antialias")
    exe = str(tmp / "antialias_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_antialias", "antialias_driver.cpp"), "-o", exe])
    blob, totals = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        total = (c["offset"] + _needed(c) + 64 + 255) // 256 * 256
        totals.append(total)
        blob.append(struct.pack("<7I6f2I", len(c["images"]), c["k"], ar.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                FILTER, c["size"][0], c["size"][1], *c["scale"], *c["bias"], c["offset"], total))
        sources = []
        for w, h, seed, crop in c["images"]:
            pitch, rows, raw = _allocation(w, h, seed)
            blob.append(struct.pack("<8I", w, h, pitch, rows, *(crop if crop is not None else (0, 0, w, h))))
            sources.append(raw)
        blob.extend(sources)
        blob.append(bytes([SENTINEL]) * total)
    (tmp / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    out, at, result = (tmp / "out.bin").read_bytes(), 0, []
    for total in totals:
        result.append((out[at:at + total], struct.unpack_from("<I", out, at + total)[0]))
        at += total + 4
    assert at == len(out)
    return result


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_body_matches_the_contract_and_stays_inside_the_tensor(packed, index):
    c, (buf, axes) = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = ar.from_bytes(buf[lo:hi], c["dtype"], (len(c["images"]), 3, oh, ow))
    for i, (w, h, seed, crop) in enumerate(c["images"]):
        want = ar.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], crop)
        assert ar.same(got[i], want, c["dtype"]), f"image {i}: {int((got[i] != want).sum())} of {want.size} elements differ"
    if c["axes"] is not None:
        assert axes == c["axes"], f"the launch built {axes} axis tables"
