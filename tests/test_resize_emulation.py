"""The resize_tensor kernels' lane body (compeg_amd/csrc/resize_body.h) on the CPU: tests/emul_resize/resize_driver.cpp,
compiled with g++ -fsanitize=address,undefined, plans every launch like the library and runs its grid lane by lane
over RGBA images laid out as the runtime allocates them -- rows and pitch padded to 16 pixels, the padding filled
with 0xA5 so that a padding byte that leaks into a tap shows, every image a heap block of its own so that a tap
outside it is the sanitizer's to report.  The destination lies one element into a larger buffer (rows, planes and
images then begin at every alignment) between sentinel bytes that must survive; a few cases lie at an aligned
address as well, where whole runs leave as 16-byte stores."""
import os
import struct
import subprocess

import pytest

import numpy as np

import numeric_edges as ne
import resize_reference as rr
from conftest import ROOT

SIZES = ((16, 8), (17, 9), (50, 26), (330, 70), (7, 5))
OUTPUTS = ((1, 1), (5, 3), (17, 9), (33, 7), (64, 64), (31, 13))
SENTINEL = 0x5C
PAD = 0xA5


def _case(images, size, k, dtype, filter, order, offset=None, identity=False, edge=None):
    """images: ((w, h, seed, crop or None), ...); a seed that is a name is a frame of tests/numeric_edges.py, and edge
    the set of its whose scale and bias the case takes"""
    scale, bias = rr.params(dtype, identity) if edge is None else ne.SETS[edge][1:]
    c = dict(images=tuple(images), size=size, k=k, dtype=dtype, filter=filter, order=order, scale=scale, bias=bias,
             offset=64 + rr.ELEM_BYTES[dtype] if offset is None else offset)
    if edge is not None:
        c["edge"] = edge
    return c


def _cases():
    cases, n = [], 0
    # every size x admissible k x output extent (and the identity extent), the other parameters in rotation so that
    # every element type, filter and order meets every k and every kind of extent
    for w, h in SIZES:
        for k in rr.ks_for(w, h):
            for size in OUTPUTS + (rr.pre_extent(w, h, k),):
                n += 1
                dtype, filter, order = rr.DTYPES[n % 4], rr.FILTERS[(n // 4) % 2], ("rgb", "bgr")[(n // 8) % 2]
                cases.append(_case(((w, h, 3, None),), size, k, dtype, filter, order))
    # every element type x filter on one geometry of each kind: down, up, identity
    for dtype in rr.DTYPES:
        for filter in rr.FILTERS:
            for size in ((31, 13), (64, 64), (25, 13)):
                cases.append(_case(((50, 26, 3, None),), size, 2, dtype, filter, "rgb"))
            cases.append(_case(((330, 70, 3, None),), (64, 64), 4, dtype, filter, "bgr"))
    # the identity planes: u8, scale 1, bias 0
    cases.append(_case(((50, 26, 3, None),), (50, 26), 1, "u8", "bilinear", "rgb", identity=True))
    # crops on 330x70: flush with the right and bottom edges, an odd origin, 1x1 (k = 1), exactly k x k
    for filter in rr.FILTERS:
        for k in (1, 2, 4, 8):
            for crop in ((330 - 97, 70 - 33, 97, 33), (5, 3, 201, 45), (4, 7, 128, 40), (329, 69, k, k) if k == 1 else (330 - k, 70 - k, k, k),
                         (13, 21, k, k)):
                n += 1
                for size in ((17, 9), rr.pre_extent(330, 70, k, crop)):
                    cases.append(_case(((330, 70, 3, crop),), size, k, rr.DTYPES[n % 4], filter, ("rgb", "bgr")[n % 2]))
    cases.append(_case(((330, 70, 3, (129, 30, 1, 1)),), (5, 3), 1, "f16", "bilinear", "rgb"))
    # one launch of five images of five sizes with a crop each
    five = ((16, 8, 3, (1, 1, 15, 7)), (17, 9, 4, (0, 0, 17, 9)), (50, 26, 5, (3, 1, 45, 21)), (66, 26, 6, (2, 0, 64, 26)), (330, 70, 7, (101, 3, 200, 64)))
    for dtype in rr.DTYPES:
        for filter in rr.FILTERS:
            cases.append(_case(five, (24, 20), 1, dtype, filter, "rgb"))
    cases.append(_case(five, (24, 20), 4, "f16", "bilinear", "bgr"))
    # a three-image launch whose planes have an odd element count (35 x 13 = 455)
    for dtype in rr.DTYPES:
        cases.append(_case(tuple((50, 26, 3 + i, None) for i in range(3)), (35, 13), 2, dtype, "bilinear", "rgb"))
    # at an aligned address: rows of whole 16-byte runs, and rows that end inside one
    for w, h, k, size in ((16, 8, 1, (64, 64)), (330, 70, 1, (64, 64)), (330, 70, 2, (33, 7)), (50, 26, 1, (48, 16))):
        for dtype in rr.DTYPES:
            cases.append(_case(((w, h, 3, None), (w, h, 4, None)), size, k, dtype, "bilinear", "bgr", offset=64))
    # the numeric edges (tests/numeric_edges.py): every set on the ramp at k = 1 (taps that straddle its tiles) and on
    # the noisy frame at k = 2 and k = 8, aligned and misaligned by one element; nearest at the ramp's identity extent
    frame, k1, size1, crop1 = ne.RESIZE_EDGE
    for name, dtype in ne.SET_DTYPES:
        for offset in (64, None):
            n += 1
            order = ("rgb", "bgr")[n % 2]
            cases.append(_case(((ne.RAMP_W, ne.RAMP_H, frame, crop1),), size1, k1, dtype, "bilinear", order, offset=offset, edge=name))
            cases.append(_case(((*ne.NOISY, "noisy", None),), (64, 64), 2, dtype, "bilinear", order, offset=offset, edge=name))
            cases.append(_case(((*ne.NOISY, "noisy", None),), (33, 7), 8, dtype, "bilinear", order, offset=offset, edge=name))
        cases.append(_case(((ne.RAMP_W, ne.RAMP_H, "ramp", None),), (ne.RAMP_W, ne.RAMP_H), 1, dtype, "nearest", "rgb", edge=name))
    return cases


CASES = _cases()


def _id(c):
    images = "+".join((seed if isinstance(seed, str) else "") + f"{w}x{h}" + ("" if crop is None else "c%d.%d.%d.%d" % crop)
                      for w, h, seed, crop in c["images"])
    if "edge" in c:
        images = f"{c['edge']}-{images}"
    return f"{images}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['dtype']}-{c['filter']}-{c['order']}-at{c['offset']}"


def _rgba(w, h, seed):
    """The frame of a case's image: tensor_reference's by seed, or one of tests/numeric_edges.py by name."""
    if isinstance(seed, str):
        rgba = ne.FRAMES[seed]()[1]
        assert rgba.shape == (h, w, 4)
        return rgba
    return rr.frame(w, h, seed=seed)[1]


def _allocation(w, h, seed):
    """(pitch, rows, bytes) of one image as the runtime allocates it."""
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    alloc = np.full((rows, pitch), PAD, dtype=np.uint8)
    alloc[:h, :w * 4] = _rgba(w, h, seed).reshape(h, w * 4)
    return pitch, rows, alloc.tobytes()


def _needed(c):
    return len(c["images"]) * 3 * c["size"][1] * c["size"][0] * rr.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through one run of the driver: case index -> the destination buffer afterwards."""
    tmp = tmp_path_factory.mktemp("emul_resize")
    exe = str(tmp / "resize_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_resize", "resize_driver.cpp"), "-o", exe])
    blob, totals = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        total = (c["offset"] + _needed(c) + 64 + 255) // 256 * 256
        totals.append(total)
        blob.append(struct.pack("<7I6f2I", len(c["images"]), c["k"], rr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                rr.FILTERS.index(c["filter"]), c["size"][0], c["size"][1], *c["scale"], *c["bias"], c["offset"], total))
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
        result.append(out[at:at + total])
        at += total
    assert at == len(out)
    return result


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_body_matches_the_formula_and_stays_inside_the_tensor(packed, index):
    c, buf = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = rr.from_bytes(buf[lo:hi], c["dtype"], (len(c["images"]), 3, oh, ow))
    for i, (w, h, seed, crop) in enumerate(c["images"]):
        with np.errstate(over="ignore"):   # (the edge sets overflow to infinity on purpose)
            want = rr.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["filter"], crop)
        assert rr.same(got[i], want, c["dtype"]), f"image {i}: {int((got[i] != want).sum())} of {want.size} elements differ"
