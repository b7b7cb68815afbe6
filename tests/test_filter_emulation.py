"""The filter_tensor kernels' lane body (compeg_amd/csrc/filter_body.h) on the CPU: tests/emul_filter/filter_driver.cpp,
a stand-alone program compiled with g++ -fsanitize=address,undefined and the flags of tests/test_antialias_emulation.py,
plans every launch with the library's planners -- records, axis tables, grid -- and runs its grid lane by lane over RGBA
images laid out as the runtime allocates them: rows and pitch padded to 16 pixels, the padding filled with 0xA5 so that
a padding byte that leaks into a tap shows, every image and the records with their tables heap blocks of their own so
that a load outside them is the sanitizer's to report.  The destination lies one element into a larger buffer between
sentinel bytes that must survive, and is itself filled with the sentinel: an element that no lane writes shows too.
Every element is compared with tests/filter_reference.py, bit for bit, with bands of 8 rows (what the library compiles)
and of 3: the result does not depend on the band."""
import os
import struct
import subprocess

import pytest

import numpy as np

import filter_reference as fr
from conftest import ROOT

SENTINEL = 0x5C
PAD_BYTE = 0xA5
GREY = (114.0, 114.0, 114.0)
COLOURS = (10.0, 114.0, 250.5)   # one value per channel: a plane that takes the wrong one shows
FIVE = tuple((w, h, 20 + i) for i, (w, h) in enumerate(fr.gr.FIVE))
# six regions over five images: image 4 twice, image 2 twice with the same crop, images 1 and 3 once, image 0 not at all;
# inner rectangles whose dy and dh are multiples of neither 8 nor 3; every axis within Lanczos' limit (21 to 1)
SIX = ((4, (101, 3, 200, 64), (2, 4, 20, 6)), (2, (3, 1, 45, 21), (0, 3, 24, 11)), (4, None, (0, 7, 24, 5)),
       (2, (3, 1, 45, 21), (0, 3, 24, 11)), (1, (5, 2, 12, 7), (7, 0, 9, 20)), (3, (2, 0, 20, 16), (23, 19, 1, 1)))


def _case(images, regions, size, k, dtype, order, kernel, pad=COLOURS, params=None, offset=None, axes=None, band=8):
    """images: ((w, h, seed), ...); regions: ((image, src or None, dst or None), ...); axes: how many axis tables the launch
    must build (None: not checked)"""
    scale, bias = params or fr.params(dtype)
    return dict(images=tuple(images), regions=tuple(regions), size=size, k=k, dtype=dtype, order=order, kernel=kernel, pad=pad, scale=scale,
                bias=bias, axes=axes, band=band, offset=64 + fr.ELEM_BYTES[dtype] if offset is None else offset)


def _cases():
    cases, n = [], 0
    one = ((330, 70, 3),)
    imagenet = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    # every kernel x element type x k: the letterbox of 330x70 into 48x40 (rows 15 .. 24: dy and dh multiples of neither band)
    for kernel in fr.KERNELS:
        for dtype in fr.DTYPES:
            for k in (1, 2, 4, 8):
                n += 1
                dst = fr.fit((330, 70), (48, 40))
                cases.append(_case(one, ((0, None, dst),), (48, 40), k, dtype, ("rgb", "bgr")[n % 2], kernel, pad=GREY if n % 3 else COLOURS,
                                   band=(8, 3)[(n // 2) % 2]))
    for kernel in fr.KERNELS:
        for band in (8, 3):
            # the contraction shape, the ImageNet pair in f32, both orders
            cases.append(_case(one, ((0, None, None),), (31, 13), 1, "f32", ("rgb", "bgr")[band % 2], kernel, params=imagenet, band=band))
            # one axis shrinks, the other grows; an output of one row, one of one column; as many rows as a band, one fewer, one more
            cases.append(_case(one, ((0, None, None), (0, (5, 3, 20, 16), (32, 16, 1, 1))), (33, 100), 1, "f16", "rgb", kernel, band=band, axes=4))
            cases.append(_case(one, ((0, (0, 0, 20, 70), None),), (40, 9), 1, "f16", "bgr", kernel, band=band))
            for oh in (1, band - 1, band, band + 1, 13):
                cases.append(_case(((50, 26, 5),), ((0, (0, 3, 50, 20), None),), (5, oh), 1, "f32", "rgb", kernel, params=imagenet, band=band))
            cases.append(_case(((17, 9, 6),), ((0, None, None), (0, None, (3, 5, 1, 1)), (0, None, (0, 1, 8, 7))), (16, 8), 1, "u8", "rgb", kernel, band=band))
            # region lists over five images of five sizes, repeated, out of order, one image skipped; more than one workgroup a slot
            for d, dtype in enumerate(fr.DTYPES):
                cases.append(_case(FIVE, SIX, (24, 20), 1, dtype, ("rgb", "bgr")[d % 2], kernel, band=band, params=imagenet if dtype != "u8" else None))
            cases.append(_case(FIVE, SIX[:5], (24, 20), 2, "f16", "bgr", kernel, offset=64, band=band))
    # each kernel at its tap limit on one axis
    for kernel, n_in, n_out in (("box", 128, 1), ("triangle", 128, 2), ("bicubic", 64, 2), ("lanczos3", 64, 3)):
        cases.append(_case(((n_in, 9, 7),), ((0, None, None),), (n_out, 9), 1, "f32", "rgb", kernel))
        cases.append(_case(((17, n_in, 8),), ((0, None, None),), (17, n_out), 1, "f16", "bgr", kernel, band=3))
    # 257 columns: more than one workgroup a band
    cases.append(_case(one, ((0, None, (0, 2, 257, 9)),), (257, 11), 1, "u8", "rgb", "bicubic"))
    return cases


CASES = _cases()


def _rect(r):
    return "w" if r is None else "%d.%d.%d.%d" % r


def _id(c):
    images = "+".join(f"{w}x{h}" for w, h, _ in c["images"])
    regions = "+".join(f"{i}s{_rect(s)}d{_rect(d)}" for i, s, d in c["regions"]) if len(c["regions"]) < 3 else f"{len(c['regions'])}regions"
    pad = "pad" + ".".join("%g" % p for p in c["pad"])
    return f"{images}-{regions}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['kernel']}-{c['dtype']}-{c['order']}-{pad}-at{c['offset']}-band{c['band']}"


_frames = {}


def _rgba(w, h, seed):
    if (w, h, seed) not in _frames:
        _frames[(w, h, seed)] = fr.frame(w, h, seed=seed)[1]
    return _frames[(w, h, seed)]


def _allocation(w, h, seed):
    """(pitch, rows, bytes) of one image as the runtime allocates it."""
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    alloc = np.full((rows, pitch), PAD_BYTE, dtype=np.uint8)
    alloc[:h, :w * 4] = _rgba(w, h, seed).reshape(h, w * 4)
    return pitch, rows, alloc.tobytes()


def _needed(c):
    return len(c["regions"]) * 3 * c["size"][1] * c["size"][0] * fr.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_filter")
    exe = str(tmp / "filter_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_filter", "filter_driver.cpp"), "-o", exe])
    return tmp, exe


@pytest.fixture(scope="module")
def packed(driver):
    """Every case through one run of the driver: case index -> (the destination buffer afterwards, axis tables built)."""
    tmp, exe = driver
    blob, totals = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        total = (c["offset"] + _needed(c) + 64 + 255) // 256 * 256
        totals.append(total)
        ow, oh = c["size"]
        blob.append(struct.pack("<9I9f2I", len(c["regions"]), len(c["images"]), c["k"], fr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                fr.KERNELS.index(c["kernel"]), ow, oh, c["band"], *c["scale"], *c["bias"], *c["pad"], c["offset"], total))
        sources = []
        for w, h, seed in c["images"]:
            pitch, rows, raw = _allocation(w, h, seed)
            blob.append(struct.pack("<4I", w, h, pitch, rows))
            sources.append(raw)
        for image, src, dst in c["regions"]:
            w, h, _ = c["images"][image]
            blob.append(struct.pack("<9I", image, *(src if src is not None else (0, 0, w, h)), *(dst if dst is not None else (0, 0, ow, oh))))
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
def test_lane_bodies_match_the_contract_and_stay_inside_the_tensor(packed, index):
    c, (buf, axes) = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = fr.from_bytes(buf[lo:hi], c["dtype"], (len(c["regions"]), 3, oh, ow))
    for r, (image, src, dst) in enumerate(c["regions"]):
        w, h, seed = c["images"][image]
        want = fr.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["kernel"], src, dst, c["pad"])
        assert fr.same(got[r], want, c["dtype"]), f"region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"
    if c["axes"] is not None:
        assert axes == c["axes"], f"the launch built {axes} axis tables"


def test_a_fused_accumulate_shows(packed):
    """The mutant of DESIGN.md 5.9 -- float32(float64(P) * float64(w) + float64(h)), what a contracted multiply-add would give --
    differs from what the lane bodies stored, for every kernel, on the contraction shape."""
    for index, c in enumerate(CASES):
        if c["size"] != (31, 13):
            continue
        w, h, seed = c["images"][0]
        lo = c["offset"]
        got = fr.from_bytes(packed[index][0][lo:lo + _needed(c)], c["dtype"], (1, 3, 13, 31))[0]
        mutant = fr.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["kernel"], fused=True)
        differing = int((got != mutant).sum())
        print(f"{c['kernel']} band {c['band']}: {differing} of {mutant.size} elements differ under a fused accumulate")
        assert differing > 0


def test_the_planner_refuses_a_grid_that_does_not_fit(driver):
    """65535 x 65535: 8193 bands of 65535 lanes a slot, 2 097 377 workgroups of 256; 2^31 - 1 workgroups is the limit, which
    1023 slots meet and 1024 do not."""
    def fits(slots):
        r = subprocess.run([driver[1], "--plan", "2", "0", "65535", "65535", str(slots)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip()
    assert fits(1) == "fits 1" and fits(1023) == "fits 1"
    assert fits(1024) == "fits 0" and fits(4096) == "fits 0"
