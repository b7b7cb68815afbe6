"""The region_tensor kernels' lane bodies (compeg_amd/csrc/region_body.h) on the CPU: tests/emul_region/region_driver.cpp,
a stand-alone program compiled with g++ -fsanitize=address,undefined and the flags of tests/test_resize_emulation.py,
plans every launch with the library's planners -- records, axis tables, grid -- and runs its grid lane by lane over RGBA
images laid out as the runtime allocates them: rows and pitch padded to 16 pixels, the padding filled with 0xA5 so that
a padding byte that leaks into a tap shows, every image and the records with their tables heap blocks of their own so
that a load outside them is the sanitizer's to report.  The destination lies one element into a larger buffer between
sentinel bytes that must survive, and is itself filled with the sentinel: an element that no lane writes shows too.
Every element is compared with tests/region_reference.py."""
import os
import struct
import subprocess

import pytest

import numpy as np

import region_reference as gr
from conftest import ROOT

FILTER = {"nearest": 0, "bilinear": 1, "antialias": 0x101}
SENTINEL = 0x5C
PAD_BYTE = 0xA5
GREY = (114.0, 114.0, 114.0)
COLOURS = (10.0, 114.0, 250.5)   # one value per channel: a plane that takes the wrong one shows
FIVE = tuple((w, h, 20 + i) for i, (w, h) in enumerate(gr.FIVE))


def _case(images, regions, size, k, dtype, order, filter, pad=COLOURS, params=None, offset=None, axes=None):
    """images: ((w, h, seed), ...); regions: ((image, src or None, dst or None), ...); axes: how many axis tables the launch
    must build (None: not checked)"""
    scale, bias = params or gr.params(dtype)
    return dict(images=tuple(images), regions=tuple(regions), size=size, k=k, dtype=dtype, order=order, filter=filter, pad=pad, scale=scale,
                bias=bias, axes=axes, offset=64 + gr.ELEM_BYTES[dtype] if offset is None else offset)


def _cases():
    cases, n = [], 0
    one = ((330, 70, 3),)
    # every filter x element type x k: the letterbox of 330x70 (k = 1; what k leaves of it at 2 and 8) into 48x40
    for filter in gr.FILTERS:
        for dtype in gr.DTYPES:
            for k in (1, 2, 8):
                n += 1
                dst = gr.fit((330, 70), (48, 40))
                cases.append(_case(one, ((0, None, dst),), (48, 40), k, dtype, ("rgb", "bgr")[n % 2], filter, pad=GREY if n % 3 else COLOURS))
    # borders that fall inside a run on both sides (u8: 16 elements a run, f32: 4; the 16-bit types between), a 1x1 dst in
    # the far corner, dst the whole output -- named and as all zeros
    for filter in gr.FILTERS:
        for dtype in gr.DTYPES:
            n += 1
            order = ("rgb", "bgr")[n % 2]
            cases.append(_case(one, ((0, None, (5, 3, 21, 9)),), (33, 17), 1, dtype, order, filter))
            cases.append(_case(one, ((0, (5, 3, 40, 30), (32, 16, 1, 1)),), (33, 17), 1, dtype, order, filter))
            cases.append(_case(one, ((0, None, None), (0, None, (0, 0, 33, 17))), (33, 17), 2, dtype, order, filter, axes=2 if filter == "antialias" else 0))
    # a dst one column wide at a run's last element and one row high; flush right and bottom
    cases.append(_case(one, ((0, None, (15, 0, 1, 17)), (0, None, (0, 16, 33, 1)), (0, None, (17, 8, 16, 9))), (33, 17), 1, "u8", "rgb", "bilinear"))
    cases.append(_case(one, ((0, (100, 0, 60, 70), (15, 0, 1, 17)), (0, (0, 6, 330, 64), (0, 16, 33, 1)), (0, None, (17, 8, 16, 9))), (33, 17), 1, "f16", "bgr",
                       "antialias"))
    # seven regions over five images of five sizes, repeated and out of order; more than one workgroup a slot
    for filter in gr.FILTERS:
        for d, dtype in enumerate(gr.DTYPES):
            cases.append(_case(FIVE, gr.SEVEN, (24, 20), 1, dtype, ("rgb", "bgr")[d % 2], filter))
    cases.append(_case(FIVE, gr.SEVEN, (24, 20), 4, "f16", "bgr", "antialias", offset=64))
    cases.append(_case(FIVE, gr.SEVEN[:3], (24, 20), 1, "f32", "rgb", "bilinear", offset=64))   # fewer regions than images
    # six crops of one frame, one repeated, one of k x k pixels in the far corner
    for k in (1, 2, 8):
        crops = ((0, (10, 5, 100, 40), None), (0, (200, 30, 64, 32), None), (0, (10, 5, 100, 40), None), (0, (330 - k, 70 - k, k, k), None),
                 (0, None, gr.fit((330, 70), (24, 20), "top_left")), (0, (129, 30, 9, 24), gr.fit((9, 24), (24, 20))))
        for filter in gr.FILTERS:
            cases.append(_case(one, crops, (24, 20), k, "f16", "rgb", filter))
    # pad values at the u8 ties and clamps, and beyond f16
    for filter in ("bilinear", "antialias"):
        for pad in ((0.5, 1.5, 2.5), (-3.0, 300.0, 254.5)):
            cases.append(_case(one, ((0, None, (5, 3, 21, 9)),), (33, 17), 1, "u8", "rgb", filter, pad=pad, params=gr.IDENTITY))
        cases.append(_case(one, ((0, None, (5, 3, 21, 9)),), (33, 17), 1, "f16", "bgr", filter, pad=(70000.0, -70000.0, 65519.0), params=gr.IDENTITY))
    return cases


CASES = _cases()


def _rect(r):
    return "w" if r is None else "%d.%d.%d.%d" % r


def _id(c):
    images = "+".join(f"{w}x{h}" for w, h, _ in c["images"])
    regions = "+".join(f"{i}s{_rect(s)}d{_rect(d)}" for i, s, d in c["regions"]) if len(c["regions"]) < 3 else f"{len(c['regions'])}regions"
    pad = "pad" + ".".join("%g" % p for p in c["pad"])
    return f"{images}-{regions}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['filter']}-{c['dtype']}-{c['order']}-{pad}-at{c['offset']}"


_frames = {}


def _rgba(w, h, seed):
    if (w, h, seed) not in _frames:
        _frames[(w, h, seed)] = gr.frame(w, h, seed=seed)[1]
    return _frames[(w, h, seed)]


def _allocation(w, h, seed):
    """(pitch, rows, bytes) of one image as the runtime allocates it."""
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    alloc = np.full((rows, pitch), PAD_BYTE, dtype=np.uint8)
    alloc[:h, :w * 4] = _rgba(w, h, seed).reshape(h, w * 4)
    return pitch, rows, alloc.tobytes()


def _needed(c):
    return len(c["regions"]) * 3 * c["size"][1] * c["size"][0] * gr.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_region")
    exe = str(tmp / "region_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_region", "region_driver.cpp"), "-o", exe])
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
        blob.append(struct.pack("<8I9f2I", len(c["regions"]), len(c["images"]), c["k"], gr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                FILTER[c["filter"]], ow, oh, *c["scale"], *c["bias"], *c["pad"], c["offset"], total))
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
    got = gr.from_bytes(buf[lo:hi], c["dtype"], (len(c["regions"]), 3, oh, ow))
    for r, (image, src, dst) in enumerate(c["regions"]):
        w, h, seed = c["images"][image]
        want = gr.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["filter"], src, dst, c["pad"])
        assert gr.same(got[r], want, c["dtype"]), f"region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"
    if c["axes"] is not None:
        assert axes == c["axes"], f"the launch built {axes} axis tables"


@pytest.mark.parametrize("filter, most", [("nearest", 2048), ("bilinear", 2048), ("antialias", 128)])
def test_the_planner_refuses_a_grid_that_does_not_fit(driver, filter, most):
    """65535 x 65535 in u8: a slot is 1 048 560 workgroups of 256 runs, antialiased 16 776 705 of 256 elements; 2^31 - 1
    workgroups is the limit.  (tests/gpu_region_worker.py asks the library for 4096 such slots and expects the rejection:
    this is why nothing is launched there.)"""
    def fits(slots):
        r = subprocess.run([driver[1], "--plan", str(FILTER[filter]), "0", "65535", "65535", str(slots)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip()
    assert fits(1) == "fits 1" and fits(most) == "fits 1"
    assert fits(most + 1) == "fits 0" and fits(4096) == "fits 0"
