"""The orient_tensor kernels' lane body (compeg_amd/csrc/orient_body.h) on the CPU: tests/emul_orient/orient_driver.cpp,
a stand-alone program compiled with g++ -fsanitize=address,undefined and the flags of tests/test_filter_emulation.py,
plans every launch with the library's planners -- dst', records, axis tables, grid -- and runs its grid lane by lane over
RGBA images laid out as the runtime allocates them: rows and pitch padded to 16 pixels, the padding filled with 0xA5,
every image and the records with their tables heap blocks of their own so that a load outside them is the sanitizer's to
report.  The destination lies one element into a larger buffer between sentinel bytes that must survive, and is itself
filled with the sentinel: an element that no lane writes shows too.  Every element is compared with
tests/orient_reference.py, bit for bit, with bands of 8 rows (what the library compiles) and of 3."""
import os
import struct
import subprocess

import pytest

import numpy as np

import orient_reference as orf
from conftest import ROOT

fr = orf.fr
SENTINEL = 0x5C
PAD_BYTE = 0xA5
GREY = (114.0, 114.0, 114.0)
COLOURS = (10.0, 114.0, 250.5)   # one value per channel: a plane that takes the wrong one shows
FIVE = tuple((w, h, 20 + i) for i, (w, h) in enumerate(fr.gr.FIVE))
ONE = ((330, 70, 3),)
PORTRAIT = fr.fit((70, 330), (48, 40))   # the 330x70 frame at orientation 6 is 70x330 upright: (20, 0, 8, 40)


def fits(c, image, src, dst, o):
    """Whether the region lies within the kernel's tap limit, against T's axes."""
    w, h, _ = c["images"][image]
    sw, sh = (src[2], src[3]) if src is not None else (w, h)
    _, _, dw, dh = orf.preimage(dst if dst is not None else (0, 0) + c["size"], o, c["size"])
    return fr.axis_ok(c["kernel"], sw // c["k"], dw) and fr.axis_ok(c["kernel"], sh // c["k"], dh)


def _case(images, regions, size, k, dtype, order, kernel, pad=COLOURS, params=None, offset=None, band=8):
    """images: ((w, h, seed), ...); regions: ((image, src or None, dst or None, orientation), ...)"""
    scale, bias = params or fr.params(dtype)
    return dict(images=tuple(images), regions=tuple(regions), size=size, k=k, dtype=dtype, order=order, kernel=kernel, pad=pad, scale=scale,
                bias=bias, band=band, offset=64 + fr.ELEM_BYTES[dtype] if offset is None else offset)


def _cases():
    cases, n = [], 0
    imagenet = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    # every orientation x element type x k on the portrait's letterbox (where its preimage fits: at k = 1 bicubic takes
    # 330 samples into 40 outputs, not into 8)
    for o in orf.ORIENTATIONS:
        for dtype in fr.DTYPES:
            for k in (1, 2, 4, 8):
                n += 1
                c = _case(ONE, ((0, None, PORTRAIT, o),), (48, 40), k, dtype, ("rgb", "bgr")[n % 2], "bicubic", pad=GREY if n % 3 else COLOURS,
                          band=(8, 3)[(n // 2) % 2])
                if fits(c, *c["regions"][0]):
                    cases.append(c)
    # the list EIGHT over five images, every kernel and element type
    for kn, kernel in enumerate(fr.KERNELS):
        for d, dtype in enumerate(fr.DTYPES):
            cases.append(_case(FIVE, orf.EIGHT, orf.SLOT, 1, dtype, ("rgb", "bgr")[d % 2], kernel, band=(8, 3)[(kn + d) % 2],
                               params=imagenet if dtype != "u8" else None))
        cases.append(_case(FIVE, orf.EIGHT, orf.SLOT, 2, "f16", "bgr", kernel, offset=64))
    # run edges: the transposing orientations write runs along U's rows, ow elements long
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f16", "f32"):
                cases.append(_case(((17, 9, 6),), ((0, None, None, o),), (ow, 5), 1, dtype, "rgb", "bicubic", band=(8, 3)[ow % 2]))
        # ... an inner rectangle that begins at dx and ends a band early, pad in front of it and behind it in the row
        for band in (8, 3):
            for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
                for dtype in ("u8", "f32", "bf16"):
                    cases.append(_case(((17, 9, 6),), ((0, (1, 0, 15, 9), (dx, 1, dw, 3), o),), (13, 5), 1, dtype, "bgr", "triangle", band=band,
                                       offset=64 + (3 if dtype == "u8" else 4)))
    # every orientation of one frame, whole, into an odd slot, the ImageNet pair
    for o in orf.ORIENTATIONS:
        cases.append(_case(ONE, ((0, None, None, o),), (31, 13) if o < 5 else (13, 31), 1, "f32", ("rgb", "bgr")[o % 2], "bicubic", params=imagenet))
    # 257 columns of T: more than one workgroup a band
    cases.append(_case(ONE, ((0, None, (2, 0, 9, 257), 6),), (11, 257), 1, "u8", "rgb", "bicubic"))
    cases.append(_case(ONE, ((0, None, None, 8), (0, None, (0, 2, 257, 9), 3)), (257, 11), 1, "f16", "rgb", "box"))
    return cases


CASES = _cases()


def _rect(r):
    return "w" if r is None else "%d.%d.%d.%d" % r


def _id(c):
    images = "+".join(f"{w}x{h}" for w, h, _ in c["images"])
    regions = "+".join(f"{i}s{_rect(s)}d{_rect(d)}o{o}" for i, s, d, o in c["regions"]) if len(c["regions"]) < 3 else f"{len(c['regions'])}regions"
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
    tmp = tmp_path_factory.mktemp("emul_orient")
    exe = str(tmp / "orient_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_orient", "orient_driver.cpp"), "-o", exe])
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
        for image, src, dst, o in c["regions"]:
            w, h, _ = c["images"][image]
            blob.append(struct.pack("<10I", image, *(src if src is not None else (0, 0, w, h)), *(dst if dst is not None else (0, 0, ow, oh)), o))
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


def test_the_cases_cover_what_they_are_meant_to():
    letterbox = [c for c in CASES if c["size"] == (48, 40)]
    assert {c["regions"][0][3] for c in letterbox} == set(orf.ORIENTATIONS)
    assert {(c["dtype"], c["k"]) for c in letterbox if c["regions"][0][3] >= 5} == {(d, k) for d in fr.DTYPES for k in (1, 2, 4, 8)}
    # EIGHT lies within every kernel's limit at k = 1 and k = 2, and its rectangles in T are the ones the design counts on
    for c in CASES:
        if c["regions"] == orf.EIGHT:
            assert all(fits(c, *r) for r in c["regions"])
    turned = [orf.preimage(dst, o, orf.SLOT) for _, _, dst, o in orf.EIGHT]
    assert [t[1] for t in turned] == [4, 3, 8, 0, 1, 2, 0, 0] and [t[3] for t in turned] == [6, 11, 5, 20, 11, 20, 1, 24]


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_bodies_match_the_contract_and_stay_inside_the_tensor(packed, index):
    c, (buf, _) = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = fr.from_bytes(buf[lo:hi], c["dtype"], (len(c["regions"]), 3, oh, ow))
    for r, (image, src, dst, o) in enumerate(c["regions"]):
        w, h, seed = c["images"][image]
        want = orf.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["kernel"], src, dst, c["pad"], o)
        assert fr.same(got[r], want, c["dtype"]), f"region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"


SANITIZE = ["-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_the_parser_reads_nothing_beyond_a_mutated_or_cut_exif_segment(tmp_path):
    """tests/emul_orient/exif_driver.cpp: front.cpp under ASan/UBSan, a stand-alone program; every byte of the APP1 payload
    set to 0x00, 0xFF and a seeded value, the file cut at every length inside the segment.  CPU only."""
    from tools import synth
    exe = str(tmp_path / "exif_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", *SANITIZE, "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "emul_orient", "exif_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), "-o", exe])
    frame = synth.make_jpeg(48, 32, seed=11)
    for n, segment in enumerate((orf.exif_app1(6, True, "last"), orf.exif_app1(8, False, "first"), orf.exif_app1(3, True, "only"))):
        path = tmp_path / f"spliced{n}.jpg"
        path.write_bytes(orf.splice(frame, segment))
        r = subprocess.run([exe, str(path), "2", str(n + 1)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-6000:]
        assert int(r.stdout.split()[1]) == 1 + 3 * (len(segment) - 4) + len(segment) + 1


def test_the_planner_sizes_a_slot_by_the_shapes_the_call_needs(driver):
    """16 x 4096 upright: 513 bands of 16 lanes, 33 workgroups; transposed 3 bands of 4096 lanes, 48 workgroups.  2^31 - 1
    workgroups is the limit: 44 739 242 slots of 48 meet it, one more does not -- unless no slot is transposed."""
    def plan(slots, upright, transposed):
        r = subprocess.run([driver[1], "--plan", "2", "0", "16", "4096", str(slots), str(upright), str(transposed)], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip()
    assert plan(44739242, 1, 1) == "fits 1" and plan(44739242, 0, 1) == "fits 1"
    assert plan(44739243, 1, 1) == "fits 0" and plan(44739243, 0, 1) == "fits 0"
    assert plan(44739243, 1, 0) == "fits 1" and plan(0, 1, 0) == "fits 0"
