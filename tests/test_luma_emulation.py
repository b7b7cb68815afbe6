"""The luma_tensor kernels' lane body (compeg_amd/csrc/luma_body.h) on the CPU: tests/emul_luma/luma_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and the flags of tests/test_nhwc_emulation.py, plans
every launch with the library's planners -- dst', records, axis tables, grid -- and runs its grid lane by lane over RGBA
images laid out as the runtime allocates them (test_orient_emulation's _allocation: rows and pitch padded to 16 pixels, the
padding filled with 0xA5), every image, the records with their tables and the one pad value heap blocks of their own so
that a load outside them is the sanitizer's to report.  Nothing is loaded into Python under a sanitizer.  The destination
lies one element into a larger buffer between sentinel bytes that must survive, and is itself filled with the sentinel:
an element that no lane writes shows too.  Every element is compared with tests/luma_reference.py, bit for bit, with bands
of 8 rows (what the library compiles) and of 3."""
import os
import struct
import subprocess

import numpy as np
import pytest

import luma_reference as lr
import test_orient_emulation as oe   # (as a module: its tests are not collected a second time)
from conftest import ROOT

orf, fr = lr.orf, lr.fr
SENTINEL = oe.SENTINEL
WEIGHTS = tuple(lr.PRESETS)
WHITE = 99   # the seed that stands for the all-255 image


def _case(images, regions, size, k, dtype, kernel, weights="bt601", pad=114.0, params=None, band=8, order="rgb"):
    """images: ((w, h, seed), ...); regions: ((image, src or None, dst or None, orientation), ...).  scale and bias are
    triples of which the kernels read element 0; the others and the order are there to have no effect."""
    scale, bias = params or fr.params(dtype)
    return dict(images=tuple(images), regions=tuple(regions), size=size, k=k, dtype=dtype, order=order, kernel=kernel, weights=weights,
                pad=pad, scale=scale, bias=bias, band=band, offset=64 + fr.ELEM_BYTES[dtype])


def _cases():
    cases, n = [], 0
    imagenet = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    # every orientation x element type x k on the portrait's letterbox (where its preimage lies within the tap limit)
    for o in orf.ORIENTATIONS:
        for dtype in fr.DTYPES:
            for k in (1, 2, 4, 8):
                n += 1
                c = _case(oe.ONE, ((0, None, oe.PORTRAIT, o),), (48, 40), k, dtype, "bicubic", ("bt601", "bt709")[n % 2],
                          pad=(114.0, 250.5)[n // 2 % 2], band=(8, 3)[(n // 4) % 2], order=("rgb", "bgr")[n // 8 % 2])
                if oe.fits(c, *c["regions"][0]):
                    cases.append(c)
    # the list EIGHT over five images, every kernel and element type
    for kn, kernel in enumerate(fr.KERNELS):
        for d, dtype in enumerate(fr.DTYPES):
            cases.append(_case(oe.FIVE, orf.EIGHT, orf.SLOT, 1, dtype, kernel, WEIGHTS[(kn + d) % 5], band=(8, 3)[(kn + d) % 2],
                               params=imagenet if dtype != "u8" else None))
        cases.append(_case(oe.FIVE, orf.EIGHT, orf.SLOT, 2, "f16", kernel, order="bgr"))
    # run edges: the transposing orientations write runs along U's rows, ow elements long
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f16", "f32"):
                cases.append(_case(((17, 9, 6),), ((0, None, None, o),), (ow, 5), 1, dtype, "bicubic", band=(8, 3)[ow % 2]))
        # ... an inner rectangle that begins at dx and ends a band early, pad in front of it and behind it in the row
        for band in (8, 3):
            for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
                for dtype in ("u8", "f32", "bf16"):
                    cases.append(_case(((17, 9, 6),), ((0, (1, 0, 15, 9), (dx, 1, dw, 3), o),), (13, 5), 1, dtype, "triangle", "bt709", band=band))
    # the same rectangles under the orientations that do not transpose
    for o in (1, 2, 3, 4):
        for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
            cases.append(_case(((17, 9, 6),), ((0, (1, 0, 15, 9), (dx, 1, dw, 3), o),), (13, 5), 1, ("u8", "f16")[dx % 2], "triangle", band=(8, 3)[o % 2]))
    # 257 columns of T: more than one workgroup a band
    cases.append(_case(oe.ONE, ((0, None, (2, 0, 9, 257), 6),), (11, 257), 1, "u8", "bicubic"))
    cases.append(_case(oe.ONE, ((0, None, None, 8), (0, None, (0, 2, 257, 9), 3)), (257, 11), 1, "f16", "box", "bt709"))
    # each preset and B alone given as numbers, at k = 1 (four taps a step and the rest) and k = 2
    for weights in WEIGHTS + ((0, 0, 65536), (1, 65534, 1)):
        for k in (1, 2):
            cases.append(_case(((50, 26, 5),), ((0, None, None, 1), (0, (3, 1, 45, 21), (1, 3, 11, 13), 5)), (24, 20), k, "f32", "bicubic", weights,
                               params=imagenet))
    # an all-255 image at k = 8: the block sum is 16320, L never passes 255
    for dtype in ("u8", "f32"):
        cases.append(_case(((64, 48, WHITE),), ((0, None, None, 1), (0, None, None, 6)), (8, 6) if dtype == "u8" else (5, 4), 8, dtype, "box", "bt601",
                           params=fr.IDENTITY))
    return cases


CASES = _cases()


def _rgba(w, h, seed):
    if seed == WHITE:
        return np.full((h, w, 4), 255, np.uint8)
    return oe._rgba(w, h, seed)


def _allocation(w, h, seed):
    """(pitch, rows, bytes) of one image as the runtime allocates it (test_orient_emulation's, for the white image too)."""
    if seed != WHITE:
        return oe._allocation(w, h, seed)
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    alloc = np.full((rows, pitch), oe.PAD_BYTE, dtype=np.uint8)
    alloc[:h, :w * 4] = 255
    return pitch, rows, alloc.tobytes()


def _id(c):
    images = "+".join(f"{w}x{h}" for w, h, _ in c["images"])
    regions = "+".join(f"{i}s{oe._rect(s)}d{oe._rect(d)}o{o}" for i, s, d, o in c["regions"]) if len(c["regions"]) < 3 else f"{len(c['regions'])}regions"
    weights = c["weights"] if isinstance(c["weights"], str) else ".".join(str(w) for w in c["weights"])
    return (f"{images}-{regions}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['kernel']}-{c['dtype']}-{c['order']}-{weights}-pad{c['pad']:g}"
            f"-band{c['band']}")


def _needed(c):
    return len(c["regions"]) * c["size"][1] * c["size"][0] * fr.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through one run of the driver: case index -> the destination buffer afterwards."""
    tmp = tmp_path_factory.mktemp("emul_luma")
    exe = str(tmp / "luma_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_luma", "luma_driver.cpp"), "-o", exe])
    blob, totals = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        total = (c["offset"] + _needed(c) + 64 + 255) // 256 * 256
        totals.append(total)
        ow, oh = c["size"]
        blob.append(struct.pack("<12I7f2I", len(c["regions"]), len(c["images"]), c["k"], fr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                fr.KERNELS.index(c["kernel"]), ow, oh, c["band"], *lr.weights_of(c["weights"]), *c["scale"], *c["bias"], c["pad"],
                                c["offset"], total))
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
        result.append(out[at:at + total])
        at += total
    assert at == len(out)
    return result


def test_the_cases_cover_what_they_are_meant_to():
    letterbox = [c for c in CASES if c["size"] == (48, 40)]
    assert {c["regions"][0][3] for c in letterbox} == set(orf.ORIENTATIONS)
    for transposing in (False, True):
        seen = {(c["dtype"], c["k"]) for c in letterbox if (c["regions"][0][3] >= 5) == transposing}
        # (1..4 take 330 samples into 8 outputs: bicubic admits that from k = 2 on)
        assert seen == {(d, k) for d in fr.DTYPES for k in ((1, 2, 4, 8) if transposing else (2, 4, 8))}
    assert {c["weights"] for c in letterbox} == {"bt601", "bt709"} and {c["order"] for c in letterbox} == {"rgb", "bgr"}
    eight = [c for c in CASES if c["regions"] == orf.EIGHT]
    assert {(c["kernel"], c["dtype"]) for c in eight} == {(kn, d) for kn in fr.KERNELS for d in fr.DTYPES}
    assert all(oe.fits(c, *r) for c in eight for r in c["regions"])
    edges = [c for c in CASES if c["size"][1] == 5 and c["regions"][0][1] is None and len(c["regions"]) == 1]
    assert {(c["regions"][0][3], c["size"][0], c["dtype"]) for c in edges} == {
        (o, ow, d) for o in (5, 6, 7, 8) for ow in (1, 7, 8, 9, 13) for d in ("u8", "f16", "f32")}
    assert {c["band"] for c in CASES} == {8, 3} and all(c["offset"] == 64 + fr.ELEM_BYTES[c["dtype"]] for c in CASES)
    assert set(WEIGHTS) | {(0, 0, 65536)} <= {c["weights"] for c in CASES}
    assert any(c["images"][0][2] == WHITE and c["k"] == 8 for c in CASES)
    # scale[1..2] and bias[1..2] differ from element 0 somewhere: were they read, it would show
    assert any(len(set(c["scale"])) == 3 and len(set(c["bias"])) == 3 for c in CASES)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_bodies_match_the_contract_and_stay_inside_the_tensor(packed, index):
    c, buf = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = fr.from_bytes(buf[lo:hi], c["dtype"], (len(c["regions"]), oh, ow))
    for r, (image, src, dst, o) in enumerate(c["regions"]):
        w, h, seed = c["images"][image]
        want = lr.expected(_rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"][0], c["bias"][0], c["weights"], c["kernel"], src, dst,
                           c["pad"], o)
        assert fr.same(got[r], want, c["dtype"]), f"region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"
        if c["images"][image][2] == WHITE and c["scale"][0] == 1.0 and c["bias"][0] == 0.0:
            assert (got[r] == 255).all()
