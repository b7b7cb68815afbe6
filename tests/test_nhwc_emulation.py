"""The nhwc_tensor kernels' lane body (compeg_amd/csrc/nhwc_body.h) on the CPU: tests/emul_nhwc/nhwc_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and the flags of tests/test_orient_emulation.py, plans
every launch with the library's planners -- dst', records, axis tables, grid -- and runs its grid lane by lane over RGBA
images laid out as the runtime allocates them (that module's _allocation: rows and pitch padded to 16 pixels, the padding
filled with 0xA5), every image and the records with their tables heap blocks of their own so that a load outside them is
the sanitizer's to report.  The destination lies one element into a larger buffer between sentinel bytes that must
survive, and is itself filled with the sentinel: an element that no lane writes shows too.  Every element is compared
with tests/nhwc_reference.py, bit for bit, with bands of 8 rows (what the library compiles) and of 3."""
import os
import struct
import subprocess

import pytest

import nhwc_reference as nr
import test_orient_emulation as oe   # (as a module: its tests are not collected a second time)
from conftest import ROOT

orf, fr = nr.orf, nr.fr
SENTINEL = oe.SENTINEL
FILL = {"u8": 127.5, "f16": 0.1, "bf16": 0.1, "f32": 0.1}   # a tie in u8 (128); rounds in f16 and bf16


def _case(images, regions, size, k, dtype, order, kernel, channels, fill=None, pad=oe.COLOURS, params=None, band=8):
    """images: ((w, h, seed), ...); regions: ((image, src or None, dst or None, orientation), ...)"""
    scale, bias = params or fr.params(dtype)
    return dict(images=tuple(images), regions=tuple(regions), size=size, k=k, dtype=dtype, order=order, kernel=kernel, channels=channels,
                fill=FILL[dtype] if fill is None else fill, pad=pad, scale=scale, bias=bias, band=band, offset=64 + fr.ELEM_BYTES[dtype])


def _cases():
    cases, n = [], 0
    imagenet = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    # every orientation x element type x k x C on the portrait's letterbox (where its preimage lies within the tap limit)
    for o in orf.ORIENTATIONS:
        for dtype in fr.DTYPES:
            for k in (1, 2, 4, 8):
                for channels in nr.CHANNELS:
                    n += 1
                    c = _case(oe.ONE, ((0, None, oe.PORTRAIT, o),), (48, 40), k, dtype, ("rgb", "bgr")[n // 2 % 2], "bicubic", channels,
                              pad=oe.GREY if n % 3 else oe.COLOURS, band=(8, 3)[(n // 4) % 2])
                    if oe.fits(c, *c["regions"][0]):
                        cases.append(c)
    # the list EIGHT over five images, every kernel and element type
    for kn, kernel in enumerate(fr.KERNELS):
        for d, dtype in enumerate(fr.DTYPES):
            cases.append(_case(oe.FIVE, orf.EIGHT, orf.SLOT, 1, dtype, ("rgb", "bgr")[d % 2], kernel, nr.CHANNELS[(kn + d // 2) % 2], band=(8, 3)[(kn + d) % 2],
                               params=imagenet if dtype != "u8" else None))
        cases.append(_case(oe.FIVE, orf.EIGHT, orf.SLOT, 2, "f16", "bgr", kernel, nr.CHANNELS[kn % 2]))
    # run edges: the transposing orientations write runs along U's rows, ow pixels long
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f16", "f32"):
                for channels in nr.CHANNELS:
                    cases.append(_case(((17, 9, 6),), ((0, None, None, o),), (ow, 5), 1, dtype, "rgb", "bicubic", channels, band=(8, 3)[ow % 2]))
        # ... an inner rectangle that begins at dx and ends a band early, pad in front of it and behind it in the row
        for band in (8, 3):
            for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
                for d, dtype in enumerate(("u8", "f32", "bf16")):
                    cases.append(_case(((17, 9, 6),), ((0, (1, 0, 15, 9), (dx, 1, dw, 3), o),), (13, 5), 1, dtype, "bgr", "triangle",
                                       nr.CHANNELS[(d + dx + band) % 2], band=band))
    # the same rectangles under the orientations that do not transpose: pad pixels carry the fill as well
    for o in (1, 2, 3, 4):
        for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
            cases.append(_case(((17, 9, 6),), ((0, (1, 0, 15, 9), (dx, 1, dw, 3), o),), (13, 5), 1, ("u8", "f16")[dx % 2], "bgr", "triangle", 4,
                               band=(8, 3)[o % 2]))
    # 257 columns of T: more than one workgroup a band
    cases.append(_case(oe.ONE, ((0, None, (2, 0, 9, 257), 6),), (11, 257), 1, "u8", "rgb", "bicubic", 3))
    cases.append(_case(oe.ONE, ((0, None, None, 8), (0, None, (0, 2, 257, 9), 3)), (257, 11), 1, "f16", "rgb", "box", 4))
    # fills that need rounding: ties in u8, beyond its range either way, values f16 and bf16 do not hold (2049: a tie, to 2048)
    for dtype, fill in (("u8", 127.5), ("u8", 126.5), ("u8", 300.0), ("u8", -2.0), ("f16", 0.1), ("f16", 2049.0), ("bf16", 1.01171875), ("f32", 0.1)):
        cases.append(_case(((17, 9, 6),), ((0, None, (1, 0, 5, 4), 1), (0, None, (1, 0, 5, 4), 7)), (7, 5), 1, dtype, "rgb", "triangle", 4, fill=fill))
    return cases


CASES = _cases()


def _id(c):
    images = "+".join(f"{w}x{h}" for w, h, _ in c["images"])
    regions = "+".join(f"{i}s{oe._rect(s)}d{oe._rect(d)}o{o}" for i, s, d, o in c["regions"]) if len(c["regions"]) < 3 else f"{len(c['regions'])}regions"
    return (f"{images}-{regions}-to{c['size'][0]}x{c['size'][1]}-k{c['k']}-{c['kernel']}-{c['dtype']}-{c['order']}-c{c['channels']}-fill{c['fill']:g}"
            f"-pad{'.'.join('%g' % p for p in c['pad'])}-band{c['band']}")


def _needed(c):
    return len(c["regions"]) * c["size"][1] * c["size"][0] * c["channels"] * fr.ELEM_BYTES[c["dtype"]]


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through one run of the driver: case index -> the destination buffer afterwards."""
    tmp = tmp_path_factory.mktemp("emul_nhwc")
    exe = str(tmp / "nhwc_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_nhwc", "nhwc_driver.cpp"), "-o", exe])
    blob, totals = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        total = (c["offset"] + _needed(c) + 64 + 255) // 256 * 256
        totals.append(total)
        ow, oh = c["size"]
        blob.append(struct.pack("<10I10f2I", len(c["regions"]), len(c["images"]), c["k"], fr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                fr.KERNELS.index(c["kernel"]), ow, oh, c["band"], c["channels"], c["fill"], *c["scale"], *c["bias"], *c["pad"],
                                c["offset"], total))
        sources = []
        for w, h, seed in c["images"]:
            pitch, rows, raw = oe._allocation(w, h, seed)
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
    assert {(c["regions"][0][3], c["channels"]) for c in letterbox} == {(o, ch) for o in orf.ORIENTATIONS for ch in nr.CHANNELS}
    for transposing in (False, True):
        seen = {(c["dtype"], c["k"], c["channels"]) for c in letterbox if (c["regions"][0][3] >= 5) == transposing}
        # (1..4 take 330 samples into 8 outputs: bicubic admits that from k = 2 on)
        assert seen == {(d, k, ch) for d in fr.DTYPES for k in ((1, 2, 4, 8) if transposing else (2, 4, 8)) for ch in nr.CHANNELS}
    eight = [c for c in CASES if c["regions"] == orf.EIGHT]
    assert {(c["kernel"], c["channels"]) for c in eight} == {(kn, ch) for kn in fr.KERNELS for ch in nr.CHANNELS}
    assert all(oe.fits(c, *r) for c in eight for r in c["regions"])
    edges = [c for c in CASES if c["size"][1] == 5 and c["regions"][0][1] is None and len(c["regions"]) == 1]
    assert {(c["regions"][0][3], c["size"][0], c["dtype"], c["channels"]) for c in edges} == {
        (o, ow, d, ch) for o in (5, 6, 7, 8) for ow in (1, 7, 8, 9, 13) for d in ("u8", "f16", "f32") for ch in nr.CHANNELS}
    assert {c["band"] for c in CASES} == {8, 3} and all(c["offset"] == 64 + fr.ELEM_BYTES[c["dtype"]] for c in CASES)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_bodies_match_the_contract_and_stay_inside_the_tensor(packed, index):
    c, buf = CASES[index], packed[index]
    ow, oh = c["size"]
    lo, hi = c["offset"], c["offset"] + _needed(c)
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = fr.from_bytes(buf[lo:hi], c["dtype"], (len(c["regions"]), oh, ow, c["channels"]))
    for r, (image, src, dst, o) in enumerate(c["regions"]):
        w, h, seed = c["images"][image]
        want = nr.expected(oe._rgba(w, h, seed), c["size"], c["k"], c["dtype"], c["scale"], c["bias"], c["order"], c["kernel"], src, dst, c["pad"], o,
                           c["channels"], c["fill"])
        assert fr.same(got[r], want, c["dtype"]), f"region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"
