"""The pack_tensor kernels' lane body (compeg_amd/csrc/tensor_body.h) on the CPU: tests/emul_tensor/pack_driver.cpp,
compiled with g++ -fsanitize=address,undefined, plans every launch like the library and runs its grid lane by lane
over an RGBA image laid out as the runtime allocates it -- rows and pitch padded to 16 pixels, the padding filled
with 0xA5 so that a padding byte that leaks into a sum shows.  The destination lies one element into a larger
buffer (rows, planes and images then begin at every alignment) between sentinel bytes that must survive; a few
cases lie at an aligned address as well, where whole runs leave as 16-byte stores."""
import os
import struct
import subprocess

import numpy as np
import pytest

import numeric_edges as ne
import tensor_reference as tr
from conftest import ROOT

SIZES = ((16, 8), (17, 9), (50, 26), (330, 70), (7, 5))
SENTINEL = 0x5C
PAD = 0xA5


def _cases():
    cases, n = [], 0
    for w, h in SIZES:
        for k in tr.ks_for(w, h):
            for dtype in tr.DTYPES:
                n += 1
                identity = dtype == "u8" and k == tr.ks_for(w, h)[0]   # (one u8 case per size: the RGB planes themselves)
                scale, bias = tr.IDENTITY if identity else ((tr.U8_SCALE, tr.U8_BIAS) if dtype == "u8" else (tr.IMAGENET_SCALE, tr.IMAGENET_BIAS))
                cases.append(dict(w=w, h=h, k=k, dtype=dtype, order=("rgb", "bgr")[n % 2], scale=scale, bias=bias, images=1,
                                  offset=64 + tr.ELEM_BYTES[dtype]))
    # a three-image batch whose planes have 325 elements
    for dtype in tr.DTYPES:
        cases.append(dict(w=50, h=26, k=2, dtype=dtype, order="rgb", scale=tr.IMAGENET_SCALE, bias=tr.IMAGENET_BIAS, images=3,
                          offset=64 + tr.ELEM_BYTES[dtype]))
    # at an aligned address: rows of whole 16-byte runs (16x8, 330x70 at k = 1 for u8: 320 + 10) and rows that end inside one
    for w, h, k in ((16, 8, 1), (330, 70, 1), (330, 70, 2), (50, 26, 1)):
        for dtype in tr.DTYPES:
            cases.append(dict(w=w, h=h, k=k, dtype=dtype, order="bgr", scale=tr.IMAGENET_SCALE, bias=tr.IMAGENET_BIAS, images=2, offset=64))
    # the numeric edges (tests/numeric_edges.py): every set on its frames, aligned and misaligned by one element --
    # the software f16's subnormal, overflow and infinity branches, the u8 clamp on infinities, denormal float32
    for name, dtype in ne.SET_DTYPES:
        _, scale, bias = ne.SETS[name]
        for frame, k in ne.PACKS:
            for offset in (64, 64 + tr.ELEM_BYTES[dtype]):
                n += 1
                w, h = ne.EXTENT[frame]
                cases.append(dict(w=w, h=h, k=k, dtype=dtype, order=("rgb", "bgr")[n % 2], scale=scale, bias=bias, images=1, offset=offset,
                                  frames=(frame,), edge=name))
    return cases


CASES = _cases()


def _id(c):
    edge = f"{c['edge']}-{c['frames'][0]}-" if "edge" in c else ""
    return f"{edge}{c['w']}x{c['h']}-k{c['k']}-{c['dtype']}-{c['order']}-n{c['images']}-at{c['offset']}"


def _source(c):
    """The images' allocations (pitch, rows, bytes) and their RGBA."""
    w, h = c["w"], c["h"]
    pitch, rows = (w + 15) // 16 * 64, (h + 15) // 16 * 16
    if "frames" in c:   # handed in by name (tests/numeric_edges.py)
        frames = [ne.FRAMES[name]()[1] for name in c["frames"]]
        assert len(frames) == c["images"] and all(f.shape == (h, w, 4) for f in frames)
    else:
        frames = [tr.frame(w, h, seed=3 + i)[1] for i in range(c["images"])]
    alloc = np.full((c["images"], rows, pitch), PAD, dtype=np.uint8)
    for i, f in enumerate(frames):
        alloc[i, :h, :w * 4] = f.reshape(h, w * 4)
    return pitch, rows, alloc.tobytes(), frames


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """Every case through one run of the driver: case index -> the destination buffer afterwards."""
    tmp = tmp_path_factory.mktemp("emul_tensor")
    exe = str(tmp / "pack_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "compeg_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emul_tensor", "pack_driver.cpp"), "-o", exe])
    blob, sizes = [struct.pack("<I", len(CASES))], []
    for c in CASES:
        pitch, rows, src, _ = _source(c)
        oh, ow = c["h"] // c["k"], c["w"] // c["k"]
        needed = c["images"] * 3 * oh * ow * tr.ELEM_BYTES[c["dtype"]]
        total = (c["offset"] + needed + 64 + 255) // 256 * 256
        sizes.append((needed, total))
        blob.append(struct.pack("<6I6f4I", c["w"], c["h"], c["images"], c["k"], tr.DTYPES.index(c["dtype"]), ("rgb", "bgr").index(c["order"]),
                                *c["scale"], *c["bias"], pitch, rows, c["offset"], total))
        blob.append(src)
        blob.append(bytes([SENTINEL]) * total)
    (tmp / "in.bin").write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    out, at, result = (tmp / "out.bin").read_bytes(), 0, []
    for needed, total in sizes:
        result.append(out[at:at + total])
        at += total
    assert at == len(out)
    return result


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_lane_body_matches_the_formula_and_stays_inside_the_tensor(packed, index):
    c, buf = CASES[index], packed[index]
    oh, ow = c["h"] // c["k"], c["w"] // c["k"]
    needed = c["images"] * 3 * oh * ow * tr.ELEM_BYTES[c["dtype"]]
    lo, hi = c["offset"], c["offset"] + needed
    assert buf[:lo] == bytes([SENTINEL]) * lo, "bytes in front of the tensor were written"
    assert buf[hi:] == bytes([SENTINEL]) * (len(buf) - hi), "bytes behind the tensor were written"
    got = tr.from_bytes(buf[lo:hi], c["dtype"], (c["images"], 3, oh, ow))
    frames = _source(c)[3]
    for i, f in enumerate(frames):
        with np.errstate(over="ignore"):   # (the edge sets overflow to infinity on purpose)
            want = tr.expected(f, c["k"], c["dtype"], c["scale"], c["bias"], c["order"])
        assert tr.same(got[i], want, c["dtype"]), f"image {i}: {int((got[i] != want).sum())} of {want.size} elements differ"


def test_identity_u8_is_the_oracles_planes():
    """(the reference helper itself) k = 1, scale 1, bias 0, u8: the R, G and B planes byte for byte."""
    rgba = tr.frame(50, 26)[1]
    want = tr.expected(rgba, 1, "u8", *tr.IDENTITY)
    assert np.array_equal(want, rgba[..., :3].transpose(2, 0, 1))
    assert np.array_equal(tr.expected(rgba, 1, "u8", *tr.IDENTITY, order="bgr"), rgba[..., 2::-1].transpose(2, 0, 1))
