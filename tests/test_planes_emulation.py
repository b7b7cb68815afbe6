"""The planes kernels' lane body (compeg_amd/csrc/planes_body.h) on the CPU: tests/emul_planes/planes_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and run directly (nothing is loaded into Python, nothing
preloaded), drives it lane by lane over exact-size heap copies of words, start positions and LUTs and an "LDS" filled with
0xA5.  Every sampling x every format it takes; destinations tight with odd extents (unaligned pitches, and a base one byte
behind a 16-byte boundary) and pitched (aligned: the vector stores); windows of 300 words and of 8, which cuts every wave's
intervals.  The destination lies between sentinels and over a pre-fill: the pitch padding, the rows below the extents, the
MCUs behind the last complete interval and the sentinels must survive.  Every byte equals tests/planes_stream.py."""
import os
import subprocess

import numpy as np
import pytest

import coef_stream as cs
import planes_stream as ps
import wide_emul as we
from conftest import ROOT

SENTINEL, PREFILL, GUARD = 0x5C, 0x3C, 256
FORMATS_OF = {"422": (("planar", "coded"), ("semiplanar", "coded"), ("yuyv", "coded"), ("uyvy", "coded"), ("planar", "420"), ("semiplanar", "420")),
              "444": (("planar", "coded"), ("semiplanar", "coded")), "440": (("planar", "coded"), ("semiplanar", "coded")),
              "420": (("planar", "coded"), ("semiplanar", "coded")), "gray": (("planar", "coded"),)}
# (window words, destination, bytes behind a 16-byte boundary)
VARIANTS = ((300, "tight", 0), (8, "tight", 1), (300, "pitched", 0), (8, "pitched", 0))


def _frames(layout):
    """Three MCUs less a pixel across and three rows of MCUs plus a pixel down (DRI 3); 130 intervals of one MCU: three
    waves; no DRI; and nine MCUs at DRI 4: the ninth is behind the last complete interval."""
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    return [ps.sized(layout, 3 * mw - 1, 2 * mh + 1, 3), ps.sized(layout, 10 * mw - 3, 13 * mh - 5, 1, standard=True, seed=5),
            ps.sized(layout, 2 * mw + 1, mh, 0, seed=9), ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_planes")
    exe = str(tmp / "planes_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_planes", "planes_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


def _pitch(f, format, chroma, destination):
    if destination == "tight":
        return None
    comps, hs, vs = ps.sampling_of(f)
    lay, _ = ps.layout(f.w, f.h, comps, hs, vs, format, chroma)
    rows = [p[2] for p in lay]
    return ((rows[0] + 15) // 16 * 16 + 16, (rows[-1] + 15) // 16 * 16 + 32 if len(rows) > 1 else 0)


def _run(driver, tmp_path, f, planes, format, chroma, window, destination, shift, luts=()):
    (tmp_path / "in.jpg").write_bytes(f.jpeg())
    comps, hs, vs = ps.sampling_of(f)
    pitch = _pitch(f, format, chroma, destination)
    lay, total = ps.layout(f.w, f.h, comps, hs, vs, format, chroma, pitch)
    flags = (4 if comps == 1 else 1) | (2 if f.standard else 0)
    args = [driver, str(tmp_path / "in.jpg"), str(tmp_path / "out.bin"), str(flags), "3", str(window), str(ps.FORMATS.index(format)),
            "1" if chroma == "420" else "0", str(shift), str(total), str(len(lay))]
    for off, pt, row, _, rows in lay:
        args += [str(off), str(pt), str(row), str(rows)]
    r = subprocess.run(args + list(luts), capture_output=True, text=True, timeout=120)
    we.note(r.stderr)
    what = f"{f.name}: {format}/{chroma}, window {window}, {destination}, shift {shift}"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    assert r.stdout.split()[1:] == [str(f.w), str(f.h), str(f.intervals), str(f.interval)], what
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + shift + total
    assert (block[:GUARD + shift] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got = block[GUARD + shift:-GUARD]
    want = ps.destination(planes, f.w, f.h, comps, hs, vs, format, chroma, pitch, before=np.full(total, PREFILL, dtype=np.uint8))
    bad = np.flatnonzero(got != want)
    if "beyond" in luts:
        return bad.size   # (the control: the caller says what it expects)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_lane_body_on_every_sampling_and_format(driver, tmp_path, layout):
    import compeg_amd as ca   # (the host front end: no device is opened)
    for f in _frames(layout):
        # (MCUs behind the last complete interval: the file's scan has a segment more than the header's count, and what
        # the reference makes of that is the oracle's to say, not cs.predict's)
        planes = ps.file_planes(ca, f.jpeg(), **f.image_kw())[0] if "/short" in f.name else ps.frame_planes(f)
        for format, chroma in FORMATS_OF[layout]:
            for window, destination, shift in VARIANTS:
                _run(driver, tmp_path, f, planes, format, chroma, window, destination, shift)


@pytest.mark.parametrize("name", ["q1_underflow/long/422/reference/dri2", "dc_hostile/own/422/reference/dri2", "positions/short/422/reference/dri4",
                                  "positions/long/422/standard/dri4", "dc_wrap/short/422/reference", "q1_underflow/long/420/reference/dri2",
                                  "dc_hostile/own/444/reference/dri2", "dc_wrap/short/440/reference"])
def test_lane_body_on_the_families_that_break_readers(driver, tmp_path, name):
    f = cs.case(name)
    planes = ps.frame_planes(f)
    for format, chroma in FORMATS_OF[f.layout][:3]:
        _run(driver, tmp_path, f, planes, format, chroma, 8, "tight", 0)
        _run(driver, tmp_path, f, planes, format, chroma, 300, "pitched", 0)


@pytest.mark.parametrize("name", [f.name for f in we.frames()])
def test_lane_body_on_tables_beyond_the_lds_share(driver, tmp_path, name):
    """cs.wide_cases / gs.wide_cases at the planner's budget (tests/emul/lut_budget.h): regime B with the direct tables staged
    in part and the fast mode off, regime C with L2 lookups from global memory beyond entry 12288 -- the driver reports
    what it staged -- and the control: told that everything is staged, every regime-C frame differs from its expectation."""
    f = we.frame(name)
    planes = ps.frame_planes(f)
    for k, (format, chroma) in enumerate(FORMATS_OF[we.layout_of(f)][:2]):
        window, destination, shift = VARIANTS[1 + 2 * k] if k < 2 else VARIANTS[0]
        _run(driver, tmp_path, f, planes, format, chroma, window, destination, shift, luts=we.PLAN)
        we.check_plan(f)
        if we.regime(f) == "C" and k == 0:
            we.check_control(f, _run(driver, tmp_path, f, planes, format, chroma, window, destination, shift, luts=we.BEYOND))


def test_ordinary_tables_decode_in_the_fast_mode(driver, tmp_path):
    f = cs.case("positions/short/422/reference/dri4")
    format, chroma = FORMATS_OF["422"][0]
    _run(driver, tmp_path, f, ps.frame_planes(f), format, chroma, 300, "tight", 0)
    l2 = cs.table_regime(f)["entries"]
    assert we.REPORTS == [(l2 + 2 * cs.FAST_ENTRIES, l2 + 2 * cs.FAST_ENTRIES, 1)]
