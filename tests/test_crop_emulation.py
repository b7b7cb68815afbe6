"""The cropped kernels' lane body and touch test (compeg_amd/csrc/crop_body.h) on the CPU: tests/emul_crop/crop_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and run directly (nothing is loaded into Python, nothing
preloaded), drives them lane by lane over exact-size heap copies of words, start positions and LUTs and an "LDS" filled with
0xA5 -- making the prologue's tests where the kernel makes them: an untouched workgroup is not set up, an untouched wave has
no window.  Every sampling x both formats; destinations tight, pitched (RGBA) and at an odd address (planar); windows of 300
words and of 8, which cuts every wave's intervals; the restart intervals and rectangles of tests/crop_stream.py.  The
destination lies between sentinels and over a pre-fill of 0xA5: the pitch padding, the MCUs behind the last complete
interval and the sentinels must survive.  Every byte equals tests/crop_stream.py.

The touch test: crop_reach against a search through the MCUs for every interval of every listed DRI and rectangle (the
search made in Python) and for every rectangle of a 5 x 4-MCU image at DRI 1 .. 21 and 0 (the search made in the driver);
two mutants of it -- off by one at the row wrap, the last MCU of an interval ignored -- must each be caught."""
import os
import re
import subprocess

import numpy as np
import pytest

import coef_stream as cs
import crop_stream as crs
import gray_stream as gs
import planes_stream as ps
import wide_emul as we
from conftest import ROOT

SENTINEL, PREFILL, GUARD = 0x5C, 0xA5, 256
# (format, destination, bytes behind a 16-byte boundary, window words)
VARIANTS = (("rgba", "tight", 0, 300), ("rgba", "pitched", 4, 8), ("rgb_planar", "tight", 0, 8), ("rgb_planar", "tight", 1, 300))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_crop")
    exe = str(tmp / "crop_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_crop", "crop_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


def _run(driver, tmp_path, f, full, rect, format, destination, shift, window, waves=3, luts=()):
    """-> the driver's counts: (skipped workgroups, waves, lanes, walked lanes, walked MCUs, stored MCUs)."""
    rgba, mask = full
    (tmp_path / "in.jpg").write_bytes(f.jpeg())
    comps, hs, vs = ps.sampling_of(f)
    pitch = (4 * rect[2] + 15) // 16 * 16 + 16 if destination == "pitched" else None
    pt, total = crs.shape(f.w, f.h, rect, format, pitch)
    flags = (4 if comps == 1 else 1) | (2 if f.standard else 0)
    args = [driver, "decode", str(tmp_path / "in.jpg"), str(tmp_path / "out.bin"), str(flags), str(waves), str(window), str(crs.FORMATS.index(format)),
            str(shift)] + [str(v) for v in rect] + [str(pt), str(total)]
    r = subprocess.run(args + list(luts), capture_output=True, text=True, timeout=120)
    we.note(r.stderr)
    what = f"{f.name}: {rect}, {format}, window {window}, {destination}, shift {shift}"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0].split()[1:] == [str(f.w), str(f.h), str(f.intervals), str(f.interval)], what
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + shift + total
    assert (block[:GUARD + shift] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got = block[GUARD + shift:-GUARD]
    want = crs.destination(rgba, mask, rect, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8))
    bad = np.flatnonzero(got != want)
    if "beyond" in luts:
        return bad.size   # (the control: the caller says what it expects)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    return tuple(int(v) for v in re.findall(r"\d+", lines[1]))


@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_lane_body_on_every_sampling_and_format(driver, tmp_path, layout):
    import compeg_amd as ca   # (the host front end: no device is opened)
    n = 0
    w, h = crs.SIZE
    for i, ri in enumerate(crs.DRIS[layout]):
        f = ps.sized(layout, w, h, ri, standard=i % 2 == 1, seed=3 + i)
        full = crs.frame_rgba(f)
        assert full[1].all()
        for rect in crs.RECTS:
            _run(driver, tmp_path, f, full, rect, *VARIANTS[n % 4])
            n += 1
        _run(driver, tmp_path, f, full, (37, 11, 150, 41), *VARIANTS[(i + 1) % 4])
        _run(driver, tmp_path, f, full, (37, 11, 150, 41), *VARIANTS[(i + 3) % 4])
    for f in (ps.sized(layout, 8, 8, 0, seed=1), ps.sized(layout, 1, 1, 0, seed=2)):
        for v in VARIANTS:
            _run(driver, tmp_path, f, crs.frame_rgba(f), (0, 0, f.w, f.h), *v)
    _run(driver, tmp_path, f, crs.frame_rgba(f), (0, 0, 1, 1), *VARIANTS[1])
    # nine MCUs at DRI 4: the ninth is not decoded -- a rectangle with it inside, one of it alone, one away from it
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    f = ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3)
    full = crs.frame_rgba(f, ca=ca)
    assert not full[1].all() and not full[1][2 * mh:, 2 * mw:].any(), "the frame must have its last MCU behind the last complete interval"
    for k, rect in enumerate(((0, 0, f.w, f.h), (2 * mw + 1, 2 * mh + 1, mw - 2, mh - 3), (1, 1, 2 * mw - 1, 2 * mh), (mw, mh, 2 * mw, 2 * mh - 1))):
        for v in (VARIANTS[k % 4], VARIANTS[(k + 2) % 4]):
            counts = _run(driver, tmp_path, f, full, rect, *v)
        if k == 1:
            assert counts[5] == 0, "nothing is stored for a rectangle inside the undecoded MCU"


def test_skipped_workgroups_waves_and_lanes(driver, tmp_path):
    """640 x 384 4:2:2 at DRI 1: 1920 intervals, 40 to an MCU row; workgroups of three waves (192 intervals) and of twelve."""
    f = ps.sized("422", 640, 384, 1, seed=11)
    assert f.intervals == 1920 and f.mcus_w == 40
    full = crs.frame_rgba(f)
    # inside MCU rows 10 .. 12 (intervals 400 .. 519): some waves of a workgroup touched, others not
    counts = _run(driver, tmp_path, f, full, (100, 85, 200, 19), "rgba", "pitched", 4, 300, waves=12)
    assert counts[0] == 2 and counts[1] == 10 and counts[2] == 128 - 39 and counts[3] == counts[4] == counts[5] == 3 * 13, counts
    counts = _run(driver, tmp_path, f, full, (100, 85, 200, 19), "rgb_planar", "tight", 1, 8, waves=3)
    assert counts[0] == 9 and counts[3] == 3 * 13, counts
    # in the last two MCU rows: the first workgroups are untouched
    counts = _run(driver, tmp_path, f, full, (3, 370, 630, 14), "rgba", "tight", 0, 300, waves=12)
    assert counts[0] == 2 and counts[3] == 80, counts
    # one pixel
    counts = _run(driver, tmp_path, f, full, (333, 200, 1, 1), "rgb_planar", "tight", 1, 300, waves=12)
    assert counts[0] == 2 and counts[3] == counts[5] == 1, counts


FAMILIES = ("dc_cats", "dc_hostile", "q1_underflow", "dc_wrap", "dc_sweep", "saturated", "gamut", "random_dense")


def _family_frames():
    """One frame of each family in each entropy mode it has, 4:2:2; every family once in another sampling; grayscale ones."""
    seen, out = set(), []
    for f in cs.cases():
        key = (f.family, f.standard, f.layout == "422")
        if f.family in FAMILIES and key not in seen:
            seen.add(key)
            out.append(f)
    seen = set()
    for f in gs.cases():
        if f.family in FAMILIES and f.family not in seen:
            seen.add(f.family)
            out.append(f)
    return out


@pytest.mark.parametrize("name", [f.name for f in _family_frames()])
def test_lane_body_on_the_coefficient_families(driver, tmp_path, name):
    f = gs.case(name) if "/gray/" in name else cs.case(name)
    full = crs.frame_rgba(f)
    rect = (3, 2, f.w - 5, f.h - 3) if f.w > 5 and f.h > 3 else (0, 0, f.w, f.h)
    _run(driver, tmp_path, f, full, rect, "rgba", "pitched", 0, 8)
    _run(driver, tmp_path, f, full, rect, "rgb_planar", "tight", 1, 300)


def test_touch_test_against_the_search_and_its_mutants(driver, tmp_path):
    cases = crs.touch_cases()
    assert len(cases) > 5000 and any(c[5] for c in cases) and not all(c[5] for c in cases)
    with open(tmp_path / "cases.txt", "w") as fh:
        for wm, total, per, box, k, want in cases:
            fh.write(f"{wm} {total} {per} {box[0]} {box[1]} {box[2]} {box[3]} {k} {want}\n")
    r = subprocess.run([driver, "touch", str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    found = {m.group(1): [int(v) for v in m.groups()[1:]] for m in
             re.finditer(r"touch (\w+) (\d+) wrong (\d+) touch_wrong (\d+) mutant_wrap (\d+) mutant_last (\d+)", r.stdout)}
    assert set(found) == {"listed", "exhaustive"}, r.stdout
    assert found["listed"][0] == len(cases) and found["listed"][1:3] == [0, 0] and found["exhaustive"][1:3] == [0, 0]
    assert found["exhaustive"][0] > 10000
    for which in ("listed", "exhaustive"):
        assert found[which][3] > 0, f"no {which} case catches the mutant that is off by one at the row wrap"
        assert found[which][4] > 0, f"no {which} case catches the mutant that ignores an interval's last MCU"


@pytest.mark.parametrize("name", [f.name for f in we.frames()])
def test_lane_body_on_tables_beyond_the_lds_share(driver, tmp_path, name):
    """cs.wide_cases / gs.wide_cases at the planner's budget (tests/emul/lut_budget.h): regime B with the direct tables staged
    in part and the fast mode off, regime C with L2 lookups from global memory beyond entry 12288 -- the driver reports
    what it staged -- and the control: told that everything is staged, every regime-C frame differs from its expectation."""
    f = we.frame(name)
    full = crs.frame_rgba(f)
    whole = (0, 0, f.w, f.h)
    inner = (f.w // 3, f.h // 4, max(1, f.w // 2), max(1, f.h // 2))
    _run(driver, tmp_path, f, full, whole, "rgba", "pitched", 4, 8, luts=we.PLAN)
    we.check_plan(f)
    _run(driver, tmp_path, f, full, inner, "rgb_planar", "tight", 1, 300, luts=we.PLAN)
    if we.regime(f) == "C":
        we.check_control(f, _run(driver, tmp_path, f, full, whole, "rgba", "pitched", 4, 8, luts=we.BEYOND))


def test_ordinary_tables_decode_in_the_fast_mode(driver, tmp_path):
    f = cs.case("random_dense/long/422/reference/dri3")
    _run(driver, tmp_path, f, crs.frame_rgba(f), (0, 0, f.w, f.h), "rgba", "tight", 0, 300)
    l2 = cs.table_regime(f)["entries"]
    assert we.REPORTS == [(l2 + 2 * cs.FAST_ENTRIES, l2 + 2 * cs.FAST_ENTRIES, 1)]
