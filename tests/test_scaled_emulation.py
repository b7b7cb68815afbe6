"""The scaled kernels' lane body (compeg_amd/csrc/scaled_body.h) on the CPU: tests/emul_scaled/scaled_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and run directly (nothing is loaded into Python, nothing
preloaded), drives it lane by lane over exact-size heap copies of words, start positions and LUTs and an "LDS" filled with
0xA5.  Every sampling x both transform sizes x both formats; destinations tight, pitched (RGBA) and at an odd address
(planar); windows of 300 words and of 8, which cuts every wave's intervals.  The destination lies between sentinels and
over a pre-fill of 0xA5: the pitch padding, the pixels of MCUs the scaled extent cuts, the MCUs behind the last complete
interval and the sentinels must survive.  Every byte equals tests/scaled_stream.py.

324 x 70: at denominator 4 the extent is 81 x 18, at 2 it is 162 x 35, and an MCU is N hs x N vs pixels, N = 8 / den.
81 is odd and 162 = 2 mod 4 and mod 8: the right edge cuts an MCU in every sampling at both scales.  35 = 3 mod 4 and mod 8
and 18 = 2 mod 4: the bottom edge cuts one too, except at denominator 4 where vs = 1 (nine MCU rows of 2 are the 18 rows);
the test asserts exactly that."""
import os
import subprocess

import numpy as np
import pytest

import coef_stream as cs
import gray_stream as gs
import planes_stream as ps
import scaled_stream as ss
import wide_emul as we
from conftest import ROOT
from test_reduced_emulation import DRIS, FAMILIES

SENTINEL, PREFILL, GUARD = 0x5C, 0xA5, 256
# (format, destination, bytes behind a 16-byte boundary, window words)
VARIANTS = (("rgba", "tight", 0, 300), ("rgba", "pitched", 4, 8), ("rgb_planar", "tight", 0, 8), ("rgb_planar", "tight", 1, 300))
DENS = (2, 4)


def _frames(layout):
    out = [ps.sized(layout, 324, 70, ri, standard=i % 2 == 1, seed=3 + i) for i, ri in enumerate(DRIS[layout])]
    if 0 not in DRIS[layout]:
        out.append(ps.sized(layout, 324, 70, 0, seed=5))   # (no DRI: one lane walks the whole image)
    out += [ps.sized(layout, 8, 8, 0, seed=1), ps.sized(layout, 1, 1, 0, seed=2)]
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    out.append(ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3))   # (nine MCUs at DRI 4: the ninth is not decoded)
    if layout == "422":
        out.append(ps.sized(layout, 640, 192, 1, seed=11))   # (960 intervals: fifteen waves, five workgroups of three)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_scaled")
    exe = str(tmp / "scaled_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_scaled", "scaled_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


def _run(driver, tmp_path, f, planes, den, format, destination, shift, window, luts=()):
    (tmp_path / "in.jpg").write_bytes(f.jpeg())
    comps, hs, vs = ps.sampling_of(f)
    ow = -(-f.w // den)
    pitch = (4 * ow + 15) // 16 * 16 + 16 if destination == "pitched" else None
    ow, oh, pt, total = ss.shape(f.w, f.h, den, format, pitch)
    flags = (4 if comps == 1 else 1) | (2 if f.standard else 0)
    args = [driver, str(tmp_path / "in.jpg"), str(tmp_path / "out.bin"), str(flags), "3", str(window), str(ss.FORMATS.index(format)),
            str(shift), str(ow), str(oh), str(pt), str(total), str(8 // den)]
    r = subprocess.run(args + list(luts), capture_output=True, text=True, timeout=120)
    we.note(r.stderr)
    what = f"{f.name}: 1/{den}, {format}, window {window}, {destination}, shift {shift}"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    assert r.stdout.split()[1:] == [str(f.w), str(f.h), str(f.intervals), str(f.interval)], what
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + shift + total
    assert (block[:GUARD + shift] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got = block[GUARD + shift:-GUARD]
    want = ss.destination(planes, f.w, f.h, den, hs, vs, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8))
    bad = np.flatnonzero(got != want)
    if "beyond" in luts:
        return bad.size   # (the control: the caller says what it expects)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("den", DENS)
@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_lane_body_on_every_sampling_scale_and_format(driver, tmp_path, layout, den):
    import compeg_amd as ca   # (the host front end: no device is opened)
    for f in _frames(layout):
        coef = ss.frame_coefficients(f, ca=ca)
        comps, hs, vs = ps.sampling_of(f)
        planes = ss.scaled_planes(coef, den, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
        if "/short" in f.name:
            assert not planes[3].all(), "the frame must have MCUs behind its last complete interval"
        if (f.w, f.h) == (324, 70):
            mw, mh = (8 // den) * hs, (8 // den) * vs
            assert -(-f.w // den) % mw, "the right edge must cut an MCU"
            assert -(-f.h // den) % mh or (den, vs) == (4, 1), "the bottom edge must cut an MCU"
        for format, destination, shift, window in VARIANTS:
            _run(driver, tmp_path, f, planes, den, format, destination, shift, window)


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
    coef = cs.predict(f)
    comps, hs, vs = ps.sampling_of(f)
    for den in DENS:
        planes = ss.scaled_planes(coef, den, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
        _run(driver, tmp_path, f, planes, den, "rgba", "pitched", 0, 8)
        _run(driver, tmp_path, f, planes, den, "rgb_planar", "tight", 1, 300)


@pytest.mark.parametrize("name", [f.name for f in we.frames()])
def test_lane_body_on_tables_beyond_the_lds_share(driver, tmp_path, name):
    """cs.wide_cases / gs.wide_cases at the planner's budget (tests/emul/lut_budget.h): regime B with the direct tables staged
    in part and the fast mode off, regime C with L2 lookups from global memory beyond entry 12288 -- the driver reports
    what it staged -- and the control: told that everything is staged, every regime-C frame differs from its expectation."""
    f = we.frame(name)
    coef = ss.frame_coefficients(f)
    comps, hs, vs = ps.sampling_of(f)
    for den, (format, destination, shift, window) in zip(DENS, (VARIANTS[1], VARIANTS[3])):
        planes = ss.scaled_planes(coef, den, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
        _run(driver, tmp_path, f, planes, den, format, destination, shift, window, luts=we.PLAN)
        we.check_plan(f)
        if we.regime(f) == "C":
            we.check_control(f, _run(driver, tmp_path, f, planes, den, format, destination, shift, window, luts=we.BEYOND))


def test_ordinary_tables_decode_in_the_fast_mode(driver, tmp_path):
    f = cs.case("random_dense/long/422/reference/dri3")
    comps, hs, vs = ps.sampling_of(f)
    planes = ss.scaled_planes(ss.frame_coefficients(f), 2, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
    _run(driver, tmp_path, f, planes, 2, "rgba", "tight", 0, 300)
    l2 = cs.table_regime(f)["entries"]
    assert we.REPORTS == [(l2 + 2 * cs.FAST_ENTRIES, l2 + 2 * cs.FAST_ENTRIES, 1)]
