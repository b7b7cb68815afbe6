"""The levels kernels' lane body (compeg_amd/csrc/levels_body.h) on the CPU: tests/emul_levels/levels_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and run directly (nothing is loaded into Python, nothing
preloaded), drives it over exact-size heap copies of words, start positions and LUTs and an "LDS" filled with 0xA5, a
wave's 64 lanes step by step as the transposed store needs them.  Every sampling x both orders; windows of 300 words and
of 8, which cuts every wave's intervals; frames whose last wave is partly used, a frame without DRI (one lane), MCUs
behind the last complete interval, and streams that run positions past 63.  The destination lies between sentinels and
over a pre-fill of 0xA5: the blocks of undecoded MCUs and the sentinels must survive.  Every byte equals
tests/levels_stream.py."""
import os
import subprocess

import numpy as np
import pytest

import coef_stream as cs
import gray_stream as gs
import levels_stream as ls
import planes_stream as ps
import wide_emul as we
from conftest import ROOT

SENTINEL, PREFILL, GUARD = 0x5C, 0xA5, 256
# (order, window words, waves a workgroup)
VARIANTS = (("zigzag", 300, 3), ("natural", 8, 1), ("natural", 300, 2), ("zigzag", 8, 16))
# 324 x 70 (189, 105, 369, 205, 369 MCUs): the DRIs divide the MCU counts; 0: no DRI, one lane.  4:2:2 at DRI 1 is 189
# intervals (a third wave of 61 lanes), at DRI 3 it is 63 (one lane short of a wave).
DRIS = {"422": (1, 3, 0), "420": (3,), "444": (3,), "440": (5,), "gray": (3,)}
FAMILIES = ("random_dense", "positions", "run_size0", "ac_sizes", "dc_cats", "dc_hostile", "dc_wrap", "q1_underflow")


def _frames(layout):
    out = [ps.sized(layout, 324, 70, ri, standard=i % 2 == 1, seed=3 + i) for i, ri in enumerate(DRIS[layout])]
    out.append(ps.sized(layout, 1, 1, 0, seed=2))
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    out.append(ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3))   # (nine MCUs at DRI 4: the ninth is not decoded)
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_levels")
    exe = str(tmp / "levels_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_levels", "levels_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


def _run(driver, tmp_path, f, levels, order, window, waves, luts=()):
    (tmp_path / "in.jpg").write_bytes(f.jpeg())
    mw, mh, comps, hs, vs = ls.frame_geometry(f)
    lay, total = ls.shape(f.w, f.h, comps, hs, vs)
    flags = (4 if comps == 1 else 1) | (2 if f.standard else 0)
    pad = [0] * (3 - comps)
    args = [driver, str(tmp_path / "in.jpg"), str(tmp_path / "out.bin"), str(flags), str(waves), str(window), str(ls.ORDERS.index(order)), str(total)]
    args += [str(x) for key in ("offset", "blocks_w", "blocks_h") for x in [c[key] for c in lay] + pad]
    r = subprocess.run(args + list(luts), capture_output=True, text=True, timeout=120)
    we.note(r.stderr)
    what = f"{f.name}: {order}, window {window}, {waves} waves a workgroup"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    assert r.stdout.split()[1:] == [str(f.w), str(f.h), str(f.intervals), str(f.interval)], what
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + total
    assert (block[:GUARD] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got = block[GUARD:-GUARD]
    want = ls.destination(levels, mw, mh, comps, hs, vs, order, before=np.full(total, PREFILL, dtype=np.uint8))
    bad = np.flatnonzero(got != want)
    if "beyond" in luts:
        return bad.size   # (the control: the caller says what it expects)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    return want


@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_lane_body_on_every_sampling_and_order(driver, tmp_path, layout):
    import compeg_amd as ca   # (the host front end: no device is opened)
    for f in _frames(layout):
        levels = ls.any_frame_levels(f, ca)
        for order, window, waves in VARIANTS:
            want = _run(driver, tmp_path, f, levels, order, window, waves)
        if "/short" in f.name:
            assert (want.reshape(-1, 128) == PREFILL).all(axis=1).any(), "the frame must have blocks behind its last complete interval"


def _family_frames():
    """One frame of each family in each entropy mode it has, 4:2:2; every family once in each other sampling it has; grayscale."""
    seen, out = set(), []
    for f in cs.cases():
        key = (f.family, f.standard if f.layout == "422" else None, f.layout)
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
    """Among them the streams that run positions past 63: `positions` (a run that overshoots, 63 coefficients without EOB, Q2's
    ZRL from 47 and 48), `run_size0` (run symbols to 67) and `random_dense`."""
    f = gs.case(name) if "/gray/" in name else cs.case(name)
    levels = ls.frame_levels(f)
    _run(driver, tmp_path, f, levels, "zigzag", 8, 2)
    _run(driver, tmp_path, f, levels, "natural", 300, 3)


def test_the_families_reach_beyond_position_31():
    """Every sampling has a frame whose chosen levels are non-zero somewhere in 32..63."""
    for layout in ("422", "444", "440", "420", "gray"):
        frames = [f for f in _family_frames() if ("/gray/" in f.name) == (layout == "gray") and (layout == "gray" or f.layout == layout)]
        assert any(ls.frame_levels(f)[:, 32:].any() for f in frames), layout


@pytest.mark.parametrize("name", [f.name for f in we.frames()])
def test_lane_body_on_tables_beyond_the_lds_share(driver, tmp_path, name):
    """cs.wide_cases / gs.wide_cases at the planner's budget (tests/emul/lut_budget.h): regime B with the direct tables staged
    in part and the fast mode off, regime C with L2 lookups from global memory beyond entry 12288 -- the driver reports
    what it staged -- and the control: told that everything is staged, every regime-C frame differs from its expectation."""
    f = we.frame(name)
    levels = ls.frame_levels(f)
    _run(driver, tmp_path, f, levels, "zigzag", 8, 2, luts=we.PLAN)
    we.check_plan(f)
    _run(driver, tmp_path, f, levels, "natural", 300, 3, luts=we.PLAN)
    if we.regime(f) == "C":
        we.check_control(f, _run(driver, tmp_path, f, levels, "natural", 300, 3, luts=we.BEYOND))


def test_ordinary_tables_decode_in_the_fast_mode(driver, tmp_path):
    """The planner's budget counts the direct AC tables (runtime.cpp: staged_lut_entries): with ordinary tables the body is
    told they are staged and the fast entropy mode is on, as on the card."""
    f = cs.case("texture/edge/422/reference/dri4")
    _run(driver, tmp_path, f, ls.frame_levels(f), "zigzag", 300, 3)
    l2 = cs.table_regime(f)["entries"]
    assert we.REPORTS == [(l2 + 2 * cs.FAST_ENTRIES, l2 + 2 * cs.FAST_ENTRIES, 1)]
