"""The fused grayscale kernels' lane body (compeg_amd/csrc/gray_body.h) on the CPU: tests/emul_gray/gray_driver.cpp, a
stand-alone program compiled with g++ -fsanitize=address,undefined and run directly, drives it lane by lane and through
the quad exchange phase by phase, over exact-size heap copies of words, start positions and LUTs and an "LDS" filled with
0xA5.  Both forms (pairs as the runtime dispatches them, and single MCUs for every interval length); outputs padded as
the runtime allocates them -- the padding pre-filled and compared: a decoded MCU the extent cuts is stored whole, nothing
else is touched -- and tight outputs that the edge cuts inside a 16-byte piece, with an unaligned and with an aligned
pitch; windows of 300 words and of 8, which cuts every wave's intervals.  The output lies between sentinels that must
survive.  Every pixel equals gs.expectation."""
import os
import subprocess

import numpy as np
import pytest

import gray_stream as gs
import wide_emul as we
from conftest import ROOT
from test_gray_stream import FIXTURES, fixture, pil_l

SENTINEL, PREFILL, GUARD = 0x5C, 0x3C, 256


def _frames():
    out = [f for f in gs.cases() if f.family in ("random_gray", "q1_underflow", "positions", "dc_hostile", "pairs") or f.mcus > 64]
    own = {}
    for f in gs.cases():
        own.setdefault(f.family, f)   # (every family once at the least: its own geometry)
    out += [f for f in own.values() if f not in out]
    return out


FRAMES = _frames()
# (form, window words, output): the output "padded" as the runtime allocates it, "tight3" = 3 pixels short each way with
# rows one behind the other (an unaligned pitch wherever that is no multiple of 4 pixels), "tight2" = 2 columns and 1 row
# short with the pitch rounded up to 16 bytes
VARIANTS = (("pairs", 300, "padded"), ("single", 300, "padded"), ("pairs", 8, "tight3"), ("pairs", 300, "tight2"), ("single", 8, "tight2"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_gray")
    exe = str(tmp / "gray_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_gray", "gray_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


def _geometry(f, output):
    """(tex_w, tex_h, pitch, rows behind the pointer)."""
    if output == "padded":
        return f.w, f.h, (f.w + 15) // 16 * 64, (f.h + 15) // 16 * 16
    if output == "tight3":
        w, h = max(1, f.w - 3), max(1, f.h - 3)
        return w, h, w * 4, h
    w, h = max(1, f.w - 2), max(1, f.h - 1)
    return w, h, (w + 3) // 4 * 16, h


def _expected(f, tex_w, tex_h, pitch, rows):
    """(the bytes behind the pointer afterwards, which of them may also have kept their pre-fill).  A decoded MCU that
    begins inside the extent and lies whole inside what is allocated, rows 16-byte aligned, is stored whole (gray_target,
    pair_half_limit) -- in an output as the runtime allocates it, every one; in a tight one its pixels outside the extent
    may stay as they were, where its pair's other MCU is the edge path's and takes it along (gray_pair_limits).  Of any
    other MCU, what lies inside the extent; the rest keeps its pre-fill."""
    full = gs.expectation(f, whole_mcus=True)
    out = np.full((rows, pitch), PREFILL, dtype=np.uint8)
    either = np.zeros((rows, pitch), dtype=bool)
    decoded = f.intervals * f.interval
    for m in range(decoded):
        my, mx = divmod(m, f.mcus_w)
        x0, y0 = mx * 8, my * 8
        if x0 >= tex_w or y0 >= tex_h:
            continue
        whole = pitch % 16 == 0 and (x0 + 8) * 4 <= pitch and y0 + 8 <= rows
        x1, y1 = (x0 + 8, y0 + 8) if whole else (min(x0 + 8, tex_w), min(y0 + 8, tex_h))
        out[y0:y1, x0 * 4:x1 * 4] = full[y0:y1, x0:x1].reshape(y1 - y0, -1)
        either[y0:y1, x0 * 4:x1 * 4] = True
    either[:tex_h, :tex_w * 4] = False
    return out, either


def _run(driver, tmp_path, f, jpeg, form, window, output, luts=()):
    (tmp_path / "in.jpg").write_bytes(jpeg)
    tex_w, tex_h, pitch, rows = _geometry(f, output)
    flags = 4 | (2 if f.standard else 0)
    r = subprocess.run([driver, str(tmp_path / "in.jpg"), str(tmp_path / "out.bin"), str(flags), "3", str(window), "1" if form == "single" else "0",
                        str(tex_w), str(tex_h), str(pitch), str(rows)] + list(luts), capture_output=True, text=True, timeout=120)
    we.note(r.stderr)
    what = f"{f.name}: {form}, window {window}, {output}"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    assert r.stdout.split()[1:] == [str(f.w), str(f.h), str(f.intervals), str(f.interval)], what
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + pitch * rows
    assert (block[:GUARD] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got, (want, either) = block[GUARD:-GUARD].reshape(rows, pitch), _expected(f, tex_w, tex_h, pitch, rows)
    if output == "padded":
        either[:] = False   # (every MCU is stored whole there)
    bad = np.argwhere((got != want) & ~(either & (got == PREFILL)))
    if "beyond" in luts:
        return len(bad)   # (the control: the caller says what it expects)
    assert not bad.size, f"{what}: {len(bad)} bytes differ, first at row {bad[0][0]} byte {bad[0][1]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", [f.name for f in FRAMES])
def test_lane_body_on_coefficient_frames(driver, tmp_path, name):
    f = gs.case(name)
    for form, window, output in VARIANTS:
        if form == "single" and f.interval == 1 and output != "padded":
            continue   # (intervals of one MCU: "pairs" is the single form already)
        _run(driver, tmp_path, f, f.jpeg(), form, window, output)


@pytest.mark.parametrize("name", FIXTURES)
def test_lane_body_on_the_fixtures(driver, tmp_path, name):
    j = fixture(name)
    f = gs.from_jpeg(j, name)
    for form, window, output in VARIANTS[:4]:
        _run(driver, tmp_path, f, j, form, window, output)


@pytest.mark.parametrize("w,h,blocks", [(8, 8, 0), (10, 10, 1), (17, 9, 2), (40, 24, 3), (40, 24, 0)])
def test_lane_body_on_pil_files(driver, tmp_path, w, h, blocks):
    j = pil_l(w, h, 95, blocks)
    f = gs.from_jpeg(j)
    for form, window, output in VARIANTS:
        _run(driver, tmp_path, f, j, form, window, output)


@pytest.mark.parametrize("name", [f.name for f in we.frames(("gray",))])
def test_lane_body_on_tables_beyond_the_lds_share(driver, tmp_path, name):
    """cs.wide_cases / gs.wide_cases at the planner's budget (tests/emul/lut_budget.h): regime B with the direct tables staged
    in part and the fast mode off, regime C with L2 lookups from global memory beyond entry 12288 -- the driver reports
    what it staged -- and the control: told that everything is staged, every regime-C frame differs from its expectation."""
    f = we.frame(name)
    for form, window, output in VARIANTS:
        if form == "single" and f.interval == 1 and output != "padded":
            continue
        _run(driver, tmp_path, f, f.jpeg(), form, window, output, luts=we.PLAN)
        we.check_plan(f)
    if we.regime(f) == "C":
        form, window, output = VARIANTS[0]
        we.check_control(f, _run(driver, tmp_path, f, f.jpeg(), form, window, output, luts=we.BEYOND))


def test_ordinary_tables_are_staged_with_their_direct_tables(driver, tmp_path):
    """The planner's budget counts the direct AC tables (runtime.cpp: staged_lut_entries) and the body is told so.  The fast
    entropy mode stays off all the same: a grayscale image's absent components name no direct table (we.fast_mode)."""
    import coef_stream as cs
    f = FRAMES[0]
    _run(driver, tmp_path, f, f.jpeg(), *VARIANTS[0])
    l2 = cs.table_regime(f)["entries"]
    assert we.REPORTS == [(l2 + 2 * cs.FAST_ENTRIES, l2 + 2 * cs.FAST_ENTRIES, 0)]
