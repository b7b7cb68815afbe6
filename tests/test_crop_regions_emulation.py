"""The region-list cropped kernels on the CPU (compeg_amd/csrc/crop_regions_body.h over crop_body.h):
tests/emul_crop_regions/crop_regions_driver.cpp, a stand-alone program compiled with g++ -fsanitize=address,undefined and
run directly (nothing is loaded into Python, nothing preloaded), takes the mixed batch's JPEGs and the region list of
tests/crop_regions_stream.py, builds the records with the library's own host code (make_crop_regions_call) and runs the
prologue's tests and decode_wave_cropped lane by lane, per sampling group, over exact-size heap copies -- the record array
included.  Both formats; tight and pitched; aligned and odd base; windows of 300 words and of 8.  The destination lies
between sentinels and over a pre-fill of 0xA5: every byte equals the expectation, so sentinels, pitch padding, slot
remainders and the undecoded MCU's pixels survive.  Two mutants -- every region decoding the first record's rectangle, a
slot placed by the region's rank inside its sampling group -- must each be caught."""
import os
import re
import subprocess

import numpy as np
import pytest

import compeg_amd as ca   # (the host front end, for the short frame's expectation: no device is opened)
import crop_regions_stream as rgs
import planes_stream as ps
import wide_emul as we
from conftest import ROOT

SENTINEL, PREFILL, GUARD = 0x5C, 0xA5, 256
# (format, destination, bytes behind a 16-byte boundary, window words)
VARIANTS = (("rgba", "tight", 0, 300), ("rgba", "pitched", 4, 8), ("rgb_planar", "tight", 0, 8), ("rgb_planar", "tight", 1, 300))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("emul_crop_regions")
    exe = str(tmp / "crop_regions_driver")
    csrc = os.path.join(ROOT, "compeg_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fno-signed-zeros", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "emul_crop_regions", "crop_regions_driver.cpp"),
                           os.path.join(csrc, "front.cpp"), os.path.join(csrc, "scan.cpp"), os.path.join(csrc, "desc.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """(frames, fulls, paths): the mixed batch, its expectation (made once, left unchanged) and its files."""
    tmp = tmp_path_factory.mktemp("emul_crop_regions_files")
    frames = rgs.mixed_batch()
    fulls = rgs.mixed_fulls(frames, ca)
    paths = []
    for i, (f, _) in enumerate(frames):
        (tmp / f"{i}.jpg").write_bytes(f.jpeg())
        paths.append(str(tmp / f"{i}.jpg"))
    return frames, fulls, paths


def _run(driver, tmp_path, batch, regions, format, destination, shift, window, waves=3, mutant=0, luts=()):
    """-> (bytes differing from the expectation, the driver's group counts)."""
    frames, fulls, paths = batch
    slot = rgs.SLOT
    pitch = (4 * slot[0] + 15) // 16 * 16 + 16 if destination == "pitched" else None
    pt, slot_bytes = rgs.shape(slot, format, pitch)
    with open(tmp_path / "manifest.txt", "w") as fh:
        fh.write(f"{rgs.FORMATS.index(format)} {pt} {slot[0]} {slot[1]} {slot_bytes} {shift} {window} {waves} {mutant} {len(frames)} {len(regions)}\n")
        for (f, _), path in zip(frames, paths):
            comps = ps.sampling_of(f)[0]
            fh.write(f"{path} {(4 if comps == 1 else 1) | (2 if f.standard else 0)}\n")
        for image, rect, place in regions:
            fh.write(f"{image} {rect[0]} {rect[1]} {rect[2]} {rect[3]} {place[0]} {place[1]}\n")
    r = subprocess.run([driver, str(tmp_path / "manifest.txt"), str(tmp_path / "out.bin")] + list(luts), capture_output=True, text=True, timeout=300)
    we.note(r.stderr)
    what = f"{format}, window {window}, {destination}, shift {shift}, mutant {mutant}"
    assert r.returncode == 0 and r.stdout.startswith("ok "), what + "\n" + r.stdout[-500:] + r.stderr[-4000:]
    total = slot_bytes * len(regions)
    block = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    assert block.size == 2 * GUARD + shift + total
    assert (block[:GUARD + shift] == SENTINEL).all() and (block[-GUARD:] == SENTINEL).all(), what + ": a sentinel was written"
    got = block[GUARD + shift:-GUARD]
    want = rgs.destination(fulls, regions, slot, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8))
    groups = [int(v) for v in re.search(r"groups (\d+) (\d+) (\d+) (\d+) (\d+)", r.stdout).groups()]
    launches = int(re.match(r"ok (\d+) launches", r.stdout).group(1))
    return np.flatnonzero(got != want), groups, launches, got, want, what


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}-{v[1]}-{v[2]}-{v[3]}")
def test_every_byte_of_the_mixed_batch(driver, tmp_path, batch, variant):
    regions = rgs.mixed_regions()
    bad, groups, launches, got, want, what = _run(driver, tmp_path, batch, regions, *variant)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    restated = rgs.launches([lay for _, lay in batch[0]], regions)
    assert groups == [sum(len(ks) for g, ks in restated if g == name) for name in rgs.GROUPS] and launches == len(restated) == 5


def test_twelve_waves_a_workgroup_and_one_region(driver, tmp_path, batch):
    """Workgroups of twelve waves (768 intervals of the large frame's 1920: untouched waves inside a touched workgroup), and
    a list of one region."""
    regions = rgs.mixed_regions()
    bad, _, _, got, want, what = _run(driver, tmp_path, batch, regions, "rgba", "pitched", 4, 300, waves=12)
    assert not bad.size, f"{what}, 12 waves: {bad.size} bytes differ, first at {bad[0]}"
    bad, groups, launches, _, _, what = _run(driver, tmp_path, batch, regions[8:9], "rgb_planar", "tight", 1, 8)
    assert not bad.size and launches == 1 and sum(groups) == 1, what


@pytest.mark.parametrize("mutant", (1, 2))
def test_the_mutants_are_caught(driver, tmp_path, batch, mutant):
    """1: the first record's rectangle for every region; 2: slot k placed by the region's rank inside its sampling group."""
    bad, _, _, _, _, what = _run(driver, tmp_path, batch, rgs.mixed_regions(), "rgba", "tight", 0, 300, mutant=mutant)
    assert bad.size, f"{what}: the mutant writes what the expectation has"


@pytest.fixture(scope="module")
def wide_batch(tmp_path_factory):
    """Every wide frame of every sampling but the strip in one batch: regimes A, B and C side by side, planned with the
    largest image's tables while each image stages its own (tests/emul/lut_budget.h)."""
    import crop_stream as crs
    tmp = tmp_path_factory.mktemp("emul_crop_regions_wide")
    frames = [(f, we.layout_of(f)) for f in we.frames() if f.mcus <= 65]
    fulls = [crs.frame_rgba(f) for f, _ in frames]
    paths = []
    for i, (f, _) in enumerate(frames):
        (tmp / f"{i}.jpg").write_bytes(f.jpeg())
        paths.append(str(tmp / f"{i}.jpg"))
    return frames, fulls, paths


def test_regions_of_images_with_tables_beyond_the_lds_share(driver, tmp_path, wide_batch, monkeypatch):
    """A region of every image -- the whole frame, or a rectangle inside it -- in one list: each launch names regions of
    regime-A, -B and -C images.  Every byte; then the control: every regime-C image's slot differs, no other does."""
    frames = wide_batch[0]
    slot = (max(f.w for f, _ in frames) + 1, max(f.h for f, _ in frames) + 1)
    monkeypatch.setattr(rgs, "SLOT", slot)
    regions = [(i, (0, 0, f.w, f.h) if i % 2 == 0 else (f.w // 3, f.h // 4, max(1, f.w // 2), max(1, f.h // 2)), (i % 2, i % 3 % 2))
               for i, (f, _) in enumerate(frames)]
    for lay in rgs.GROUPS:
        assert {we.regime(f) for f, l in frames if l == lay} == set("ABC"), lay
    bad, groups, launches, got, want, what = _run(driver, tmp_path, wide_batch, regions, "rgba", "pitched", 4, 8, luts=we.PLAN)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
    assert launches == 5 and sum(groups) == len(regions)
    assert len(we.REPORTS) == len(frames) and {r[0] for r in we.REPORTS} == {12288}, "the batch is planned with its largest image's tables"
    for (f, _), report in zip(frames, we.REPORTS):
        assert report[1:] == we.planned(f)[1:] or we.regime(f) == "A", f.name
        assert report[2] == we.fast_mode(f), f.name
    bad, _, _, got, want, what = _run(driver, tmp_path, wide_batch, regions, "rgb_planar", "tight", 0, 300, luts=we.PLAN)
    assert not bad.size, f"{what}: {bad.size} bytes differ, first at {bad[0]}"
    bad, _, _, got, want, what = _run(driver, tmp_path, wide_batch, regions, "rgba", "pitched", 4, 8, luts=we.BEYOND)
    differs = (got.reshape(len(regions), -1) != want.reshape(len(regions), -1)).any(axis=1)
    for (f, _), d in zip(frames, differs):
        assert d == (we.regime(f) == "C"), f"{f.name}: regime {we.regime(f)}, its slot {'differs' if d else 'does not differ'} under the control"
