"""The scan edge matrix (tests/scan_edges.py) without a GPU: on every one of its cases the host preprocessor agrees
with the oracle; the restated references (flags, window span, kept bytes, the parser's segment end) agree with
brute-force versions; the harness that drives the kernels on the card was built with a gfx950 code object in it.

3433 (segment, expected) pairs in the scan groups (CASE_COUNT, asserted below, so that a case that goes missing is
noticed), many of them at several misalignments and between both kinds of neighbours, and 12 pull groups."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scan_edges as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "gpu_scan", "scan_harness")
LLVM = "/opt/rocm/lib/llvm/bin"
CASE_COUNT = 3433


def _cases(names):
    seen = {}
    for name in names:
        for im in se.group(name).images:
            seen.setdefault((im.seg, im.expected), f"{name} {im.name}")
    return seen


def test_case_count():
    assert len(_cases(se.SCAN_GROUP_NAMES)) == CASE_COUNT


@pytest.mark.parametrize("name", se.SCAN_GROUP_NAMES)
def test_host_preprocessor_agrees_with_the_oracle(name):
    import compeg_amd as ca
    for (seg, expected), what in _cases([name]).items():
        count, words, starts, err = se.oracle_scan(seg, expected)
        sb, got_err = ca.ScanBuffer(), None
        try:
            sb.process(seg, expected)
        except ca.Error as e:
            assert e.code == ca.E_COUNT_MISMATCH
            got_err = str(e)
        assert got_err == err, what
        assert sb.processed_scan_data() == words, what
        assert sb.start_positions() == starts.tobytes(), what


def test_the_matrix_is_what_the_issue_asks_for():
    """Structure: the run lengths, positions and followers of the ladder; every length with its expected counts; the
    capacity edge; all four misalignments with both neighbours in every scan group; the grouped launch's mix."""
    assert set(se.RUNS) == set(range(1, 21)) | {31, 32, 33, 47, 48, 49, 255, 256, 257} | set(range(509, 531))
    for end in se.ENDS:
        g = se.group(f"ladder[{end}]")
        assert len({im.seg for im in g.images}) >= len(se.RUNS) * (len(se.FOLLOW) - (end == "end")) - 8
        assert max(len(im.seg) for im in g.images) <= 2 * se.TILE
    for name in se.SCAN_GROUP_NAMES:
        g = se.group(name)
        if name.startswith(("ladder", "dense", "seam", "length")):
            by_seg = {}
            for im in g.images:
                by_seg.setdefault(im.seg, set()).add((im.mis, im.fill))
            assert any(len(v) == 8 for v in by_seg.values()), name
        assert {im.mis for g2 in (g,) for im in g2.images} <= {0, 1, 2, 3}
    for n in se.LENGTHS:
        g = se.group(f"length[{n}]")
        first = next(im for im in g.images if im.name.startswith("expected"))
        count = se.oracle_scan(first.seg, 0)[0]
        expected = {im.expected for im in g.images if im.seg == first.seg}
        assert {count, count + 1, 0, 1} <= expected and (count == 0 or count - 1 in expected)
        if count > 2:
            assert any(se.slots_for(e) < count for e in expected if e), n
        last = next(im for im in g.images if im.name.startswith("power-of-two"))
        assert last.expected & (last.expected - 1) == 0 and se.oracle_scan(last.seg, last.expected)[3] is None
        assert all(len(im.seg) == n for im in g.images)
    # the capacity edge: 4096 bytes of xx FF D0 and one more byte give 5464 output bytes, len + len/3 is 5461
    edge = next(im for im in se.group("dense").images if im.name == "xx-ff-d0[4097-tail1]")
    assert len(edge.seg) == 4097 and len(se.oracle_scan(edge.seg, edge.expected)[1]) == 5464 == 4097 + 4097 // 3 + 4 - 2
    mixed = se.group("mixed")
    tiles = {(len(im.seg) + se.TILE - 1) // se.TILE for im in mixed.images[mixed.skip:]}
    assert {0, 1, 2} <= tiles and max(tiles) >= 257 and mixed.skip > 0 and mixed.with_span
    assert {im.patch for im in mixed.images[mixed.skip:]} == {True, False}
    first, second = se.group("reuse[first]"), se.group("reuse[second]")
    assert se.GROUP_NAMES.index("reuse[second]") == se.GROUP_NAMES.index("reuse[first]") + 1 and second.keep and not first.keep
    for a, b in zip(first.images, second.images):
        assert (len(a.seg), a.slots, a.mis, a.patch) == (len(b.seg), b.slots, b.mis, b.patch) and a.seg != b.seg or not a.seg


@pytest.mark.parametrize("name", se.SMALL_GROUP_NAMES)
def test_references_agree_with_brute_force(name):
    g = se.group(name)
    step = max(1, len(g.images) // 60)          # (the brute-force versions are slow: every step-th image of a ladder)
    for im in g.images[::step]:
        seg = im.seg
        assert se.flags(seg) == se.flags_brute(seg), im.name
        # bit 1 is never clear where the reference's parser would end the segment
        assert (se.parser_end(seg) is not None) == bool(se.flags(seg) & 2), im.name
        count, words, starts, _ = se.oracle_scan(seg, im.expected)
        # kept bytes: the output without its padding
        nwords, nstarts = len(words) // 4, min(count, im.slots)
        if count <= im.slots:
            ends = list(starts[1:]) + [nwords]
            assert se.kept_bytes(seg) <= 4 * nwords and se.kept_bytes(seg) > 4 * nwords - 4 * count, im.name
            assert all(int(a) <= int(b) for a, b in zip(starts, ends)), im.name
        slow, i = 0, 0
        while i < len(seg):
            if seg[i] != 0xFF:
                slow, i = slow + 1, i + 1
            elif i + 1 < len(seg):
                slow, i = slow + (seg[i + 1] == 0), i + 2
            else:
                break
        assert se.kept_bytes(seg) == slow, im.name
        for intervals in {im.expected, count, count + 70, 1, 64, 65}:
            assert se.wave_span(starts, nstarts, nwords, intervals) == se.wave_span_brute(starts, nstarts, nwords, intervals), im.name


def test_flag_definitions_at_their_edges():
    ff = b"\xff"
    assert se.flags(b"\x41" + ff * 511 + b"\x00" * 40) == 0
    assert se.flags(b"\x41" * 16 + ff * 512 + b"\x00" * 40) == 1       # chunk start 528 has 512 FFs in front of it
    assert se.flags(b"\x41" * 15 + ff * 512 + b"\x00" * 40) == 0       # ... 527 is no chunk start
    assert se.flags(ff * 512 + b"\x00") == 0                            # the run reaches the segment's start: g = 512
    assert se.flags(ff * 528) == 0 and se.flags(ff * 529) == 1          # g < len
    assert se.flags(b"\xff\xd8") == 2 and se.flags(b"\xff\xff\xc0") == 2 and se.flags(b"\xff\xd7\xff\x00\xff\xff") == 0
    assert se.flags(b"\xd8\xff") == 0 and se.flags(b"") == 0 and se.flags(ff) == 0
    assert se.parser_end(b"\x01\xff\xd0\x02\xff\xff\xd9") == 5 and se.parser_end(b"\x01\xff\x00\xff") is None


def test_harness_is_built_with_the_shipped_kernels(tmp_path):
    lib = os.path.join(ROOT, "compeg_amd", "libcompeg_hip.so")
    if not (os.path.exists(lib) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))):
        pytest.skip("library or llvm-objdump not here")
    assert os.path.exists(HARNESS), "build() leaves tests/gpu_scan/scan_harness"
    exe = shutil.copy(HARNESS, tmp_path / "harness")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", exe], check=True, capture_output=True, cwd=tmp_path)
    objects = [p for p in tmp_path.iterdir() if "gfx950" in p.name]
    assert objects, "no gfx950 code object in the harness"
    symbols = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", str(objects[0])], check=True, capture_output=True, text=True).stdout
    for kernel in ("count_kernel", "tile_scan_kernel", "emit_kernel", "span_kernel", "pull_kernel", "pull3_kernel"):
        assert kernel in symbols, kernel


def test_case_file_round_trip(tmp_path):
    """The case file as the harness reads it: sizes add up (the harness itself runs on the card only)."""
    names = ["seam", "pull[17]", "pull3[two]"]
    path = tmp_path / "cases.bin"
    se.write_cases(path, names)
    raw = path.read_bytes()
    want = 8 + 20 + sum(24 + (len(im.seg) + 3) // 4 * 4 for im in se.group("seam").images) + 8 + 4 + 32 + 8 + 12 + (se.PULL_STRIDE + 16) + 0 + 16
    assert len(raw) == want and np.frombuffer(raw[:8], dtype="<u4").tolist() == [se.MAGIC, 3]
