"""Frames whose Huffman tables outgrow their share of LDS (tests/coef_stream.py: WIDE_KINDS, wide_cases; tests/gray_stream.py:
wide_cases) against the oracle and the host front end (no GPU).

The kernels stage L1, then L2, then the two direct AC tables, and the planners stop at cs.LDS_SHARE entries behind L1.  A
file is in regime A (everything staged: every frame of cs.cases()), B (all of L2 staged, the direct tables in part: the
fast entropy mode must stay off) or C (L2 lookups at and beyond entry 12288 come from global memory).  Here: that
cs.table_regime counts what the front end and the oracle build, that the oracle decodes what the writer predicted, that
the frames are laid out as their kinds promise -- which tables lie on which side of the boundary, which code lengths the
used symbols have there --, that B and C occur in every sampling, and that one block beyond `full` both parsers refuse.
The emulated bodies run these frames in tests/test_coef_emulation.py and the drivers' modules, the card in
tests/test_gpu_wide_tables.py."""
import numpy as np
import pytest

import coef_stream as cs
import compeg_amd as ca
import gray_stream as gs
from oracle import oracle as orc

COLOUR = [f.name for f in cs.wide_cases()]
GRAY = [f.name for f in gs.wide_cases()]
SAMPLINGS = ("422", "444", "440", "420", "gray")


def frame(name):
    return next(f for f in cs.wide_cases() + gs.wide_cases() if f.name == name)


def used_symbols(f):
    """table slot -> the symbols the stream codes with it."""
    out = {t: set() for t in range(4)}
    for k, (diff, syms) in enumerate(f.dus):
        td, ta, _ = f.sel[f.comp_of_du[k % f.dus_per_mcu]]
        out[2 * td].add(cs.mag(diff)[0])
        out[2 * ta + 1] |= {r << 4 | s for (r, s, _) in syms}
    return out


def used_entries(f, t):
    """[(L2 entry, code length)] of the used symbols of table slot t whose codes are longer than 8 bits."""
    return [(cs.entry_of(f, t, s), f.huff[t][s]) for s in used_symbols(f)[t] if f.huff[t][s] > 8]


@pytest.mark.parametrize("name", COLOUR + GRAY)
def test_table_regime_counts_what_the_parsers_build(name):
    f = frame(name)
    r = cs.table_regime(f)
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    assert len(img.huffman_l2()) == 2 * r["entries"]
    t = gs.twin(f) if isinstance(f, gs.GrayFrame) else f   # (the oracle parses three components: the twin has the same tables)
    o = orc.ImageData(t.jpeg(), **t.image_kw())
    assert len(o.l2()) == 2 * r["entries"] and o.l2() == img.huffman_l2() and o.l1() == img.huffman_l1()
    assert r["entries"] == cs.L2_BLOCK * sum(r["blocks"]) <= cs.INDEX_SPACE
    assert r["regime"] == ("A" if r["entries"] + 2 * cs.FAST_ENTRIES <= cs.LDS_SHARE else "B" if r["entries"] <= cs.LDS_SHARE else "C")
    # every block is one the delegates of L1 name, in the order of the concatenation
    l1 = np.frombuffer(img.huffman_l1(), dtype=np.uint16).reshape(4, 256)
    for slot in range(4):
        mine = sorted({int(e) & 0x7FFF for e in l1[slot] if e & 0x8000})
        assert mine == [r["first"][slot] + cs.L2_BLOCK * k for k in range(r["blocks"][slot])], (name, slot)


@pytest.mark.parametrize("name", COLOUR)
def test_oracle_decodes_what_the_writer_predicted(name):
    f = frame(name)
    pred = cs.predict(f)
    rgba, coef = orc.ImageData(f.jpeg(), **f.image_kw()).decode(want_coefficients=True, strict=True)
    assert np.array_equal(coef.reshape(-1, 32), pred[:, :32]), name
    assert np.array_equal(cs.expectation(f), rgba), name


@pytest.mark.parametrize("name", GRAY)
def test_grayscale_expectation(name):
    """The oracle's decode of the twin where neither reader runs dry (tests/test_gray_stream.py); in reference mode the
    oracle's own entropy pass over the one-component block as well."""
    f = frame(name)
    a, b = {}, {}
    pred = cs.predict(f, facts=a)
    cs.predict(gs.twin(f), facts=b)
    if not a["dry"] and not b["dry"]:
        t = gs.twin(f)
        assert np.array_equal(gs.expectation(f), orc.ImageData(t.jpeg(), **t.image_kw()).decode(strict=True)), name
    if not f.standard:
        img = ca.ImageData(f.jpeg(), allow_grayscale=True)
        off, n = img.scan_range()
        sb = orc.ScanBuffer()
        sb.process(f.jpeg()[off:off + n], img.parallelism())
        words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32).copy()
        starts = np.frombuffer(sb.start_positions(), dtype=np.uint32).copy()
        md, l1, l2 = (np.frombuffer(x, dtype=np.uint8).copy() for x in (img.metadata(), img.huffman_l1(), img.huffman_l2()))
        coef = np.zeros(f.intervals * f.interval * 32, dtype=np.int32)
        orc.lib().orc_huffman_pass(md.ctypes.data, l1.ctypes.data, l2.ctypes.data, len(img.huffman_l2()), words.ctypes.data, words.size,
                                   starts.ctypes.data, starts.size, coef.ctypes.data, coef.size)
        assert np.array_equal(coef.reshape(-1, 32), pred[:, :32]), name


def test_one_block_beyond_full_is_refused_by_both_parsers():
    full = cs.table_regime(cs.ac_sizes("full", dc=True))
    assert full["entries"] == cs.INDEX_SPACE and sum(full["blocks"]) == 128
    for lay in cs.LAYOUTS:
        f = cs.one_block_too_many(lay)
        assert sum(cs.table_regime(f)["blocks"]) == 129 and max(cs.table_regime(f)["blocks"]) <= 128   # (no single table is too large)
        with pytest.raises(orc.OracleError):
            orc.ImageData(f.jpeg(), **f.image_kw())
        with pytest.raises(ca.Error) as e:
            ca.ImageData(f.jpeg(), **f.image_kw())
        assert e.value.code == ca.E_MALFORMED and "15-bit L2 index space" in str(e.value)
    g = gs.gray_of(cs.one_block_too_many("444"))
    with pytest.raises(ca.Error) as e:
        ca.ImageData(g.jpeg(), **g.image_kw())
    assert e.value.code == ca.E_MALFORMED


def test_regimes_b_and_c_occur_in_every_sampling():
    seen = {(("gray" if isinstance(f, gs.GrayFrame) else f.layout), cs.table_regime(f)["regime"]) for f in cs.wide_cases() + gs.wide_cases()}
    for lay in SAMPLINGS:
        for regime in "ABC":
            assert (lay, regime) in seen, (lay, regime)
    for lay in SAMPLINGS:
        mine = [f for f in cs.wide_cases() + gs.wide_cases() if ("gray" if isinstance(f, gs.GrayFrame) else f.layout) == lay]
        assert {f.standard for f in mine if cs.table_regime(f)["regime"] == "C"} == {False, True}, lay
        assert {f.standard for f in mine if cs.table_regime(f)["regime"] == "B"} == {False, True}, lay
        assert any(f.mcus == 1 for f in mine) and any(f.intervals == 65 for f in mine) and any(f.ri == 0 and f.mcus > 1 for f in mine), lay
    assert not {f.name for f in cs.wide_cases()} & {f.name for f in cs.cases()}
    assert max(f.mcus for f in cs.wide_cases() + gs.wide_cases()) == 520   # (the dense strip, which cuts a window; nothing larger)
    strip = cs.wide_case("random_dense_strip/wide_c/422/reference")
    facts = {}
    cs.predict(strip, facts=facts)
    assert strip.intervals == 1 and not facts["dry"] and len(gs.file_scan(strip.jpeg())) > 6144 * 4


@pytest.mark.parametrize("kind,regime", [("wide_a", "A"), ("wide_b", "B"), ("wide_b48", "B"), ("wide_c", "C"), ("full", "C")])
def test_a_frame_per_regime_differs_from_its_short_twin_in_bytes_only(kind, regime):
    for lay in cs.LAYOUTS:
        f, twin = cs.wide_case(f"ac_sizes_dc/{kind}/{lay}/reference"), cs.ac_sizes("short", lay, dc=True)
        assert cs.table_regime(f)["regime"] == regime and cs.table_regime(twin)["entries"] == 0
        assert f.dus == twin.dus and f.jpeg() != twin.jpeg()
        assert np.array_equal(cs.predict(f), cs.predict(twin))
        assert np.array_equal(orc.ImageData(f.jpeg(), **f.image_kw()).decode(), orc.ImageData(twin.jpeg(), **twin.image_kw()).decode())


def test_the_boundaries_are_where_the_kinds_say():
    a, b48 = cs.table_regime(cs.ac_sizes("wide_a")), cs.table_regime(cs.ac_sizes("wide_b48"))
    assert a["entries"] == cs.ALL_STAGED == 8192 and b48["entries"] == cs.LDS_SHARE == 12288   # the last file of A, of B
    assert cs.regime_of(cs.ALL_STAGED + cs.L2_BLOCK) == "B" and cs.regime_of(cs.LDS_SHARE + cs.L2_BLOCK) == "C"


@pytest.mark.parametrize("name", [n for n in COLOUR if "/wide_c/" in n or "/wide_c2/" in n or "/full/" in n])
def test_regime_c_frames_look_up_on_both_sides_of_the_boundary(name):
    f = frame(name)
    r = cs.table_regime(f)
    share = cs.LDS_SHARE
    if f.family == "dc_cats":
        # (its AC symbols are EOBs.)  DC codes of 10 .. 16 bits: they escape the cooperative kernel's direct DC table
        # (kDcFastBits = 9); those of the chroma table lie beyond the boundary
        assert {f.huff[0][s] for s in used_symbols(f)[0]} >= {9, 10, 11, 12, 13, 14}
        dc1 = used_entries(f, 2)
        assert r["first"][2] >= share and min(e for e, _ in dc1) >= share and {n for _, n in dc1} >= {9, 10, 11, 12, 13, 14}
        return
    th0, th1 = used_entries(f, 1), used_entries(f, 3)
    assert th0 and th1
    for t in (1, 3):   # codes of at most 8 bits in the same tables
        assert any(f.huff[t][s] <= 8 for s in used_symbols(f)[t]), (name, t)
    if f.tables == "wide_c":
        assert r["first"][2] == share, "Th0 AC ends at the boundary: wholly staged"
        assert max(e for e, _ in th0) < share <= r["first"][3] <= min(e for e, _ in th1)
        assert min(e for e, _ in used_entries(f, 2) or [(share, 0)]) >= share   # (Th1 DC beyond it too)
    else:
        assert r["first"][1] < share < r["first"][2], "the boundary lies inside Th0 AC"
        assert min(e for e, _ in th0) < share <= max(e for e, _ in th0), "one table is read from both places"
        assert min(e for e, _ in th1) >= share
    beyond = {n for t in (1, 3) for e, n in used_entries(f, t) if e >= share}
    if f.family == "random_dense":   # (every AC symbol in use, in luma and in chroma)
        assert beyond == set(range(9, 17)), (name, sorted(beyond))
    else:   # (a table is built over the symbols of all components; each uses some of them)
        assert len(beyond) >= 3 and min(beyond) == 9 and max(beyond) >= 11, (name, sorted(beyond))
    if f.tables == "full":   # the used chroma symbols of the tail sit in the file's last block, up to the 15-bit index's end
        assert r["entries"] == cs.INDEX_SPACE
        last = [e for e, n in th1 if n >= 10]
        assert last and min(last) >= cs.INDEX_SPACE - cs.L2_BLOCK and max(last) <= 0x7FFF


def test_grayscale_regime_c_frames_decode_beyond_the_boundary():
    for g in gs.wide_cases():
        r = cs.table_regime(g)
        if r["regime"] != "C":
            continue
        td, ta, _ = g.sel[0]
        mine = used_entries(g, 2 * ta + 1) + used_entries(g, 2 * td)
        assert any(e >= cs.LDS_SHARE for e, _ in mine), g.name
        if g.name.endswith("/th1"):
            assert (td, ta) == (1, 1) and min(e for e, _ in mine) >= cs.LDS_SHARE
