"""The coefficient-level frames of tests/coef_stream.py against the oracle and the host front end (no GPU).

Every case: the oracle keeps exactly the coefficients the writer predicted (which proves the writer, and that the case
holds what its name says), the edge the case is named after is really in it (counted by the predictor, and at the DC
codes by stepping the oracle's own reader), the product's front end builds what the oracle's does, and the numpy
restatement of the reference's IDCT and colour step gives the oracle's pixels.  Then the restatement's mutants: each
must change the expectation of a named case, or the cases could not tell a kernel that went wrong that way."""
import numpy as np
import pytest

import coef_stream as cs
import compeg_amd as ca
from oracle import oracle as orc
from test_host_parity import _same_image

NAMES = [f.name for f in cs.cases()]
_DECODED = {}


def decoded(f):
    """(oracle's RGBA, oracle's coefficients [data units, 32], predicted coefficients [data units, 64], facts)."""
    if f.name not in _DECODED:
        facts = {}
        pred = cs.predict(f, facts=facts)
        img = orc.ImageData(f.jpeg(), **f.image_kw())
        rgba, coef = img.decode(want_coefficients=True, strict=True)
        _DECODED[f.name] = (rgba, coef.reshape(-1, 32), pred, facts)
    return _DECODED[f.name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_keeps_the_predicted_coefficients(name):
    f = cs.case(name)
    _, coef, pred, _ = decoded(f)
    assert coef.shape[0] == pred.shape[0] == f.intervals * f.interval * f.dus_per_mcu
    assert not pred[:, 32:].any()
    bad = np.nonzero((coef != pred[:, :32]).any(axis=1))[0]
    assert not bad.size, f"{name}: {bad.size} data units differ, first {bad[0]}: {coef[bad[0]]} != {pred[bad[0], :32]}"


@pytest.mark.parametrize("name", NAMES)
def test_restatement_gives_the_oracles_pixels(name):
    f = cs.case(name)
    want, _, pred, _ = decoded(f)
    got = cs.rgba(f, pred)
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"


@pytest.mark.parametrize("name", NAMES)
def test_front_end_agrees_with_the_oracle(name):
    f = cs.case(name)
    if f.layout == "422" and not f.standard:
        assert _same_image(f.jpeg())
        return
    got, want = ca.ImageData(f.jpeg(), **f.image_kw()), orc.ImageData(f.jpeg(), **f.image_kw())
    assert (got.width(), got.height(), got.parallelism()) == (want.width(), want.height(), want.parallelism())
    assert got.metadata() == want.metadata()
    assert got.huffman_l1() == want.l1() and got.huffman_l2() == want.l2()
    assert got.scan_range() == want.scan_range()


def test_both_parsers_reject_16_bit_quantisation_tables():
    j = cs.case("basis_q1/short/422/reference/dri1").jpeg()
    at = j.find(b"\xff\xdb")
    assert j[at + 2:at + 5] == bytes([0, 67, 0])
    wide = b"\xff\xdb" + (131).to_bytes(2, "big") + bytes([0x10]) + b"".join(int(q).to_bytes(2, "big") for q in j[at + 5:at + 69])
    assert not _same_image(j[:at] + wide + j[at + 69:])   # Pq = 1: rejected by both, with one message


# ---- the edges are real -----------------------------------------------------------------------------------------------

def _levels(f):
    """Every (position the symbol lands on, size, level) the writer coded, by the reference's position arithmetic."""
    out = []
    zrl = 16 if f.standard else 17
    for _, syms in f.dus:
        pos = 1
        for (r, s, bits) in syms:
            if (r, s) == (0, 0):
                break
            if (r, s) == (15, 0):
                pos += zrl
                continue
            pos += r
            out.append((pos, s, cs.extend(bits, s), r))
            pos += 1
    return out


def _code_lengths(f, slot_parity):
    return {n for t, lengths in f.huff.items() if t % 2 == slot_parity for n in lengths.values()}


def _oracle_left_at_dc_codes(f):
    """The bits the oracle's own reader holds in front of every DC code of the frame's first interval that it reaches
    by the writer's symbols (stepping orc.BitStream through the codes the writer wrote): the set of counts, and the
    count at which it first held fewer than the code and its magnitude need (None: never)."""
    sb = orc.ScanBuffer()
    img = orc.ImageData(f.jpeg(), **f.image_kw())
    sb.process(img.scan_data(), img.parallelism())
    words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32)
    codes = {t: cs.canonical(l)[2] for t, l in f.huff.items()}
    seen, short = set(), None
    for iv in range(f.intervals):
        b = orc.BitStream(words, int(np.frombuffer(sb.start_positions(), dtype=np.uint32)[iv]))
        for du in range(iv * f.interval * f.dus_per_mcu, (iv + 1) * f.interval * f.dus_per_mcu):
            td, ta, _ = f.sel[f.comp_of_du[du % f.dus_per_mcu]]
            diff, syms = f.dus[du]
            size, bits = cs.mag(diff)
            code, n = codes[2 * td][size]
            if f.standard:
                b.refill()
            seen.add(b.left)
            if b.left < n + size:
                short = b.left if short is None else short
                break   # (the reader is dry: the rest of the interval is not the writer's symbols any more)
            assert b.peek(n) == code, (f.name, du)
            b.consume(n)
            assert b.peek(size) == bits
            b.consume(size)
            for (r, s, mbits) in syms:
                b.refill()
                code, n = codes[2 * ta + 1][r << 4 | s]
                assert b.peek(n) == code and b.left >= n + s, (f.name, du)
                b.consume(n)
                assert b.peek(s) == mbits
                b.consume(s)
    return seen, short


@pytest.mark.parametrize("name", NAMES)
def test_the_edge_is_real(name):
    f = cs.case(name)
    _, coef, pred, facts = decoded(f)
    levels = _levels(f)
    fam, dpm = f.family, f.dus_per_mcu
    if fam not in ("dc_hostile", "q1_underflow", "random_dense"):
        assert facts["dry"] == 0, "every data unit decodes from its own bits"
    if f.mcus > 64:   # (the strips; and the two sweeps, which need a chroma data unit per value: one MCU each)
        assert fam in ("dc_wrap", "dc_sweep", "gamut") or "strip" in name
    if f.tables == "short":
        assert max(_code_lengths(f, 0) | _code_lengths(f, 1)) <= 8
    elif f.tables == "edge":
        assert _code_lengths(f, 0) | _code_lengths(f, 1) <= {9, 10, 11, 12}
        assert len(_code_lengths(f, fam != "dc_cats")) == 4   # (both sides of kDcFastBits = 9 / kFastBits = 11)
    elif f.tables == "long":
        assert _code_lengths(f, 0) | _code_lengths(f, 1) == {16}
    if fam == "ac_sizes":
        got = {(s, v, r) for (_, s, v, r) in levels}
        for s in range(1, 16):
            for v in cs._ends(s):
                assert (s, v, 0) in got and (s, v, 15) in got
        assert b"\xff\x00" in f.jpeg()[f.jpeg().find(b"\xff\xda"):]
        if f.tables == "long":
            assert f.huff[1][0xFF] == 16 and facts["max_symbol_bits"] == 31
            assert any(s == 15 and r == 15 for (_, s, _, r) in levels)
    elif fam == "dc_cats":
        cats = {cs.mag(d)[0]: f.huff[0][cs.mag(d)[0]] for d, _ in f.dus}
        assert set(cats) == set(range(16))
        assert {d for d, _ in f.dus} >= {v for s in range(1, 16) for v in cs._ends(s)}
        if f.tables == "long":
            assert cats[15] == 16 and facts["max_symbol_bits"] == 31
    elif fam == "dc_hostile":
        assert f.huff[0][16] == 2 and f.huff[0][17] == 16
        assert {cs.mag(d)[0] for d, _ in f.dus} >= {16, 17}
    elif fam == "q1_underflow":
        assert f.huff[1][0x00] == 16 and f.huff[0][15] == 16
        seen, short = _oracle_left_at_dc_codes(f)
        assert seen == facts["left_at_dc"]
        assert {n % 32 for n in seen} == set(range(32)), "the DC codes fall at every bit phase of a 32-bit word"
        if f.standard:
            assert short is None and facts["dry"] == 0 and min(seen) >= 32
        else:
            # the oracle's reader holds fewer than the 31 bits the symbol needs at a DC code: at every count a reader that
            # has just taken a 16-bit EOB can hold below 31
            assert short is not None and short < 31
            assert facts["underflow_left"] == set(range(16, 31))
            assert facts["dry"] > 0
    elif fam == "positions":
        landed = {p for (p, _, _, _) in levels}
        assert landed >= {31, 32, 46, 47, 62, 63} and max(landed) > 63
        zrls = [sum(1 for s in syms if s == cs.ZRL) for _, syms in f.dus]
        assert {1, 2, 3} <= set(zrls)
        assert any(len(syms) == 63 and cs.EOB not in syms for _, syms in f.dus)
        assert any(syms == [cs.EOB] for d, syms in f.dus if d)
        assert (pred[:, 31] != 0).any()
        # a ZRL from 46, 47 and 48: 17 positions on it ends the data unit from 47 and 48 and leaves 63 from 46; 16 on
        # (standard) only from 48
        zrl_from = {}
        for _, syms in f.dus:
            pos = 1
            for k, (r, s, _) in enumerate(syms):
                if (r, s) == (15, 0):
                    zrl_from.setdefault(pos, set()).add(k + 1 == len(syms))
                    pos += 16 if f.standard else 17
                elif (r, s) != (0, 0):
                    pos += r + 1
        assert zrl_from[46] == {False} and zrl_from[47] == {not f.standard} and zrl_from[48] == {True}
    elif fam == "run_size0":
        assert {r << 4 for _, syms in f.dus for (r, s, _) in syms if s == 0 and 0 < r < 15} == set(range(0x10, 0xF0, 0x10))
        assert any(s > 0 for (_, s, _, _) in levels)
    elif fam == "pairs":
        if f.tables == "short":
            assert f.huff[1] == {0x00: 1, 0x01: 2, 0x11: 3} and f.huff[0] == {0: 1, 1: 2}
        assert all(s == 1 for (_, s, _, _) in levels)
        assert sum(1 for _, syms in f.dus if syms == [cs.EOB]) >= 8
        sb = cs.symbol_bits(f)
        if f.tables == "short":
            # two symbols inside the walk tables' prefix: every symbol is 1..4 bits; pairs begin at every bit of a 32-bit
            # word, some straddle its end, and some EOB is a word's last bit with the next unit's DC code in the next word
            assert max(n + m for (_, _, n, m) in sb) <= 4
            assert {at % 32 for (sym, at, _, _) in sb if sym != "dc"} == set(range(32))
            assert any(at % 32 + n + m < 32 <= at % 32 + n + m + n2 + m2 for (_, at, n, m), (_, _, n2, m2) in zip(sb, sb[1:]))
            assert any(a[0] == 0 and a[1] % 32 == 31 and b[0] == "dc" for a, b in zip(sb, sb[1:]))
        else:
            assert min(n for (_, _, n, _) in sb) == 16   # every symbol escapes
    elif fam == "basis":
        q = int(f.qtable(0)[0])
        for pos in range(32):
            alone = pred[(np.count_nonzero(pred, axis=1) == 1) & (pred[:, pos] != 0), pos]
            assert set(alone.tolist()) >= {q, -q, 32767 * q, -32767 * q}, pos
        assert any(all(p >= 32 for (p, _, _, _) in _levels_of(f, syms)) and len(syms) > 30 for _, syms in f.dus)
    elif fam == "dc_sweep":
        for c in range(3):
            mine = [k for k in range(dpm) if f.comp_of_du[k] == c]
            vals = set(np.concatenate([pred[k::dpm, 0] for k in mine]).tolist())
            assert vals >= set(range(-1100, 1101)), c
    elif fam == "gamut":
        smp = cs.samples(pred).reshape(-1, dpm, 64)
        assert (smp == smp[:, :, :1]).all(), "flat data units"
        cb, cr, y = smp[:, dpm - 2, 0], smp[:, dpm - 1, 0], smp[:, 0, 0]
        for other in (0, 128, 255):
            assert set(cb[cr == other].tolist()) == set(range(256)) and set(cr[cb == other].tolist()) == set(range(256))
        assert set(smp[:, :dpm - 2, 0].ravel().tolist()) == {0, 1, 127, 128, 254, 255}
    elif fam == "saturated":
        assert (np.abs(pred[:, :32]) == 32767 * 255).sum() >= 16 * 32
        assert 32767 * 255 * 8 > 1 << 24
    elif fam == "dc_wrap":
        assert f.ri == 0 and f.mcus >= 300 and f.mcus_w == 1
        assert facts["max_pred_q"] >= 1 << 31
        y = cs.samples(pred).reshape(-1, dpm, 64)[:, 0, 0]
        flips = (f.mcus * (dpm - 2) * 32767 * 255) >> 31   # (the predictor x quantiser passes that many multiples of 2^31)
        assert flips >= 1 and set(y.tolist()) == {0, 255} and np.count_nonzero(np.diff(y.astype(int))) == flips
    elif fam == "cancel":
        mine = pred[pred[:, 1] != 0]   # (not the flat units that fill the last interval)
        amp = np.abs(mine[:, [1, 6]])
        assert len(mine) >= 60 * dpm and amp.min() > 300000 and amp[:, 0].min() > 1 << 19 and (mine[:, 0] == 4).all()
        mid = cs.samples(mine)
        assert ((mid == 128) | (mid == 129)).any(axis=(1, 2)).mean() > 0.9, "a column on the truncation boundary"
    elif fam == "texture":
        mid = cs.samples(pred)
        assert ((mid > 0) & (mid < 255)).mean() > 0.5, "most samples between the clamps"
    elif fam == "random_dense":
        assert len(f.huff[1]) == 242 and len(f.huff[0]) == 16
        assert {s for (_, s, _, _) in levels} == set(range(1, 16))
        assert len(f.dus) >= 3 * 63   # (a few hundred data units in 64 MCUs at the most)
        assert (facts["dry"] == 0) == (f.ri == 0)


def _levels_of(f, syms):
    g = cs.Frame("one", f.layout, 1, 1, [(0, syms)], f.huff, standard=f.standard)
    return _levels(g)


def test_families_and_layouts_are_all_there():
    seen = {(f.family, f.layout) for f in cs.cases()}
    for fam in cs.ENTROPY_FAMILIES + cs.ARITHMETIC_FAMILIES:
        for lay in cs.LAYOUTS:
            assert (fam, lay) in seen, (fam, lay)
    tabs = {(f.family, f.tables) for f in cs.cases() if f.layout == "422"}
    for fam in ("ac_sizes", "dc_cats", "run_size0"):
        assert {(fam, t) for t in ("short", "edge", "long")} <= tabs
    assert {f.ri for f in cs.cases() if f.family == "random_dense" and f.layout == "422"} == {0, 1, 3, 7}
    assert {f.standard for f in cs.cases() if f.family == "q1_underflow"} == {False, True}


# ---- sensitivity ------------------------------------------------------------------------------------------------------

# mutant -> the named cases that must tell it from the restatement (each was written for that clause)
CATCHES = {
    # (only `cancel` shows single roundings: elsewhere a sample's distance from the next integer is far above an ulp)
    "fma_rows": ("cancel/short/422/reference/dri1",),
    "round_nearest": ("dc_sweep/short/422/reference/dri1", "texture/edge/422/reference/dri4"),
    # (a lone coefficient beyond 16 bits clamps every sample either way; among 32 of them the unsaturated DC takes over)
    "saturate16": ("saturated/short/422/reference/dri1", "random_dense/long/422/reference"),
    "logical_shift": ("gamut/short/422/reference/dri1",),
    "cut31": ("positions/short/422/reference/dri4", "basis_q1/short/422/reference/dri1"),
    "cut33": ("positions/short/422/reference/dri4", "basis_q1/short/422/reference/dri1"),
    "zrl16": ("positions/short/422/reference/dri4", "basis_q1/short/422/reference/dri1"),
}


@pytest.mark.parametrize("mutant", cs.MUTANTS)
def test_every_mutant_is_caught_by_a_named_case(mutant):
    assert set(CATCHES) == set(cs.MUTANTS)
    for name in CATCHES[mutant]:
        f = cs.case(name)
        want = decoded(f)[0]
        got = cs.expectation(f, mutant)
        assert np.array_equal(cs.expectation(f), want)
        assert not np.array_equal(got, want), f"{name} cannot tell the mutant {mutant}"
