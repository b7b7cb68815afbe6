"""The levels decode (quantised DCT coefficients as int16 blocks) where no device is needed (include/compeg_hip.h, "Levels
decode").

compeg_levels_shape against hand-computed layouts and against its restatement (tests/levels_stream.py), the refusals that
need no object, quant_table in both orders against the frames' own tables and a golden file's DQT; then the expectation
itself: for every frame of tests/coef_stream.py (and the grayscale ones), wrap32(level x q) at positions 0..31 is what the
oracle's entropy pass leaves in its coefficient buffer -- position 0 where the DC predictor fits 16 bits, its low 16 bits
otherwise -- and three mutants of the expectation (Q3 acting, a ZRL of the other length, the natural-order permutation
applied twice) are each told apart by a named frame.  (What needs a decoder or a batch needs a device:
tests/test_gpu_levels.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import compeg_amd as ca
import coef_stream as cs
import gray_stream as gs
import levels_stream as ls
import planes_stream as ps
import reduced_stream as rs
from compeg_amd._lib import LevelsLayout, LevelsSpec, lib
from conftest import GOLDEN

K = 128   # bytes of a block

# (w, h, components, (hs, vs)) -> per component (offset, blocks_w, blocks_h, width_in_blocks, height_in_blocks), total: by hand
BY_HAND = {
    (1, 1, 3, (2, 1)): (((0, 2, 1, 1, 1), (2 * K, 1, 1, 1, 1), (3 * K, 1, 1, 1, 1)), 4 * K),
    (1, 1, 3, (1, 1)): (((0, 1, 1, 1, 1), (K, 1, 1, 1, 1), (2 * K, 1, 1, 1, 1)), 3 * K),
    (1, 1, 3, (1, 2)): (((0, 1, 2, 1, 1), (2 * K, 1, 1, 1, 1), (3 * K, 1, 1, 1, 1)), 4 * K),
    (1, 1, 3, (2, 2)): (((0, 2, 2, 1, 1), (4 * K, 1, 1, 1, 1), (5 * K, 1, 1, 1, 1)), 6 * K),
    (1, 1, 1, (1, 1)): (((0, 1, 1, 1, 1),), K),
    # 324 x 70: 21 x 9 MCUs of 16 x 8; 41 x 9 of 8 x 8; 41 x 5 of 8 x 16; 21 x 5 of 16 x 16
    (324, 70, 3, (2, 1)): (((0, 42, 9, 41, 9), (378 * K, 21, 9, 21, 9), (567 * K, 21, 9, 21, 9)), 756 * K),
    (324, 70, 3, (1, 1)): (((0, 41, 9, 41, 9), (369 * K, 41, 9, 41, 9), (738 * K, 41, 9, 41, 9)), 1107 * K),
    (324, 70, 3, (1, 2)): (((0, 41, 10, 41, 9), (410 * K, 41, 5, 41, 5), (615 * K, 41, 5, 41, 5)), 820 * K),
    (324, 70, 3, (2, 2)): (((0, 42, 10, 41, 9), (420 * K, 21, 5, 21, 5), (525 * K, 21, 5, 21, 5)), 630 * K),
    (324, 70, 1, (1, 1)): (((0, 41, 9, 41, 9),), 369 * K),
    # 3840 x 2160: 240 x 270, 480 x 270, 480 x 135, 240 x 135 MCUs
    (3840, 2160, 3, (2, 1)): (((0, 480, 270, 480, 270), (129600 * K, 240, 270, 240, 270), (194400 * K, 240, 270, 240, 270)), 259200 * K),
    (3840, 2160, 3, (1, 1)): (((0, 480, 270, 480, 270), (129600 * K, 480, 270, 480, 270), (259200 * K, 480, 270, 480, 270)), 388800 * K),
    (3840, 2160, 3, (1, 2)): (((0, 480, 270, 480, 270), (129600 * K, 480, 135, 480, 135), (194400 * K, 480, 135, 480, 135)), 259200 * K),
    (3840, 2160, 3, (2, 2)): (((0, 480, 270, 480, 270), (129600 * K, 240, 135, 240, 135), (162000 * K, 240, 135, 240, 135)), 194400 * K),
    (3840, 2160, 1, (1, 1)): (((0, 480, 270, 480, 270),), 129600 * K),
}
KEYS = ("offset", "blocks_w", "blocks_h", "width_in_blocks", "height_in_blocks")


@pytest.mark.parametrize("case", list(BY_HAND), ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-{c[3][0]}x{c[3][1]}")
def test_shape_by_hand(case):
    w, h, comps, sampling = case
    want_comps, want_total = BY_HAND[case]
    assert want_total == 33177600 or (w, h, sampling) != (3840, 2160, (2, 1))   # (the 33 MB of a 4K 4:2:2 frame: its RGBA's bytes)
    for order in ls.ORDERS:
        got, total = ca.levels_shape(w, h, sampling, comps, order)
        assert total == want_total and len(got) == comps
        assert tuple(tuple(c[k] for k in KEYS) for c in got) == want_comps
    mine, mine_total = ls.shape(w, h, comps, *sampling)
    assert (mine, mine_total) == (got, total)


def test_shape_against_its_restatement_on_many_extents():
    rng = np.random.default_rng(4)
    for _ in range(300):
        w, h = int(rng.integers(1, 70000)), int(rng.integers(1, 70000))
        for comps, sampling in ((3, (2, 1)), (3, (1, 1)), (3, (1, 2)), (3, (2, 2)), (1, (1, 1))):
            assert ca.levels_shape(w, h, sampling, comps) == ls.shape(w, h, comps, *sampling)


def test_the_layout_struct_is_the_headers():
    assert C.sizeof(LevelsSpec) == 16 and C.sizeof(LevelsLayout) == 88
    lay = LevelsLayout()
    lay.reserved = 7
    ca.check(lib.compeg_levels_shape(C.byref(LevelsSpec()), 17, 9, 1, 1, 1, C.byref(lay)))
    assert lay.reserved == 0 and lay.components == 1 and lay.blocks_w[1] == lay.blocks_h[2] == lay.offset[1] == 0 and lay.total_bytes == 3 * 2 * K


class Raises:
    def __init__(self, code, *words):
        self.code, self.words = code, words

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        assert kind is not None and issubclass(kind, ca.Error), f"no error where {self.words} was expected"
        assert e.code == self.code and all(w in str(e) for w in self.words) and "COMPEG_" not in str(e), (e.code, str(e))
        return True


def test_refusals_without_a_device():
    lay = LevelsLayout()
    lay.total_bytes = 99

    def shape(spec, w=16, h=8, comps=3, hs=2, vs=1, out=lay):
        ca.check(lib.compeg_levels_shape(C.byref(spec) if spec is not None else None, w, h, comps, hs, vs, C.byref(out) if out is not None else None))

    for k in range(3):
        spec = LevelsSpec()
        spec.reserved[k] = 1
        with Raises(ca.E_INVALID_ARG, "reserved must be 0"):
            shape(spec)
    spec = LevelsSpec()
    spec.order = 2
    with Raises(ca.E_INVALID_ARG, "order 2", "zigzag", "natural"):
        shape(spec)
    with Raises(ca.E_INVALID_ARG, "order 9"):
        ca.levels_shape(16, 8, order=9)
    with pytest.raises(ca.Error, match="unknown levels order"):
        ca.levels_shape(16, 8, order="raster")
    for hs, vs in ((3, 1), (1, 3), (4, 2), (0, 1), (2, 0)):
        with Raises(ca.E_INVALID_ARG, f"luma sampling {hs}x{vs}"):
            shape(LevelsSpec(), hs=hs, vs=vs)
    with Raises(ca.E_INVALID_ARG, "luma sampling 2x1", "grayscale"):
        shape(LevelsSpec(), comps=1)
    with Raises(ca.E_INVALID_ARG, "2 components"):
        shape(LevelsSpec(), comps=2)
    with Raises(ca.E_INVALID_ARG, "no pixels"):
        shape(LevelsSpec(), w=0)
    with Raises(ca.E_INVALID_ARG, "spec is NULL"):
        shape(None)
    with Raises(ca.E_INVALID_ARG, "layout is NULL"):
        shape(LevelsSpec(), out=None)
    with Raises(ca.E_INVALID_ARG, "overflow", "4294967295x4294967295"):
        shape(LevelsSpec(), w=0xFFFFFFFF, h=0xFFFFFFFF, hs=1, vs=1)
    assert lay.total_bytes == 99, "nothing is written on failure"
    # the largest extent a JPEG header can state is far inside
    assert ca.levels_shape(65535, 65535, (1, 1))[1] == 3 * 8192 * 8192 * K


# ---- quant_table -----------------------------------------------------------------------------------------------------

def test_quant_table_of_the_frames_own_tables():
    for f in (cs.texture(), cs.texture("420"), cs.random_dense(3, "444"), cs.dc_wrap("440"), gs.case(gs.cases()[0].name)):
        img = ca.ImageData(f.jpeg(), **f.image_kw())
        comps = ps.sampling_of(f)[0]
        for c in range(comps):
            q = f.qtable(f.sel[c][2])
            got = img.quant_table(c)
            assert got.dtype == np.uint16 and got.shape == (64,) and np.array_equal(got, q), (f.name, c)
            assert np.array_equal(img.quant_table(c, "zigzag"), q)
            nat = img.quant_table(c, "natural")
            assert np.array_equal(nat, q[cs.ZIGZAG]) and np.array_equal(nat[np.argsort(cs.ZIGZAG)], q), (f.name, c)
        with Raises(ca.E_INVALID_ARG, f"component {comps}", f"has {comps}"):
            img.quant_table(comps)
        with Raises(ca.E_INVALID_ARG, "order 2"):
            img.quant_table(0, 2)
    f = cs.texture()
    assert not np.array_equal(f.qtable(0), f.qtable(0)[cs.ZIGZAG]), "the two orders of this table must differ"


def _dqt(jpeg):
    """{table id: 64 values in the file's (zig-zag) order} of a file's 8-bit DQT segments."""
    out, at = {}, 2
    while at < len(jpeg) and jpeg[at] == 0xFF and jpeg[at + 1] != 0xDA:
        n = int.from_bytes(jpeg[at + 2:at + 4], "big")
        if jpeg[at + 1] == 0xDB:
            seg = jpeg[at + 4:at + 2 + n]
            for k in range(len(seg) // 65):
                out[seg[65 * k] & 15] = np.frombuffer(seg[65 * k + 1:65 * k + 65], dtype=np.uint8).astype(np.uint16)
        at += 2 + n
    return out


def test_quant_table_of_a_golden_files_dqt():
    files = ps.golden_files(ca, GOLDEN)
    assert files
    seen = 0
    for name, j, kw in files:
        tables, img = _dqt(j), ca.ImageData(j, **kw)
        sof = j.index(b"\xff\xc0")
        for c in range(img.components()):
            tq = j[sof + 10 + 3 * c + 2]
            assert np.array_equal(img.quant_table(c), tables[tq]), (name, c)
            assert np.array_equal(img.quant_table(c, "natural"), tables[tq][cs.ZIGZAG]), (name, c)
            seen += 1
    assert seen >= 6


# ---- the expectation against the oracle ------------------------------------------------------------------------------

def _all_frames():
    return list(cs.cases()) + [f for f in gs.cases() if "/w5" in f.name or f.family == "random_gray"][:24]


def _frame(name):
    return gs.case(name) if "/gray/" in name else cs.case(name)


@pytest.mark.parametrize("name", [f.name for f in _all_frames()])
def test_levels_times_quantiser_are_the_oracles_coefficients(name):
    f = _frame(name)
    coef = rs.file_coefficients(ca, f.jpeg(), **f.image_kw())[0]
    levels = ls.frame_levels(f)
    assert levels.dtype == np.int16 and levels.shape == coef.shape
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    q = np.stack([f.qtable(f.sel[comps[n % dpm]][2]) for n in range(dpm)])[np.arange(levels.shape[0]) % dpm]
    ac = ls.dequantised_low(levels, np.ones(64), "zigzag").astype(np.int64) * q[:, :32]
    ac = (((ac + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).astype(np.int32)
    assert np.array_equal(ac[:, 1:], coef[:, 1:32]), f"{name}: AC positions 1..31"
    pred = ls.predictors(f).astype(np.int64)
    fits = (pred >= -32768) & (pred <= 32767)
    assert np.array_equal(ac[fits, 0], coef[fits, 0]), f"{name}: DC where the predictor fits 16 bits"
    assert np.array_equal(levels[:, 0], ls.low16(pred)), f"{name}: position 0 is the predictor's low 16 bits"
    want_dc = (((pred * q[:, 0] + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).astype(np.int32)
    assert np.array_equal(want_dc, coef[:, 0]), f"{name}: the predictor itself against the oracle's DC"
    if f.family == "dc_wrap":
        assert not fits.all(), "dc_wrap's predictor must leave 16 bits"
    # the natural order through the same check
    nat = ls.ordered(levels, "natural")
    assert np.array_equal(ls.dequantised_low(nat, np.ones(64), "natural"), ls.dequantised_low(levels, np.ones(64), "zigzag"))


@pytest.mark.parametrize("layout", list(ps.SAMPLINGS))
def test_short_frames_by_the_reader_are_the_oracles(layout):
    """The frames with MCUs behind their last complete interval: reader_levels over the oracle's preprocessed scan, against the
    oracle's coefficients at 0..31; and on a whole frame reader_levels is frame_levels."""
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    f = ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3)
    levels = ls.any_frame_levels(f, ca)
    coef = rs.file_coefficients(ca, f.jpeg(), **f.image_kw())[0]
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    q = np.stack([f.qtable(f.sel[comps[n % dpm]][2]) for n in range(dpm)])[np.arange(levels.shape[0]) % dpm]
    assert levels.shape == coef.shape and levels.shape[0] == 8 * dpm
    assert np.array_equal(levels[:, :32].astype(np.int64) * q[:, :32], coef[:, :32])
    g = ps.sized(layout, 324, 70, 3 if layout != "440" else 5, seed=5)
    assert np.array_equal(ls.reader_levels(g, *ls.scan_words(ca, g.jpeg(), **g.image_kw())), ls.frame_levels(g))


# ---- the mutants -----------------------------------------------------------------------------------------------------

# mutant -> the frame that tells it from the expectation
TELLS = {"cut32": "positions/short/422/reference/dri4", "zrl16": "positions/long/422/standard/dri4", "natural_twice": "random_dense/long/422/reference/dri3"}


@pytest.mark.parametrize("mutant", ls.MUTANTS)
def test_mutants_of_the_expectation_are_told_apart(mutant):
    f = cs.case(TELLS[mutant])
    for order in ("natural",) if mutant == "natural_twice" else ls.ORDERS:
        good, bad = ls.frame_destination(f, order), ls.frame_destination(f, order, mutant=mutant)
        assert good.shape == bad.shape and not np.array_equal(good, bad), f"{mutant} is not told apart by {f.name} in {order} order"
    if mutant == "cut32":
        a, b = ls.frame_levels(f), ls.frame_levels(f, "cut32")
        assert np.array_equal(a[:, :32], b[:, :32]) and a[:, 32:].any() and not b[:, 32:].any()


def test_every_sampling_has_chosen_levels_beyond_31():
    for layout in ("422", "444", "440", "420"):
        frames = [f for f in cs.cases() if f.layout == layout and f.family in ("positions", "random_dense", "run_size0")]
        assert any(ls.frame_levels(f)[:, 32:].any() for f in frames), layout
    assert any(ls.frame_levels(f)[:, 32:].any() for f in gs.cases())


def test_scatter_and_views_are_inverse():
    f = cs.random_dense(3, "420")
    levels = ls.frame_levels(f)
    mw, mh, comps, hs, vs = ls.frame_geometry(f)
    buf = ls.destination(levels, mw, mh, comps, hs, vs)
    y, cb, cr = ls.views(buf, f.w, f.h, comps, hs, vs)
    dpm = f.dus_per_mcu
    # MCU 1's four luma units lie at blocks (0, 2), (0, 3), (1, 2), (1, 3); its chroma at (0, 1)
    assert np.array_equal(y[0, 2], levels[dpm]) and np.array_equal(y[0, 3], levels[dpm + 1]) and np.array_equal(y[1, 2], levels[dpm + 2])
    assert np.array_equal(y[1, 3], levels[dpm + 3]) and np.array_equal(cb[0, 1], levels[dpm + 4]) and np.array_equal(cr[0, 1], levels[dpm + 5])
    assert os.path.isdir(GOLDEN)
