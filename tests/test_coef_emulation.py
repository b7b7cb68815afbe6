"""The coefficient-level frames of tests/coef_stream.py through the emulated kernel bodies (tests/emul: the gfx950
bodies compiled for the host with ASan + UBSan, run lane by lane), by the route list of test_kernel_emulation._check:
fused, paired, two-kernel, split, streamed windows, cooperative with 4 / 2 / 1 rounds, walk + lane-per-MCU at its four
row settings; the records pipeline and the layout kernels (whole windows, single-MCU form, streamed) for 4:4:4, 4:4:0
and 4:2:0.  Every route's pixels equal the oracle's bit for bit, and the entropy records the runner leaves behind hold
what the writer predicted.

A route may say "does not qualify" only where must_not_qualify() says so: the cooperative kernel and the walk for
`dc_hostile` (a DC category above 15: the direct tables cannot hold it), the cooperative kernel for the two strips
(one interval of more than kCoopMaxRestart = 256 MCUs).  Everything else must run on every route.

cs.wide_cases() -- Huffman tables that outgrow their share of LDS (cs.table_regime) -- run the same routes twice: with
the entries the planners stage, min(staged_lut_entries, 12288) behind L1 (runtime.cpp, kernels.hip: plan_huffman), where
regime B has the direct tables in part and regime C reads L2 from global memory beyond entry 12288, and with everything
staged.  (The cooperative kernel stages all its tables whatever the budget, as plan_coop does.)  The walk + lane-per-MCU
route stages what plan_walk stages -- the share's entries and the direct DC tables -- whatever `l2` is given, and
refuses tables beyond the share as the dispatch does (runtime.cpp: walk_luts_fit): its walk reads the direct tables
from LDS alone.  A control walks such tables all the same and must get wrong pixels: what the card showed before the
dispatch kept them off the route."""
import numpy as np
import pytest

import coef_stream as cs
from oracle import oracle as orc
from test_kernel_emulation import STATS, _run, runner  # noqa: F401  (the fixture builds tests/emul)

NAMES = [f.name for f in cs.cases()]
WIDE = [f.name for f in cs.wide_cases()]


def must_not_qualify(f):
    """The routes of 4:2:2 that refuse the frame (all others must take it)."""
    if f.layout != "422":
        return set()   # (the layouts' kernels take every frame of their layout)
    if f.family == "dc_hostile":
        return {"coop", "walk"}
    if f.ri == 0 and f.mcus > 256:
        return {"coop"}
    return set()


def _routes(f):
    """(route, what to call it, _run's arguments)."""
    if f.layout == "422":
        out = [(n, n, dict(fused=k)) for n, k in (("fused", 1), ("pair", 2), ("two_kernel", 3), ("split", 0))]
        out += [("stream", f"streamed window, {rows} rows", dict(fused=7, window=rows)) for rows in (16, 3)]
        out += [("coop", f"cooperative, {p} round(s)", dict(fused=5, window=0, coop_passes=p)) for p in (4, 2, 1)]
        out += [("walk", f"walk + lane-per-MCU, {rows} rows", dict(fused=8, window=rows, below=below, chunk=chunk))
                for rows, below, chunk in ((40, 20, 1), (12, 3, 2), (2, 1, 1), (64, 30, 5))]
        return out
    out = [("records", "records", dict(fused=4)), ("layout", "layout kernel", dict(fused=6, waves=3, window=300))]
    if f.interval % 2:
        out.append(("layout", "layout kernel, single MCUs", dict(fused=6, waves=3, window=300, singles=True)))
    out += [("layout", f"layout kernel streamed, {rows} rows", dict(fused=6, waves=2, layout_rows=rows, stage=stage, below=below))
            for rows, stage, below in ((24, 8, 24), (3, 8, 2), (6, 0xf, 3))]
    return out


def _check_records(f, tmp_path, pred, what):
    """out.dc holds a product -- predictor x quantiser, wrapped to 32 bits, what the reference stores at position 0;
    out.ac holds levels, 16 bits each at zig-zag 1..31 (idct_data_unit multiplies them by the quantiser: |level| < 2^15
    and q < 2^8, so level x q is exact and below 2^23, nothing to wrap), slot 0 unused."""
    dc = np.fromfile(tmp_path / "dc", dtype=np.int32)
    ac = np.fromfile(tmp_path / "ac", dtype=np.int16).reshape(-1, cs.RETAINED).astype(np.int64)
    assert dc.size == ac.shape[0] == pred.shape[0], what
    assert np.array_equal(dc, pred[:, 0]), f"{what}: DC records are not the wrapped products"
    q = np.stack([f.qtable(f.sel[c][2])[:cs.RETAINED] for c in f.comp_of_du] * (dc.size // f.dus_per_mcu))
    assert np.abs(ac * q).max() < 1 << 23
    assert np.array_equal((ac * q)[:, 1:], pred[:, 1:cs.RETAINED]), f"{what}: AC records x quantiser are not the predicted products"


@pytest.mark.parametrize("name", NAMES)
def test_emulated_routes_on_coefficient_frames(runner, tmp_path, name):
    f = cs.case(name)
    want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    pred = cs.predict(f)
    refused = set()
    for route, what, kw in _routes(f):
        # (_run adds the runner's rare-path counters to test_kernel_emulation.STATS, which that module's own cases have to
        # fill -- test_emulated_rare_paths_were_reached: these frames' counts are taken out again)
        kept = dict(STATS)
        try:
            got = _run(runner, tmp_path, f.jpeg(), standard=f.standard, **kw)
        finally:
            STATS.clear()
            STATS.update(kept)
        if got is None:
            refused.add(route)
            continue
        assert route not in must_not_qualify(f), f"{name}: {what} took a frame it has to refuse"
        assert got.shape == want.shape and np.array_equal(got, want), \
            f"{name}: {what}: {int((got != want).any(axis=2).sum())} pixels differ"
        if route in ("two_kernel", "split"):
            _check_records(f, tmp_path, pred, f"{name}: {what}")
    assert refused == must_not_qualify(f), f"{name}: refused by {sorted(refused)}, expected {sorted(must_not_qualify(f))}"


def staged_lut_entries(f):
    """runtime.cpp: staged_lut_entries -- L2, padded to a dword, and the two direct AC tables."""
    return (cs.table_regime(f)["entries"] + 1 & ~1) + 2 * cs.FAST_ENTRIES


@pytest.mark.parametrize("name", WIDE)
def test_emulated_routes_on_wide_table_frames(runner, tmp_path, name):
    f = cs.wide_case(name)
    want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    budgets = sorted({min(staged_lut_entries(f), cs.LDS_SHARE), staged_lut_entries(f)})
    assert len(budgets) == (1 if cs.table_regime(f)["regime"] == "A" else 2)
    for l2 in budgets:
        refused = set()
        for route, what, kw in _routes(f):
            if route == "coop" and l2 != budgets[0]:
                continue   # (the runner stages all of the cooperative kernel's tables: one run)
            kept = dict(STATS)
            try:
                got = _run(runner, tmp_path, f.jpeg(), standard=f.standard, l2=l2, **kw)
            finally:
                STATS.clear()
                STATS.update(kept)
            if got is None:
                refused.add(route)
                continue
            assert got.shape == want.shape and np.array_equal(got, want), \
                f"{name}: {what}, {l2} entries staged: {int((got != want).any(axis=2).sum())} pixels differ"
        expected = (must_not_qualify(f) | ({"walk"} if f.layout == "422" and cs.table_regime(f)["regime"] != "A" else set())) - (set() if l2 == budgets[0] else {"coop"})
        assert refused == expected, f"{name}: refused by {sorted(refused)}, expected {sorted(expected)}"


@pytest.mark.parametrize("name", ["positions/wide_b/422/standard/dri4", "positions/wide_c/422/standard/dri4", "random_dense_strip/wide_c/422/reference"])
def test_the_walk_cannot_take_tables_beyond_the_lds_share(runner, tmp_path, name):
    """Why walk_luts_fit exists: at plan_walk's budget the direct AC and DC tables of a regime-B or -C image are not (all)
    in LDS, and the walk reads them nowhere else.  Walked all the same, these frames decode wrong -- as they did on the
    card, through `walk_mcu`, before the dispatch kept them off the route; as the runtime runs it, the route refuses them."""
    f = cs.wide_case(name)
    want = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    kept = dict(STATS)
    try:
        assert _run(runner, tmp_path, f.jpeg(), 8, window=40, below=20, standard=f.standard) is None
        got = _run(runner, tmp_path, f.jpeg(), 8, window=40, below=20, standard=f.standard, walk_any_tables=True)
    finally:
        STATS.clear()
        STATS.update(kept)
    assert got is not None and got.shape == want.shape and not np.array_equal(got, want), f"{name}: the walk decodes it right without its direct tables"
