"""The coefficient-level frames of tests/coef_stream.py through the emulated kernel bodies (tests/emul: the gfx950
bodies compiled for the host with ASan + UBSan, run lane by lane), by the route list of test_kernel_emulation._check:
fused, paired, two-kernel, split, streamed windows, cooperative with 4 / 2 / 1 rounds, walk + lane-per-MCU at its four
row settings; the records pipeline and the layout kernels (whole windows, single-MCU form, streamed) for 4:4:4, 4:4:0
and 4:2:0.  Every route's pixels equal the oracle's bit for bit, and the entropy records the runner leaves behind hold
what the writer predicted.

A route may say "does not qualify" only where must_not_qualify() says so: the cooperative kernel and the walk for
`dc_hostile` (a DC category above 15: the direct tables cannot hold it), the cooperative kernel for the two strips
(one interval of more than kCoopMaxRestart = 256 MCUs).  Everything else must run on every route."""
import numpy as np
import pytest

import coef_stream as cs
from oracle import oracle as orc
from test_kernel_emulation import STATS, _run, runner  # noqa: F401  (the fixture builds tests/emul)

NAMES = [f.name for f in cs.cases()]


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
