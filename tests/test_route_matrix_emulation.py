"""The route matrix (tests/route_matrix.py) through every emulated kernel body that applies (tests/emul: the gfx950 bodies
compiled for the host with ASan + UBSan), with the output tight and padded as the runtime allocates it, against the
oracle.  Each body meets every width class and every DRI class of its layout in both entropy modes; the coverage is
asserted inside the test that ran the cells, so that no selection of tests can leave a cell empty unnoticed."""
import collections

import numpy as np
import pytest

import route_matrix as rm
from test_kernel_emulation import _run, runner  # noqa: F401  (runner: the module fixture that builds the emulator)

# (EMUL_FUSED, what the emulator runs) per layout, and the knobs each body cycles through cell by cell
BODIES_422 = {
    "fused": (1, [{}]),
    "pair": (2, [{}]),
    "two_kernel": (3, [{}]),
    "split": (0, [{}]),
    "coop": (5, [dict(window=0, coop_passes=4), dict(window=0, coop_passes=1)]),
    "stream": (7, [dict(window=16), dict(window=3)]),
    "walk": (8, [dict(window=40, below=20), dict(window=12, below=3, chunk=2), dict(window=2, below=1),
                 dict(window=64, below=30, chunk=5)]),
}
BODIES_LAYOUT = {
    "records": (4, [{}]),
    "fused_layout": (6, [dict(waves=3, window=300)]),
    "layout_stream": (6, [dict(waves=2, layout_rows=24, stage=8, below=24), dict(waves=2, layout_rows=3, stage=8, below=2),
                          dict(waves=2, layout_rows=6, stage=0xF, below=3)]),
    "singles": (6, [dict(waves=3, window=300, singles=True)]),   # (odd restart intervals only)
}
# a body that declines an image (the emulator says it does not qualify) -- where that is expected
DECLINES = {("coop", "none"), ("coop", "257"), ("coop", "beyond")}


def _bodies(layout):
    return BODIES_422 if layout == "422" else BODIES_LAYOUT


@pytest.mark.parametrize("layout", sorted(rm.LAYOUTS))
def test_route_matrix_through_the_emulated_bodies(runner, tmp_path, layout):   # noqa: F811
    cells = rm.cells(layout)
    seen = collections.Counter()
    bad = []
    for k, cell in enumerate(cells):
        jpeg = cell.jpeg()
        want = rm.want(cell)
        small = k < len(rm.small_cells(layout))
        for body, (fused, knobs) in _bodies(layout).items():
            r = cell.ri or cell.mcus
            if body == "singles" and (r % 2 == 0 or layout == "420"):
                continue
            kw = dict(knobs[k % len(knobs)], standard=cell.standard)
            # (tight and padded both where the edge cuts an MCU of a small cell; else one of them, in turn)
            ragged = small and (cell.w % cell.mcu[0] or cell.h % cell.mcu[1])
            for padded in ((False, True) if ragged else ((k + len(body)) % 2 == 1,)):
                try:
                    got = _run(runner, tmp_path, jpeg, fused, padded=padded, **kw)
                except AssertionError as e:   # (the emulator failed: a sanitizer's report -- name the cell with it)
                    bad.append(f"{body} padded={padded} {kw}: {cell.name}: emulator failed: {str(e)[-600:]}")
                    continue
                if got is None:
                    assert (body, cell.dri_class) in DECLINES or (body == "coop" and cell.mcus > 256), (body, cell.name)
                    continue
                seen[(body, cell.width_class, cell.dri_class, cell.entropy)] += 1
                if not np.array_equal(got, want):
                    diff = (got != want).any(axis=2) if got.shape == want.shape else None
                    ys, xs = np.nonzero(diff) if diff is not None else ([0], [0])
                    bad.append(f"{body} padded={padded} {kw}: {cell.name}: "
                               f"{int(diff.sum()) if diff is not None else 'shape'} pixels differ, first at x={xs[0]} y={ys[0]}")
    assert not bad, f"{len(bad)} decodes differ from the oracle:\n" + "\n".join(bad[:40])
    # coverage: every body x every width class x every DRI class of this layout's cells, both entropy modes
    widths = {c.width_class for c in cells}
    dris = {c.dri_class for c in cells}
    empty = []
    for body in _bodies(layout):
        got_w = {w for (b, w, _, _) in seen if b == body}
        got_d = {d for (b, _, d, _) in seen if b == body}
        got_e = {e for (b, _, _, e) in seen if b == body}
        need_d = {d for d in dris if (body, d) not in DECLINES}
        if body == "singles":
            need_d = {c.dri_class for c in cells if (c.ri or c.mcus) % 2}
        need_w = widths if body != "singles" else {c.width_class for c in cells if (c.ri or c.mcus) % 2}
        empty += [(body, "width", w) for w in sorted(need_w - got_w)]
        empty += [(body, "dri", d) for d in sorted(need_d - got_d)]
        empty += [(body, "entropy", e) for e in sorted({"reference", "standard"} - got_e)]
    if layout == "420":
        empty = [e for e in empty if e[0] != "singles"]
    print(f"route matrix {layout}: {sum(seen.values())} emulated decodes;",
          {b: sum(v for (bb, *_), v in seen.items() if bb == b) for b in _bodies(layout)})
    assert not empty, f"emulated cells without a decode: {empty}"


def test_route_matrix_extent_limit_matches_the_oracle():
    """EXTREME + 1 pixels on either axis: the oracle's parser and the library's reject the frame alike; EXTREME itself
    decodes (tests above)."""
    import compeg_amd as ca   # (parsing only: no device)
    from oracle import oracle as orc
    for layout, w, h, jpeg in rm.rejected_frames():
        with pytest.raises(orc.OracleError):
            orc.ImageData(jpeg, allow_sampling=True)
        with pytest.raises(ca.Error) as e:
            ca.ImageData(jpeg, allow_sampling=layout != "422")
        assert "16-bit" in str(e.value), (layout, w, h, str(e.value))
