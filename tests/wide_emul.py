"""What the emulation modules of the seven stand-alone drivers (tests/emul_reduced, _planes, _gray, _crop, _crop_regions,
_scaled, _levels) share for the frames whose Huffman tables outgrow their share of LDS (cs.wide_cases, gs.wide_cases): which
frames a driver runs, what it must report of its staging (tests/emul/lut_budget.h: "luts in_lds=N l2_staged=N fast=0|1" on
stderr, a line per image), and the control -- `beyond`, which tells the body that everything is staged while the planner's
12288 entries are: every regime-C frame must then differ from its expectation, or it never looks up beyond the boundary."""
import re

import coef_stream as cs
import gray_stream as gs

PLAN, BEYOND = ("plan",), ("plan", "beyond")
REPORTS = []   # the reports of the last run: [(in_lds, l2_staged, fast)]


def note(stderr):
    REPORTS[:] = [tuple(int(v) for v in m) for m in re.findall(r"^luts in_lds=(\d+) l2_staged=(\d+) fast=([01])$", stderr, re.M)]


def layout_of(f):
    return "gray" if isinstance(f, gs.GrayFrame) else f.layout


def frames(layouts=("422", "444", "440", "420", "gray"), families=None):
    out = [f for f in cs.wide_cases() + gs.wide_cases() if layout_of(f) in layouts and (families is None or f.family in families)]
    assert {cs.table_regime(f)["regime"] for f in out} == set("ABC")
    return out


def frame(name):
    return next(f for f in cs.wide_cases() + gs.wide_cases() if f.name == name)


def regime(f):
    return cs.table_regime(f)["regime"]


def planned(f):
    """(entries staged behind L1, what the body is told of them, whether the fast entropy mode is on) as the planner has it:
    runtime.cpp: staged_lut_entries = L2 + the two direct AC tables; kernels.hip: plan_huffman stages 12288 at the most."""
    l2 = cs.table_regime(f)["entries"]
    in_lds = min(l2 + 2 * cs.FAST_ENTRIES, cs.LDS_SHARE)
    return in_lds, min(in_lds, l2 + 2 * cs.FAST_ENTRIES), int(fast_mode(f))


def fast_mode(f):
    """Regime A; and never a grayscale image: its two absent components name no direct table (desc.cpp: fast_table = 2), and
    fast_tables_usable asks all three."""
    return regime(f) == "A" and layout_of(f) != "gray"


def check_plan(f, at=0):
    """The run before this was at the planner's budget: the driver's report is the planner's arithmetic, and the fast mode is
    on in regime A alone."""
    assert REPORTS and REPORTS[at] == planned(f), (f.name, REPORTS, planned(f))
    assert REPORTS[at][2] == fast_mode(f), f.name


def check_control(f, differing):
    """The run before this was the control's."""
    assert REPORTS and REPORTS[0][1] == 0xFFFFFFFF and REPORTS[0][0] == planned(f)[0] and REPORTS[0][2] == 0, (f.name, REPORTS)
    assert differing, f"{f.name}: decodes to its expectation with L2 lookups beyond the staged entries going to LDS: it never looks up there"


SAMPLINGS = ("422", "444", "440", "420", "gray")


def same_size_batches(layout):
    """Two batches of images of one size in the layout, regimes mixed, the largest tables neither first nor last: the
    `ac_sizes` frames (A, B and C) and the `random_dense` frames of 65 intervals (B and C)."""
    mine = frames((layout,))
    out = []
    for family, kinds in (("ac_sizes", ("wide_c", "wide_a", "full", "wide_b", "wide_b48")), ("random_dense", ("wide_b", "wide_c2", "full", "wide_b48", "wide_c"))):
        batch = [next(f for f in mine if f.family == family and f.tables == k and f.mcus <= 65) for k in kinds]
        assert len({(f.w, f.h) for f in batch}) == 1 and {regime(f) for f in batch} >= set("BC")
        out.append(batch)
    assert {regime(f) for f in out[0]} == set("ABC")
    return out
