"""Huffman tables that outgrow their share of LDS, on the card: every RGBA route with the frames of cs.wide_cases() and
gs.wide_cases() (tests/coef_stream.py: WIDE_KINDS, table_regime).  Regime A: L2 and both direct AC tables staged, the
fast entropy mode on.  B: all of L2 staged, the direct tables in part, the fast mode off.  C: L2 lookups at and beyond
entry 12288 come from global memory.  The cases live in tests/gpu_wide_tables_worker.py and run in one process of their
own that imports torch before the library and stops at the first error of the device; each case is reported here, every
decode is compared with the oracle over the whole output (grayscale: gs.expectation), and `last_kernel()` of every decode
is held against the tables below -- what the MI355X answered when the cases were written.

Routes regime-C frames reached on the card (the module's route counter, test_every_route_decodes_regime_c_frames, prints
the numbers): `coop_team` (Decoder 4:2:2; batches `coop`, `many`, the uniform batches), `pair` (batch `pair`, the mixed
A/B/C batches of 4:2:2, laboratory knob set 2), `fused_stream` (Decoder: the dense strip, the extension layouts with
device preprocessing; batch `stream`; knob set 3), `fused_layout` (4:4:4, 4:4:0, 4:2:0 and the grayscale kernel, Decoder
and batches), `generic` (the batch of all samplings; knob set 0), `split` (knob set 0) and `fused` (batch `fused`: 2100 images of 65
intervals, beyond the cooperative kernel's launches and the paired kernel's; knob set 1).

Not reached, by the dispatch: `walk_mcu`.  The walk reads the direct AC and DC tables from LDS wherever L2 ends
(coop_body.h: coop_tables) and plan_walk stages 12288 entries and the direct DC tables at the most, so runtime.cpp
(walk_luts_fit) keeps images of regimes B and C, and batches that hold one, off the route.  It did not when these cases
were written: `ac_sizes_dc/wide_b/422/reference` and the other regime-B and -C frames of batch `walk`, and the Decoder on
`random_dense_strip/wide_c/422/reference`, decoded to wrong pixels through `walk_mcu`.  Batch `walk` -- intervals of 4
and 16 MCUs, light: the route's own shape -- now asserts the kernel the card takes instead, and `walk_a`, the same
recipe without the regime-B and -C frames, that regime A still walks."""
import collections
import json
import os
import subprocess
import sys

import pytest

import coef_stream as cs
import gpu_wide_tables_worker as worker
import gray_stream as gs

pytestmark = pytest.mark.gpu

FRAMES = {f.name: f for f in cs.wide_cases() + gs.wide_cases()}


def layout_of(name):
    f = FRAMES[name]
    return "gray" if isinstance(f, gs.GrayFrame) else f.layout


def regime(name):
    return cs.table_regime(FRAMES[name])["regime"]


# ---- what the card answered -------------------------------------------------------------------------------------------

# Decoder, 4:2:2: the cooperative kernel (a DRI, or one interval of at most 64 MCUs); the dense strip, one interval of 520
# MCUs, the streamed kernel
DECODER_422 = {"random_dense_strip/wide_c/422/reference": "fused_stream"}
# Extension layouts and grayscale: whole windows; with device preprocessing the window is planned from an estimated span
# (twice the average), which cuts it for these frames: streamed (as test_gpu_coef.DEVICE_STREAMED)
DEVICE_STREAMED = {f"{fam}/{kind}/{lay}/reference" for lay in ("444", "440", "420")
                   for fam, kind in [("ac_sizes_dc", k) for k in ("wide_a", "wide_b", "wide_b48", "wide_c", "full")]}


def decoder_kernel(name, prep):
    if layout_of(name) == "422":
        return DECODER_422.get(name, "coop_team")
    return "fused_stream" if prep == "device" and name in DEVICE_STREAMED else "fused_layout"


# batch recipe (worker.batch_recipes) -> kernel, the same under preprocessing 0, 1 and 2, unchunked and chunked
BATCH = {"many": "coop_team", "fused": "fused", "pair": "pair", "coop": "coop_team", "stream": "fused_stream", "walk": "pair", "walk_a": "walk_mcu",
         "gray": "fused_layout", "mixed": "generic", "layout_444": "fused_layout", "layout_440": "fused_layout", "layout_420": "fused_layout"}
# the mixed A / B / C batches and the uniform ones, by sampling
MIXED = {"422": "pair", "444": "fused_layout", "440": "fused_layout", "420": "fused_layout", "gray": "fused_layout"}
UNIFORM = {"422": "coop_team", "444": "fused_layout", "440": "fused_layout", "420": "fused_layout", "gray": "fused_layout"}
# knob set k of test_gpu_route_matrix.LAB -> (Decoder: by frame name, else by sampling; batch of the sampling's frames)
_EXT = ("444", "440", "420", "gray")
LAB = [
    (dict({"422": "split"}, **{lay: "generic" for lay in _EXT}),) * 2,
    # (COMPEG_WALK = 0 closes the batch's walk route; a Decoder still takes it for light intervals of 8 MCUs or more --
    # with tables that fit: regime A)
    (dict({"422": "fused", "ac_sizes_dc/wide_a/422/reference": "walk_mcu"}, **{lay: "fused_layout" for lay in _EXT}),
     dict({"422": "fused"}, **{lay: "fused_layout" for lay in _EXT})),
    (dict({"422": "pair"}, **{lay: "fused_layout" for lay in _EXT}),) * 2,
    # (the streamed form exists for 4:2:0 and for the paired 4:4:4 / 4:4:0 kernels: intervals of two MCUs or more)
    ({"422": "fused_stream", "420": "fused_stream", "444": None, "440": None, "gray": "fused_layout"},
     {"422": "fused_stream", "420": "fused_stream", "444": "fused_layout", "440": "fused_layout", "gray": "fused_layout"}),
]


def lab_decoder_kernel(k, name):
    table = LAB[k][0]
    want = table.get(name, table[layout_of(name)])
    if want is None:   # knob set 3, 8-pixel MCUs: streamed where the frame's intervals hold two MCUs or more
        want = "fused_stream" if FRAMES[name].interval >= 2 else "fused_layout"
    return want


def expected(key):
    p = key.split("|")
    if p[0] == "decoder":
        return decoder_kernel(p[1], p[2])
    if p[0] == "batch":
        return BATCH[p[1]]
    if p[0] == "mixed":
        return MIXED[p[1]]
    if p[0] == "uniform":
        return UNIFORM[p[1]]
    k = int(p[0][3:])
    return lab_decoder_kernel(k, p[2]) if p[1] == "decoder" else LAB[k][1][p[2]]


def check_kernels(kernels):
    return [f"{key}: last_kernel() = {got}, expected {expected(key)}" for key, got in kernels.items() if got != expected(key)]


def regime_c_in(key):
    """Does the decode behind this key hold a regime-C frame?  (worker.bind is not needed: the recipes are plain lists.)"""
    p = key.split("|")
    if p[0] == "decoder":
        return regime(p[1]) == "C"
    if p[0] in ("mixed", "uniform"):
        return True
    if p[0] == "batch":
        return p[1] != "walk_a"
    return regime(p[2]) == "C" if p[1] == "decoder" else True


# ---- the tests --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_wide_tables") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_wide_tables(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_every_decode_took_the_kernel_of_the_tables(results):
    done, log = results
    assert done.get("kernels"), log
    fails = check_kernels(done["kernels"])
    assert not fails, "\n".join(fails)


def test_every_route_decodes_regime_c_frames(results):
    """The route counter: decodes that held a regime-C frame, by kernel.  Every route the tables above name must have one --
    but `walk_mcu`, which the dispatch keeps such tables off (the module's docstring)."""
    done, log = results
    assert done.get("kernels"), log
    count = collections.Counter(kernel for key, kernel in done["kernels"].items() if regime_c_in(key))
    print("decodes that held a regime-C frame, by kernel:", dict(count))
    named = {expected(key) for key in done["kernels"]}
    assert named >= {"fused", "pair", "coop_team", "fused_stream", "walk_mcu", "fused_layout", "generic", "split"}
    for kernel in sorted(named - {"walk_mcu"}):
        assert count[kernel] > 0, f"no regime-C frame went through {kernel}: {dict(count)}"
    assert count["walk_mcu"] == 0, "a regime-C frame on the walk route: its direct tables are not staged there"
    gray = [key for key, kernel in done["kernels"].items() if kernel == "fused_layout" and regime_c_in(key) and ("|gray" in key or "/gray/" in key)]
    assert gray, "no regime-C frame went through the grayscale kernel"


def test_the_worker_is_quick(results):
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the wide-tables worker takes too long for a suite that runs with every change"
