"""The coefficient-level frames of tests/coef_stream.py on the card: the device-only forms of the decode arithmetic (the
hand-written walk block of chase_run_lean, pack_rows3 / pack_rows2's v_cvt_pk_u8_f32 under a switched rounding mode,
aan_cross's packed adds) meet the values no encoder of 8-bit pictures emits.  Every decode is compared with the oracle
over the whole output and asserts `last_kernel()`: the tables below are what the MI355X answered when the cases were
written, and hold from then on.

  * Decoder: the shipped dispatch, host and device preprocessing, blocking and start_decode (DECODER).
  * Batch: all 4:2:2 cases in one batch (streamed at any count: the strips' one interval cuts whole windows), those
    with a DRI (`fused`), the small ones with an interval of one MCU for the cooperative kernel, two batches of mixed
    longer intervals -- built like test_gpu_route_matrix.BATCHES["walk_long"] -- for the walk + lane-per-MCU route, one
    batch per extension layout; preprocessing modes 0, 1 and 2 (BATCH).
  * The laboratory library under the four knob sets of test_gpu_route_matrix.LAB, each in a fresh child process, every
    case through a Decoder and one batch per layout: `split`, `fused`, `pair`, `fused_stream`, the layout kernels (LAB).
  * `dc_hostile` (a DC category above 15): only that a kernel ran and the pixels are the oracle's; its name is printed."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coef_stream as cs
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

_WANT = {}


def want(f):
    if f.name not in _WANT:
        _WANT[f.name] = orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    return _WANT[f.name]


def by_layout(layout):
    return [f for f in cs.cases() if f.layout == layout]


# ---- what the card answered -------------------------------------------------------------------------------------------

# Decoder, 4:2:2: the cooperative kernel for every frame with a DRI and for the small ones without (one interval of at most
# 64 MCUs); the `dc_wrap` strip (one interval of 320 light MCUs) takes the walk + lane-per-MCU route, the dense strip
# (520 MCUs of 32 words each: beyond the walk's rows, use_mcu_route) the streamed kernel.
DECODER_422 = {"dc_wrap/short/422/reference": "walk_mcu", "random_dense_strip/long/422/reference": "fused_stream"}
# Extension layouts: whole windows when the host preprocessed the scan; on the device path the window is planned from an
# estimated span (twice the average), which cuts it for these frames: streamed
DEVICE_STREAMED = {f"{fam}/{lay}/reference" + dri
                   for lay in ("444", "440", "420")
                   for fam, dri in (("ac_sizes/long", ""), ("run_size0/edge", ""), ("dc_wrap/short", ""),
                                    ("random_dense/long", "/dri3"), ("texture/edge", "/dri4"))} | {
                       "saturated/short/420/reference/dri1", "saturated/short/444/reference/dri2", "saturated/short/440/reference/dri2"}


def decoder_kernel(f, device):
    if f.layout == "422":
        return DECODER_422.get(f.name, "coop_team")
    return "fused_stream" if device and f.name in DEVICE_STREAMED else "fused_layout"


# batch recipe (batch_recipes) -> kernel, the same under preprocessing 0, 1 and 2
BATCH = {"all_422": "fused_stream", "fused": "fused", "coop": "coop_team", "walk": "walk_mcu", "walk_arithmetic": "walk_mcu",
         "layout_444": "fused_layout", "layout_440": "fused_layout", "layout_420": "fused_layout"}

# knob set k of test_gpu_route_matrix.LAB -> (Decoder, batch of the layout's cases): a kernel by case name, else by
# (layout, the restart interval holds two MCUs or more), else by layout
_LAB_WALK = ("ac_sizes/short/422/reference", "ac_sizes/edge/422/reference", "ac_sizes/long/422/reference",
             "dc_wrap/short/422/reference", "basis_q255/short/422/reference/dri8", "dc_sweep/short/422/reference/dri8",
             "gamut/short/422/reference/dri8", "cancel/short/422/reference/dri9")
LAB = [
    ({"422": "split", "444": "generic", "440": "generic", "420": "generic"},) * 2,
    # (COMPEG_WALK = 0 closes the batch's walk route; a Decoder still takes it for light intervals of 8 MCUs or more)
    (dict({"422": "fused", "444": "fused_layout", "440": "fused_layout", "420": "fused_layout"}, **{n: "walk_mcu" for n in _LAB_WALK}),
     {"422": "fused", "444": "fused_layout", "440": "fused_layout", "420": "fused_layout"}),
    ({"422": "pair", "444": "fused_layout", "440": "fused_layout", "420": "fused_layout"},) * 2,
    # (the streamed form exists for 4:2:0 and for the paired 4:4:4 / 4:4:0 kernels: intervals of two MCUs or more)
    ({"422": "fused_stream", "420": "fused_stream", ("444", True): "fused_stream", ("444", False): "fused_layout",
      ("440", True): "fused_stream", ("440", False): "fused_layout"},
     {"422": "fused_stream", "420": "fused_stream", "444": "fused_layout", "440": "fused_layout"}),
]


# ---- the plans ---------------------------------------------------------------------------------------------------------

# (mixed intervals of 3 MCUs and more: no common DRI for the cooperative kernel, light MCUs, few enough of them for
# use_mcu_route's 14.5 x DRI - 40 > MCUs / 5300)
WALK_BATCH = ("ac_sizes/short/422/reference", "ac_sizes/edge/422/reference", "ac_sizes/long/422/reference",
              "dc_cats/short/422/reference/dri4", "q1_underflow/long/422/reference/dri4",
              "positions/short/422/reference/dri4", "positions/long/422/reference/dri4",
              "run_size0/short/422/reference/dri3", "run_size0/edge/422/reference/dri3", "run_size0/long/422/reference/dri3",
              "pairs/short/422/reference/dri6", "pairs/long/422/reference/dri6", "texture/edge/422/reference/dri4",
              "random_dense/long/422/reference/dri3", "random_dense/long/422/reference/dri7")


# (the arithmetic families at intervals of 8 and 9 MCUs: gamut's 576 intervals an image ask for 14.5 x 8 - 40)
WALK_ARITHMETIC = ("basis_q255/short/422/reference/dri8", "dc_sweep/short/422/reference/dri8", "gamut/short/422/reference/dri8",
                   "saturated/short/422/reference/dri8", "cancel/short/422/reference/dri9")


def batch_recipes():
    c422 = by_layout("422")
    out = {
        "all_422": c422,                              # (the strips' one interval cuts whole windows: streamed)
        "fused": [f for f in c422 if f.ri],           # (gamut alone is 72 waves: beyond the paired kernel's 1024)
        "coop": [f for f in c422 if f.ri == 1 and f.mcus <= 64][:12],
        "walk": [cs.case(n) for n in WALK_BATCH],
        "walk_arithmetic": [cs.case(n) for n in WALK_ARITHMETIC],
    }
    for lay in ("444", "440", "420"):
        out["layout_" + lay] = by_layout(lay)
    return out


def decode_with_decoder(ca, gpu, f, device):
    """-> [(how, kernel, pixels equal)] of a fresh Decoder: blocking, then start_decode."""
    dec = ca.Decoder(gpu)
    dec.set_device_preprocess(device)
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    out = []
    for how in ("blocking", "start_decode"):
        if how == "blocking":
            dec.decode_blocking(img)
        else:
            dec.start_decode(img).wait()
        out.append((how, dec.last_kernel(), bool(np.array_equal(dec.read_texture(f.w, f.h), want(f)))))
    return out


def decode_with_batch(ca, batch, frames):
    """-> (kernel, [slots whose pixels differ])."""
    batch.upload([ca.ImageData(f.jpeg(), allow_sampling=True, standard_entropy=f.standard) for f in frames])
    batch.decode()
    batch.wait()
    return batch.last_kernel(), [i for i, f in enumerate(frames) if not np.array_equal(batch.read_output(i), want(f))]


# ---- the tests --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ca():
    import compeg_amd
    return compeg_amd


@pytest.fixture(scope="module")
def gpu(ca):
    return ca.Gpu.open(0)


@pytest.mark.parametrize("layout", sorted(cs.LAYOUTS))
def test_decoder_on_coefficient_frames(ca, gpu, layout):
    fails = []
    for f in by_layout(layout):
        for device in (False, True):
            for how, kernel, ok in decode_with_decoder(ca, gpu, f, device):
                what = f"{f.name} ({'device' if device else 'host'} preprocessing, {how})"
                if f.family == "dc_hostile":
                    print(f"{what}: {kernel}")
                    if kernel in ("", "none"):
                        fails.append(f"{what}: no kernel ran")
                elif kernel != decoder_kernel(f, device):
                    fails.append(f"{what}: last_kernel() = {kernel}, expected {decoder_kernel(f, device)}")
                if not ok:
                    fails.append(f"{what}: {kernel}: pixels differ from the oracle")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batches_of_coefficient_frames(ca, gpu, mode):
    fails = []
    batch = ca.Batch(gpu)
    batch.set_device_preprocess(mode)
    for name, frames in batch_recipes().items():
        kernel, bad = decode_with_batch(ca, batch, frames)
        if kernel != BATCH[name]:
            fails.append(f"batch {name} mode {mode}: last_kernel() = {kernel}, expected {BATCH[name]}")
        fails += [f"batch {name} mode {mode} ({kernel}): slot {i}, {frames[i].name}: pixels differ" for i in bad]
    assert len(batch_recipes()["coop"]) <= 12
    assert not fails, "\n".join(fails)


_LAB_CODE = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import compeg_amd as ca
import coef_stream as cs
import test_gpu_coef as t
gpu = ca.Gpu.open(0)
for layout in sorted(cs.LAYOUTS):
    for f in t.by_layout(layout):
        how, kernel, ok = t.decode_with_decoder(ca, gpu, f, False)[0]
        print(json.dumps(["decoder", layout, f.name, kernel, ok]), flush=True)
    frames = t.by_layout(layout)
    kernel, bad = t.decode_with_batch(ca, ca.Batch(gpu), frames)
    print(json.dumps(["batch", layout, [frames[i].name for i in bad], kernel, not bad]), flush=True)
print("lab done")
'''


def run_lab(ca, knobs):
    """One knob set in a fresh child process -> [[caller, layout, case name(s), kernel, pixels equal]]."""
    lab = os.path.join(os.path.dirname(ca.LIB_PATH), "libcompeg_hip_lab.so")
    assert os.path.exists(lab), "make -C compeg_amd/csrc lab (__graft_entry__.build() does)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LAB_CODE, root], env=dict(os.environ, COMPEG_LIB=lab, **knobs),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lab done" in r.stdout, (knobs, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("[")]


def lab_kernel(table, f_or_layout):
    """A LAB table's kernel: by case name, else by (layout, whether the frame's intervals are pairs of MCUs), else by
    layout."""
    if isinstance(f_or_layout, str):
        return table[f_or_layout]
    f = f_or_layout
    return table.get(f.name, table.get((f.layout, f.interval >= 2), table.get(f.layout)))


@pytest.mark.parametrize("k", range(4))
def test_lab_routes_on_coefficient_frames(ca, gpu, k):
    import test_gpu_route_matrix as grm
    knobs = grm.LAB[k][0]
    dec_want, batch_want = LAB[k]
    fails = []
    for caller, layout, names, kernel, ok in run_lab(ca, knobs):
        if caller == "decoder":
            f = cs.case(names)
            if f.family == "dc_hostile":
                print(f"lab {knobs}: {names}: {kernel}")
                if kernel in ("", "none"):
                    fails.append(f"lab {knobs}: {names}: no kernel ran")
            elif kernel != lab_kernel(dec_want, f):
                fails.append(f"lab {knobs} decoder: {names}: {kernel}, expected {lab_kernel(dec_want, f)}")
        else:
            if kernel != lab_kernel(batch_want, layout):
                fails.append(f"lab {knobs} batch {layout}: {kernel}, expected {lab_kernel(batch_want, layout)}")
        if not ok:
            fails.append(f"lab {knobs} {caller} {layout} ({kernel}): pixels differ: {names}")
    assert not fails, "\n".join(fails)


def test_the_tables_reach_every_route_with_every_family():
    """By the tables above -- which the tests of this module assert decode by decode -- the walk route, the cooperative
    kernel, `fused`, `pair`, `fused_stream`, `split` and the layout kernels of the three extension layouts each decode a
    case of every family.  Not admitted, by the dispatch: `dc_hostile` by the walk tables (a DC category above 15) --
    whichever kernel takes it is printed, not asserted; `dc_wrap` by the cooperative kernel (its point is one interval of
    320 MCUs, above kCoopMaxRestart)."""
    import test_gpu_route_matrix as grm
    reach = collections.defaultdict(set)
    for f in cs.cases():
        for device in (False, True):
            reach[(decoder_kernel(f, device), f.layout)].add(f.family)
        for dec_want, _ in LAB:
            reach[(lab_kernel(dec_want, f), f.layout)].add(f.family)
    for name, frames in batch_recipes().items():
        reach[(BATCH[name], frames[0].layout)] |= {f.family for f in frames}
    for _, batch_want in LAB:
        for lay in cs.LAYOUTS:
            reach[(lab_kernel(batch_want, lay), lay)] |= {f.family for f in by_layout(lay)}
    assert len(LAB) == len(grm.LAB)
    every = set(cs.ENTROPY_FAMILIES + cs.ARITHMETIC_FAMILIES) - {"dc_hostile"}
    need = {("walk_mcu", "422"): every, ("coop_team", "422"): every - {"dc_wrap"}}
    need.update({(k, "422"): every for k in ("fused", "pair", "fused_stream", "split")})
    need.update({(k, lay): every for k in ("fused_layout", "fused_stream", "generic") for lay in ("444", "440", "420")})
    missing = {key: sorted(fams - reach[key]) for key, fams in need.items() if fams - reach[key]}
    assert not missing, missing
