"""The GPU cases of tests/test_gpu_wide_tables.py: RGBA decodes of frames whose Huffman tables outgrow their share of LDS
(cs.wide_cases, gs.wide_cases; cs.table_regime) through Decoder and Batch, every byte of every output against the oracle
(grayscale: gs.expectation).  Run in one process of their own that imports torch before the library
(tests/gpu_luma_worker.py: why) and stops at the first error of the device.

    python tests/gpu_wide_tables_worker.py RESULTS.json [substring of the case names to run]

RESULTS.json: case name -> null, or what went wrong; "kernels": {decode -> last_kernel()}, which the test module holds
against its tables; "wall_s".  The laboratory cases each start one fresh child process (the lab library reads its knobs
when it is loaded)."""
import json
import os
import subprocess
import sys
import time
import traceback

import numpy as np

torch = ca = cs = gs = orc = gpu = None   # set by main(): torch first
KERNELS = {}
_WANT = {}
LAYOUTS = ("422", "444", "440", "420", "gray")


def layout_of(f):
    return "gray" if isinstance(f, gs.GrayFrame) else f.layout


def regime(f):
    return cs.table_regime(f)["regime"]


def want(f):
    if f.name not in _WANT:
        _WANT[f.name] = gs.expectation(f) if isinstance(f, gs.GrayFrame) else orc.ImageData(f.jpeg(), **f.image_kw()).decode()
    return _WANT[f.name]


def image(f):
    return ca.ImageData(f.jpeg(), allow_sampling=True, allow_grayscale=True, standard_entropy=f.standard)


class DeviceTrouble(Exception):
    """A child process that used the card did not end well: nothing more is started on it."""


def wide(layout=None):
    return [f for f in cs.wide_cases() + gs.wide_cases() if layout is None or layout_of(f) == layout]


def named(*names):
    every = {f.name: f for f in cs.wide_cases() + gs.wide_cases() + cs.cases()}
    return [every[n] for n in names]


# ---- Decoder -----------------------------------------------------------------------------------------------------------

def decoder(layout):
    """Every wide frame of the layout: host and device preprocessing, decode_blocking and start_decode on one Decoder each."""
    fails = []
    for f in wide(layout):
        for device in (False, True):
            dec = ca.Decoder(gpu)
            dec.set_device_preprocess(device)
            img = image(f)
            for how in ("blocking", "start_decode"):
                if how == "blocking":
                    dec.decode_blocking(img)
                else:
                    dec.start_decode(img).wait()
                key = f"decoder|{f.name}|{'device' if device else 'host'}|{how}"
                KERNELS[key] = dec.last_kernel()
                got = dec.read_texture(f.w, f.h)
                if got.shape != want(f).shape or not np.array_equal(got, want(f)):
                    fails.append(f"{key} ({KERNELS[key]}, regime {regime(f)}): {int((got != want(f)).any(axis=2).sum())} pixels differ")
    assert not fails, "\n".join(fails)


# ---- Batch -------------------------------------------------------------------------------------------------------------

def _cycle(frames, n):
    return [frames[i % len(frames)] for i in range(n)]


_WALK_A = ("dc_cats/short/422/reference/dri4", "positions/short/422/reference/dri4", "run_size0/edge/422/reference/dri3",
           "pairs/short/422/reference/dri6", "texture/edge/422/reference/dri4")


def batch_recipes():
    """name -> (frames, chunk of the chunked run).  Each is built after test_gpu_coef.batch_recipes / test_gpu_route_matrix.BATCHES
    for one route, and holds regime-C frames (most of them nothing else)."""
    w422 = wide("422")
    c422 = [f for f in w422 if regime(f) == "C"]
    dri1 = [f for f in c422 if f.ri == 1]
    out = {
        # DRI 1, two waves an image, 700 images: more than the paired kernel's 1024 waves, still the cooperative kernel's
        "many": (_cycle([f for f in dri1 if f.intervals == 65], 700), 650),
        # ... 2100 images: 4 x 65 x 2100 data units are beyond the cooperative kernel's launches too (use_coop_kernel: 2 x
        # 1024 x 256), which leaves `fused`; the chunked run's first launch, 2060 images, is still beyond both
        "fused": (_cycle([f for f in dri1 if f.intervals == 65], 2100), 2060),
        # DRIs of 1 and 4 mixed: no common interval for the cooperative kernel, a one-MCU interval closes the walk
        "pair": (_cycle([f for f in c422 if f.ri], 24), 7),
        "coop": (_cycle(dri1, 12), 5),
        # the dense strip's one interval cuts whole windows
        "stream": ([f for f in c422 if f.mcus > 1], 4),
        # intervals of 4 and 16 MCUs, light -- the shape of the walk + lane-per-MCU route (regime-A frames of cs.cases()
        # beside them, as in test_gpu_coef.WALK_BATCH): with a regime-B or -C image the dispatch keeps the batch off it
        # (runtime.cpp: walk_luts_fit); without them (`walk_a`) it walks
        "walk": ([f for f in w422 if f.interval >= 4 and f.mcus <= 64] + named(*_WALK_A), 5),
        "walk_a": ([f for f in w422 if f.interval >= 4 and f.mcus <= 64 and regime(f) == "A"] + named(*_WALK_A), 2),
        "gray": (wide("gray"), 6),
        "mixed": ([f for lay in LAYOUTS for f in wide(lay) if regime(f) == "C" and f.mcus <= 65], 11),
    }
    for lay in ("444", "440", "420"):
        out["layout_" + lay] = (wide(lay), 5)
    return out


def _decode_batch(batch, frames, chunk, what):
    batch.upload([image(f) for f in frames])
    batch.set_chunk(chunk)
    batch.decode()
    batch.wait()
    KERNELS[what] = batch.last_kernel()
    bad = [i for i, f in enumerate(frames) if not np.array_equal(batch.read_output(i), want(f))]
    return [f"{what} ({KERNELS[what]}): slot {i}, {frames[i].name} (regime {regime(frames[i])}): pixels differ" for i in bad[:8]]


def batches(mode):
    """Every recipe unchunked and chunked under one preprocessing mode, one Batch object re-uploaded across the route changes."""
    fails = []
    batch = ca.Batch(gpu)
    batch.set_device_preprocess(mode)
    for name, (frames, chunk) in batch_recipes().items():
        assert any(regime(f) == "C" for f in frames) or name == "walk_a", name
        fails += _decode_batch(batch, frames, 0, f"batch|{name}|{mode}|whole")
        fails += _decode_batch(batch, frames, chunk, f"batch|{name}|{mode}|chunked")
    assert not fails, "\n".join(fails)


def mixed_regimes():
    """Regime A, B and C images of one sampling in one batch -- planned with the largest image's tables while each image
    stages its own --, the regime-C image first, in the middle and last; chunks of three, so that a launch holds regime-A
    images alone while the batch's maximum is C; and a uniform batch of one regime-C image sixteen times (the look-alike
    path stages the tables once)."""
    fails = []
    for lay in LAYOUTS:
        mine = wide(lay)
        a = [f for f in mine if regime(f) == "A"] + [f for f in (gs.cases() if lay == "gray" else cs.cases()) if layout_of(f) == lay and f.mcus <= 64][:5]
        b = [f for f in mine if regime(f) == "B"][:3]
        c = [f for f in mine if regime(f) == "C" and f.mcus <= 65]
        assert len(a) >= 3 and b and len(c) >= 3, lay
        for mode in (0, 2):
            batch = ca.Batch(gpu)
            batch.set_device_preprocess(mode)
            for where in ("first", "middle", "last"):
                rest = a[:3] + b + a[3:6]
                at = {"first": 0, "middle": 3 + len(b) // 2, "last": len(rest)}[where]
                frames = rest[:at] + [c[0]] + rest[at:]
                assert {regime(f) for f in frames} == set("ABC")
                fails += _decode_batch(batch, frames, 0, f"mixed|{lay}|{mode}|{where}|whole")
                if where != "first":
                    assert {regime(f) for f in frames[:3]} == {"A"}, "the first launch holds regime-A images alone"
                fails += _decode_batch(batch, frames, 3, f"mixed|{lay}|{mode}|{where}|chunked")
            for k, f in enumerate(c[:3]):
                fails += _decode_batch(batch, [f] * 16, 0 if k % 2 == 0 else 5, f"uniform|{lay}|{mode}|{f.name}")
    assert not fails, "\n".join(fails)


# ---- the laboratory library ------------------------------------------------------------------------------------------------

_LAB_CODE = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import gpu_wide_tables_worker as w
w.bind(with_torch=False)   # (nothing of torch's is used here: the library alone, as in test_gpu_coef's laboratory runs)
kernels = {}
fails = []
for layout in w.LAYOUTS:
    frames = w.wide(layout)
    for f in frames:
        dec = w.ca.Decoder(w.gpu)
        dec.decode_blocking(w.image(f))
        kernels[f"lab|decoder|{f.name}"] = dec.last_kernel()
        if not w.np.array_equal(dec.read_texture(f.w, f.h), w.want(f)):
            fails.append(f"decoder {f.name} ({dec.last_kernel()}): pixels differ")
    batch = w.ca.Batch(w.gpu)
    batch.upload([w.image(f) for f in frames])
    batch.decode()
    batch.wait()
    kernels[f"lab|batch|{layout}"] = batch.last_kernel()
    fails += [f"batch {layout} ({batch.last_kernel()}): {f.name}: pixels differ" for i, f in enumerate(frames) if not w.np.array_equal(batch.read_output(i), w.want(f))]
print(json.dumps({"kernels": kernels, "fails": fails}), flush=True)
print("lab done")
'''


def lab(k):
    """Knob set k of test_gpu_route_matrix.LAB (`split` among them) in a fresh child process: every wide frame through a
    Decoder, one batch per layout."""
    import test_gpu_route_matrix as grm
    knobs = grm.LAB[k][0]
    lib = os.path.join(os.path.dirname(ca.LIB_PATH), "libcompeg_hip_lab.so")
    assert os.path.exists(lib), "make -C compeg_amd/csrc lab (__graft_entry__.build() does)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, "-c", _LAB_CODE, root], env=dict(os.environ, COMPEG_LIB=lib, **knobs), capture_output=True, text=True, timeout=100)
    except subprocess.TimeoutExpired as e:
        raise DeviceTrouble(f"lab {knobs}: no end after {e.timeout} s") from None   # (well inside the limit the test module gives this whole worker)
    if r.returncode != 0 or "lab done" not in r.stdout:
        raise DeviceTrouble(f"lab {knobs}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    out = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("{")))
    KERNELS.update({key.replace("lab|", f"lab{k}|"): v for key, v in out["kernels"].items()})
    assert not out["fails"], f"lab {knobs}:\n" + "\n".join(out["fails"])


CASES = {f"decoder[{lay}]": (decoder, (lay,)) for lay in LAYOUTS}
CASES.update({f"batches[{mode}]": (batches, (mode,)) for mode in (0, 1, 2)})
CASES["mixed_regimes"] = (mixed_regimes, ())
CASES.update({f"lab[{k}]": (lab, (k,)) for k in range(4)})


def bind(with_torch=True):
    """The modules and the device, torch first."""
    global torch, ca, cs, gs, orc, gpu
    if with_torch:
        import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import coef_stream as cs
    import gray_stream as gs
    from oracle import oracle as orc
    gpu = ca.Gpu.open(0)


def main(out_path, only=""):
    t0 = time.time()
    bind()
    results, device_said_no = {}, False
    for name, (fn, args) in CASES.items():
        if only not in name:
            continue
        t1 = time.time()
        try:
            fn(*args)
            results[name] = None
        except ca.Error as e:
            results[name] = f"compeg_amd.Error {e.code}: {e}\n{traceback.format_exc()}"
            device_said_no = e.code == ca.E_HIP
        except AssertionError:
            results[name] = traceback.format_exc()
        except Exception:   # (torch's own errors come from the device as well)
            results[name] = traceback.format_exc()
            device_said_no = True
        print(f"{name}: {'ok' if results[name] is None else 'FAILED'} in {time.time() - t1:.2f} s", flush=True)
        results["wall_s"] = round(time.time() - t0, 2)
        results["kernels"] = KERNELS
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
        if device_said_no:   # nothing more is started on it
            break
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
