"""The levels decode on the card (include/compeg_hip.h, "Levels decode"): Decoder.decode_levels and Batch.decode_levels
through decode_levels_422 / _444 / _440 / _420 / _gray_kernel, every byte of the destination -- between sentinels, over a
pre-fill -- against tests/levels_stream.py: the coefficient families (random_dense, positions, run_size0, ac_sizes, dc_cats,
dc_hostile, dc_wrap, q1_underflow) in every sampling and both orders, both entropy modes, with chosen levels in positions
32..63 in every sampling; a frame of one MCU, frames without DRI (one lane), 65 and 1030 intervals, MCUs behind the last
complete interval, an interval longer than the window cap; the golden files and mjpeg.jpg at positions 0..31 through
wrap32(level x q) against the oracle; batches (chunks, preprocessing modes, image i at i x total_bytes, RGBA decodes and
packs around the levels decodes, last_kernel, quant_table), the refusals that need an object, and the ordering across
streams with the producer's stream stalled (tests/stream_stall.py), both ways round, for Decoder and Batch.  The cases live
in tests/gpu_levels_worker.py and run, all of them, in one process of their own that imports torch before the library and
stops at the first error of the device; each case is reported here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_levels_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_levels") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_levels_decode(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_the_worker_is_quick(results):
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the levels worker takes too long for a suite that runs with every change"
