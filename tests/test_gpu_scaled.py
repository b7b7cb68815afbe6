"""The scaled decode on the card (include/compeg_hip.h, "Scaled decode"): Decoder.decode_scaled and Batch.decode_scaled
through decode_scaled_422 / _444 / _440 / _420 / _gray_kernel at N = 4 and N = 2, every byte of the destination -- between
sentinels, over a pre-fill -- against tests/scaled_stream.py, at denominators 2 and 4: 324 x 70 in every sampling (the edges
cut MCUs) at restart intervals that divide the MCU counts and without DRI, 960 intervals, MCUs behind the last complete
interval, 8 x 8 and 1 x 1 frames, an interval longer than the window cap, the coefficient families in both entropy modes, the
golden files, DC-only frames against the card's own decode_reduced, denominator 8 byte for byte decode_reduced with
last_kernel "reduced", batches (chunks, preprocessing modes, RGBA decodes and packs around the scaled decodes, last_kernel
"scaled"), the refusals that need an object, and the ordering across streams with the producer's stream stalled
(tests/stream_stall.py), both ways round, for Decoder and Batch.  The cases live in tests/gpu_scaled_worker.py and run, all
of them, in one process of their own that imports torch before the library and stops at the first error of the device; each
case is reported here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_scaled_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_scaled") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_scaled_decode(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_the_worker_is_quick(results):
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the scaled worker takes too long for a suite that runs with every change"
