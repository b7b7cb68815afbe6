"""Planar YCbCr output on the card (include/compeg_hip.h, "Planar YCbCr output"): Decoder.decode_planes and
Batch.decode_planes through decode_planes_422 / _444 / _440 / _420 / _gray_kernel, every byte of the destination -- between
sentinels, over a pre-fill -- against tests/planes_stream.py: geometry and restart intervals per sampling, 960 intervals,
an interval longer than the window cap, the coefficient families that break readers, every format and the 4:2:0 option
tight and pitched, a truncated last interval, the golden files against the card's own RGBA, batches (chunks, preprocessing
modes, RGBA decodes around the planes decodes), the refusals that need an object, and the ordering across streams with the
producer's stream stalled (tests/stream_stall.py).  The cases live in tests/gpu_planes_worker.py and run, all of them, in
one process of their own that imports torch before the library and stops at the first error of the device; each case is
reported here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_planes_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_planes") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_planes_decode(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_the_worker_is_quick(results):
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the planes worker takes too long for a suite that runs with every change"
