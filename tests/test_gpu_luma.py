"""Luma tensor output on the card (include/compeg_hip.h, "Luma tensor output"): Decoder.pack_tensor_luma /
Batch.pack_tensor_luma into torch tensors, every element against the oracle's RGBA put through the header's contract
(tests/luma_reference.py), bit for bit, or against plane 0 of what pack_tensor_oriented itself stored for the same
arguments.  The cases live in tests/gpu_luma_worker.py and run, all of them, in one process of their own that imports
torch before the library (like tests/test_gpu_nhwc.py) and stops at the first error of the device; each case is reported
here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_luma_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_luma") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_luma_tensor_output(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]
