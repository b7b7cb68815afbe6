"""The cropped decode of a region list on the card (include/compeg_hip.h, "Cropped decode of a region list"):
Batch.decode_cropped_regions and Decoder.decode_cropped_regions through decode_cropped_regions_422 / _444 / _440 / _420 /
_gray_kernel, every byte of the destination -- between sentinels, over a pre-fill -- against tests/crop_regions_stream.py:
the mixed batch (five samplings, 8 x 8, 1 x 1, 1920 intervals, an MCU behind the last complete interval) with the full
region list in both formats, tight / pitched, aligned / odd, in the three preprocessing modes and with chunks of 0, 1 and 3
regions; the identity with the one-rectangle decode on a uniform batch and with the card's own RGBA decode; the Decoder
form; lists of one region and of none; RGBA decodes and a pack around the region decode; last_kernel; the refusals that
need an object; and the ordering across streams with the producer's stream stalled (tests/stream_stall.py), both ways
round, for Decoder and Batch.  The cases live in tests/gpu_crop_regions_worker.py and run, all of them, in one process of
their own that imports torch before the library and stops at the first error of the device; each case is reported here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_crop_regions_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_crop_regions") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_cropped_regions_decode(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_the_worker_is_quick(results):
    """(The bound is the cropped suite's: tests/test_gpu_crop.py.)"""
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the region worker takes too long for a suite that runs with every change"
