"""The cropped decode on the card (include/compeg_hip.h, "Cropped decode"): Decoder.decode_cropped and Batch.decode_cropped
through decode_cropped_422 / _444 / _440 / _420 / _gray_kernel, every byte of the destination -- between sentinels, over a
pre-fill -- against tests/crop_stream.py: 324 x 70 in every sampling (both edges cut an MCU) at restart intervals that divide
the MCU counts, wrap over MCU rows and span several, and without DRI, with rectangles from one pixel to the whole frame;
1920 intervals with rectangles that leave waves and whole workgroups untouched; MCUs behind the last complete interval
inside and outside the rectangle; 8 x 8 and 1 x 1 frames; an interval longer than the window cap; the coefficient families
in both entropy modes; the golden files; the identity with the card's own RGBA decode; batches (chunks, preprocessing modes,
RGBA decodes and packs around the cropped decodes, last_kernel); the refusals that need an object; and the ordering across
streams with the producer's stream stalled (tests/stream_stall.py), both ways round, for Decoder and Batch.  The cases live
in tests/gpu_crop_worker.py and run, all of them, in one process of their own that imports torch before the library and
stops at the first error of the device; each case is reported here."""
import json
import os
import subprocess
import sys

import pytest

import gpu_crop_worker as worker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_crop") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=300)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_cropped_decode(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


def test_the_worker_is_quick(results):
    """(The bound is the reduced suite's: tests/test_gpu_reduced.py.)"""
    done, log = results
    assert done.get("wall_s") is not None, log
    print(f"worker: {done['wall_s']} s")
    assert done["wall_s"] < 60, "the cropped worker takes too long for a suite that runs with every change"
