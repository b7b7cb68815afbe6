"""Ordering across streams with the producer stream held busy (tests/stream_stall.py): every pack entry point of Decoder and
Batch behind the decode it reads and in front of the decode that overwrites what it reads, the record block and its pinned
slots, texture growth, the Gpu's own stream, and the calls that wait on the host.  The cases live in
tests/gpu_ordering_worker.py and run, all of them, in one process of their own that imports torch before the library
(like tests/test_gpu_orient.py) and stops at the first error of the device; each case is reported here.  A case passes
only if it saw its race window open: the stalled stream had not drained when the consumer was issued."""
import json
import os
import subprocess
import sys

import pytest

import gpu_ordering_worker as worker
import stream_stall


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_ordering") / "results.json"
    r = subprocess.run([sys.executable, os.path.abspath(worker.__file__), str(out)], capture_output=True, text=True, timeout=600)
    done = json.loads(out.read_text()) if out.exists() else {}
    return done, f"worker exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(worker.CASES))
def test_ordering_with_the_producer_stalled(results, name):
    done, log = results
    assert name in done, f"{name} did not run: {log}"
    assert done[name] is None, done[name]


@pytest.mark.gpu
def test_the_stall_is_bounded_and_the_worker_quick(results):
    """The stall's length is measured on the card, not fixed in advance: a few tens of milliseconds, never above the limit."""
    done, log = results
    assert done.get("stall_ms") is not None, f"no stall was calibrated: {log}"
    print(f"stall: {done['stall_ms']:.1f} ms of {done['stall_kind']}; worker: {done.get('wall_s')} s")
    assert stream_stall.TARGET_MS / 3 <= done["stall_ms"] <= stream_stall.REFUSED_MS
    assert done["wall_s"] < 30, "the ordering worker takes too long for a suite that runs with every change"


@pytest.mark.parametrize("name", list(worker.CASES))
def test_the_outcomes_a_case_tells_apart_differ(name):
    """Without a card: the reference of the outcome a case wants is not that of the stale or overtaken one."""
    worker.precondition(name)
