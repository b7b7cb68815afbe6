"""The scan kernels themselves (count, tile_scan, emit, span, pull, pull3) on the card, on the edge matrix of
tests/scan_edges.py: misaligned segments between FF or 00 neighbours, outputs of exactly the documented size between
guards, all of it prefilled with A5 (or with the previous launch's output), many images to a launch.  One process of
tests/gpu_scan/scan_harness (built by build(), linked with the library's own scan_kernels.o) runs every group; each
group is reported here, compared byte for byte with the references."""
import os
import shutil
import subprocess

import pytest

import scan_edges as se

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_scan", "scan_harness")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = tmp_path_factory.mktemp("gpu_scan_edges")
    cases = out / "cases.bin"
    se.write_cases(cases, se.GROUP_NAMES)
    assert os.path.exists(HARNESS), "tests/gpu_scan/scan_harness is not built (build() makes it)"
    r = subprocess.run(["timeout", "-k", "10", "240", HARNESS, str(cases), str(out)], capture_output=True, text=True)
    yield out, f"harness exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    shutil.rmtree(out, ignore_errors=True)   # (every launch's whole arena: some hundred megabytes)


def _launch(results, name):
    out, log = results
    path = out / f"g{se.GROUP_NAMES.index(name):04d}.bin"
    assert path.exists(), f"{name} did not run: {log}"
    return se.read_result(path)


@pytest.mark.parametrize("name", se.GROUP_NAMES)
def test_scan_kernels(results, name):
    g = se.group(name)
    rows, arena = _launch(results, name)
    if isinstance(g, se.PullGroup):
        se.check_pull(g, rows, arena)
    else:
        before = _launch(results, se.GROUP_NAMES[se.GROUP_NAMES.index(name) - 1])[1] if g.keep else None
        se.check_scan(g, rows, arena, before)


def test_harness_ran_every_group(results):
    _, log = results
    assert log.startswith("harness exit 0\n"), log
