"""bench.py --dump-outputs without a GPU: dump_outputs against a stand-in batch.  The files stay within the 64 MB the
option allows whatever the batch and frame size, hold exactly the sampled pixels of the sampled slots, and the same
arguments write the same bytes."""
import os

import numpy as np
import pytest

LIMIT_BYTES = 64 * 10**6
NAMES = ["rgba_sample.npy", "rgba_sample_pixels.npy", "rgba_sample_slots.npy"]


@pytest.fixture(scope="module")
def bench():
    # (importing bench.py sets GPU_MAX_HW_QUEUES for its own process: leave this process's environment as it was)
    before = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench as b
    if before is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    else:
        os.environ["GPU_MAX_HW_QUEUES"] = before
    return b


class StubBatch:
    """compeg_amd.Batch.read_output's shape and type -- slot i's (height, width, 4) uint8 image -- with a pattern of
    its own in every slot."""

    def __init__(self, width, height):
        self.base = np.resize(np.arange(251, dtype=np.uint8), (height, width, 4))

    def read_output(self, index):
        return self.base ^ np.uint8(index % 256)


def _dump(bench, tmp_path, name, batch, width, height):
    d = tmp_path / name
    bench.dump_outputs(StubBatch(width, height), batch, str(d))
    return d


@pytest.mark.parametrize("batch,width,height", [(1, 3840, 2160), (2, 3840, 2160), (256, 3840, 2160),
                                                (1, 7680, 4320), (6, 640, 360)])
def test_dump_outputs_within_limit_exact_and_repeatable(bench, tmp_path, batch, width, height):
    a = _dump(bench, tmp_path, "a", batch, width, height)
    b = _dump(bench, tmp_path, "b", batch, width, height)
    assert sorted(os.listdir(a)) == NAMES
    total = sum(os.path.getsize(a / n) for n in NAMES)
    assert total <= LIMIT_BYTES, total
    for n in NAMES:
        assert (a / n).read_bytes() == (b / n).read_bytes(), n

    rgba = np.load(a / "rgba_sample.npy")
    pix = np.load(a / "rgba_sample_pixels.npy")
    slots = np.load(a / "rgba_sample_slots.npy")
    assert rgba.dtype == np.float32 and pix.dtype == np.float64 and slots.dtype == np.float64
    assert len(slots) == min(batch, bench.DUMP_SLOTS) and slots[0] == 0 and slots[-1] == batch - 1
    assert len(np.unique(slots)) == len(slots) and len(np.unique(pix)) == len(pix)
    if width * height * 24 <= bench.DUMP_BYTES:          # small frames: every pixel
        assert np.array_equal(pix, np.arange(width * height))
    assert rgba.shape == (len(slots), len(pix), 4)
    stub = StubBatch(width, height)
    for k, s in enumerate(slots.astype(np.int64)):
        want = stub.read_output(int(s)).reshape(-1, 4)[pix.astype(np.int64)]
        assert np.array_equal(rgba[k], want.astype(np.float32)), int(s)
