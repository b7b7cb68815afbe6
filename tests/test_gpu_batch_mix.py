"""Look-alike batches on every batch route with a flat grid, and other table selectors on every route.

A batch is `uniform` (runtime.cpp: note_batch_properties) when its images have the same number of restart intervals
and the same LUT bytes; the flat grids then let a wave or a workgroup walk units of several images, with what it
staged from one of them.  Frames that keep those but differ in anything else -- which Huffman table each component
takes (tools/synth.py: SELECTOR_SETS), quantisers, geometry, the entropy mode -- are mixed in here at the batch's first,
second, middle and last place, and every slot is checked against the oracle; with the launches chunked unevenly, and
with the scan preprocessed on the device.  Kernel identity is asserted on every decode."""
import numpy as np
import pytest

from oracle import oracle as orc
from tools import synth

pytestmark = pytest.mark.gpu

SETS = synth.SELECTOR_SETS
WALKABLE = [n for n in sorted(SETS) if n not in ("default", "three_pairs")]   # (three_pairs: more pairs than the walk holds)


@pytest.fixture(scope="module")
def ca():
    import compeg_amd
    return compeg_amd


@pytest.fixture(scope="module")
def gpu(ca):
    return ca.Gpu.open(0)


_WANT = {}


def _want(jpeg, standard=False, sampling=False):
    """The oracle's decode, once per distinct frame."""
    key = (jpeg, standard, sampling)
    if key not in _WANT:
        _WANT[key] = orc.ImageData(jpeg, allow_sampling=sampling, standard_entropy=standard).decode()
    return _WANT[key]


def _check_slot(got, want, i, what):
    if not np.array_equal(got, want):
        diff = (got != want).any(axis=2)
        ys, xs = np.nonzero(diff) if got.shape == want.shape else ([0], [0])
        raise AssertionError(f"{what}: slot {i}: {int(diff.sum()) if got.shape == want.shape else 'shape'} pixels differ, "
                             f"first at x={xs[0]} y={ys[0]}")


def _decode(ca, gpu, items, kernel, what, chunk=0, device=False, sampling=False):
    """items: (jpeg, standard_entropy) per slot.  One batch, the kernel asserted, every slot against the oracle."""
    batch = ca.Batch(gpu)
    if device:
        batch.set_device_preprocess(2)
    batch.upload([ca.ImageData(j, allow_sampling=sampling, standard_entropy=s) for j, s in items])
    if chunk:
        batch.set_chunk(chunk)
    batch.decode()
    batch.wait()
    how = f"{what} chunk={chunk} device={device}"
    assert batch.last_kernel() == kernel, (how, batch.last_kernel())
    for i, (j, s) in enumerate(items):
        _check_slot(batch.read_output(i), _want(j, s, sampling), i, how)


def _odd_places(n):
    return sorted({0, 1, n // 2, n - 1})


def _look_alikes(base, odd, n):
    """n slots cycling through the base frames, the odd frame at the first, second, middle and last place."""
    items = [base[i % len(base)] for i in range(n)]
    for i in _odd_places(n):
        items[i] = odd
    return items


def _frames(w, h, ri, count, seed, sampling=(2, 1), **kw):
    return [synth.make_jpeg(w, h, seed=seed + i, kind=0, quality=85, ri=ri, sampling=sampling, **kw) for i in range(count)]


def _odd_frames(w, h, ri, seed, sampling=(2, 1), selectors=WALKABLE, entropy=True):
    """The odd ones out of a batch of w x h frames at this DRI: (what, (jpeg, standard), base frames of their batch)."""
    base = [(j, False) for j in _frames(w, h, ri, 3, seed, sampling)]
    out = []
    for name in selectors:
        out.append((name, (synth.make_jpeg(w, h, seed=seed + 50, ri=ri, sampling=sampling, tables=SETS[name]), False), base))
    out.append(("quantisers", (synth.make_jpeg(w, h, seed=seed + 51, quality=60, ri=ri, sampling=sampling,
                                                qtables=(1, 0, 0)), False), base))
    out.append(("portrait", (synth.make_jpeg(h, w, seed=seed + 52, ri=ri, sampling=sampling), False), base))
    if entropy:
        # (ZRL-free tables: the direct AC tables are the same in both entropy modes, so the batch is still `uniform`)
        nz = [(j, False) for j in _frames(w, h, ri, 3, seed + 60, sampling, flags=synth.NO_ZRL)]
        out.append(("standard_entropy", (synth.make_jpeg(w, h, seed=seed + 53, ri=ri, sampling=sampling, flags=synth.NO_ZRL), True), nz))
    return out


def test_look_alikes_through_the_fused_kernel(ca, gpu):
    """decode_fused_422_kernel's flat grid (DRI = 1, 112.5 waves per 1280 x 720 frame: workgroups span images):
    the shapes of test_gpu_parity.py::test_uniform_batch_spans_images_with_its_workgroups."""
    for what, odd, base in _odd_frames(1280, 720, 1, 1100, selectors=[n for n in sorted(SETS) if n != "default"]):
        # (launches of 19 frames and 5: below about 18 frames the first launch would be the cooperative kernel's)
        items = _look_alikes(base, odd, 24)
        _decode(ca, gpu, items, "fused", f"fused {what}")
        _decode(ca, gpu, items, "fused", f"fused {what}", chunk=19)


def test_look_alikes_through_the_streamed_batch_kernel(ca, gpu):
    """decode_fused_422_stream_kernel's flat grid (960 x 720, DRI = 16: test_batch_kernel_with_streamed_windows)."""
    for what, odd, base in _odd_frames(960, 720, 16, 1200, selectors=[n for n in sorted(SETS) if n != "default"]):
        items = _look_alikes(base, odd, 256)
        _decode(ca, gpu, items, "fused_stream", f"stream {what}")
        _decode(ca, gpu, items, "fused_stream", f"stream {what}", chunk=180)
        _decode(ca, gpu, items, "fused_stream", f"stream {what}", device=True)


@pytest.mark.parametrize("ri,n,chunk", [(30, 120, 47), (120, 300, 110)])
def test_look_alikes_through_the_walk_route(ca, gpu, ri, n, chunk):
    """walk_mcus_422_kernel and the decode from its records (960 x 720: test_walk_route_batches).  The flat walk
    grid hoists a wave's walk tables from its first image: images on other selectors, or in the other entropy mode,
    must take the grid of a row per image (walk_state_shared).  (Enough images for workgroups of two waves or more,
    which the flat grid lets straddle two images; chunks of 25 images or more: smaller launches are the cooperative
    kernel's.)"""
    cases = _odd_frames(960, 720, ri, 1300 + ri)
    if ri == 30:
        # 120 intervals each: 1280 x 720 at DRI = 60 beside 960 x 720 at DRI = 45
        cases.append(("other DRI", (synth.make_jpeg(1280, 720, seed=1390, ri=60), False),
                      [(j, False) for j in _frames(960, 720, 45, 3, 1380)]))
    for what, odd, base in cases:
        items = _look_alikes(base, odd, n)
        _decode(ca, gpu, items, "walk_mcu", f"walk DRI={ri} {what}")
        _decode(ca, gpu, items, "walk_mcu", f"walk DRI={ri} {what}", chunk=chunk)
        _decode(ca, gpu, items, "walk_mcu", f"walk DRI={ri} {what}", device=True)


@pytest.mark.parametrize("sampling", [(1, 1), (1, 2), (2, 2)])
def test_look_alikes_through_the_layouts_streamed_kernels(ca, gpu, sampling):
    """decode_fused_444 / _440 / _420_stream_kernel's flat grid (960 x 720, DRI = 16:
    test_extension_layouts_with_streamed_windows)."""
    for what, odd, base in _odd_frames(960, 720, 16, 1400 + 10 * sampling[1] + sampling[0], sampling,
                                       selectors=[n for n in sorted(SETS) if n != "default"], entropy=False):
        items = _look_alikes(base, odd, 300)
        _decode(ca, gpu, items, "fused_stream", f"layout {sampling} {what}", sampling=True)
        _decode(ca, gpu, items, "fused_stream", f"layout {sampling} {what}", chunk=250, sampling=True)
        _decode(ca, gpu, items, "fused_stream", f"layout {sampling} {what}", device=True, sampling=True)


def test_cooperative_kernel_small_batches_of_mixed_selectors(ca, gpu):
    """Two and three images on different selectors (960 x 720, DRI = 4): the cooperative kernel, walk tables of each
    image's own."""
    frames = {name: (synth.make_jpeg(960, 720, seed=1500 + k, ri=4, tables=SETS[name]), False)
              for k, name in enumerate(sorted(SETS))}
    for names in (("default", "swapped"), ("crossed", "default"), ("one_table", "split_chroma", "default"),
                  ("swapped", "crossed", "one_table"), ("default", "three_pairs")):
        _decode(ca, gpu, [frames[n] for n in names], "coop_team", f"coop {names}")


def test_per_image_grids_of_mixed_selectors(ca, gpu):
    """Mixed sizes, every selector set at least once: the per-image grid of the fused kernel and of the streamed one,
    and a launch small enough for the paired-wave kernel."""
    shapes = [(1000, 1000), (1016, 990), (936, 1004), (1280, 720), (250, 70), (1921, 1081)]
    names = sorted(SETS)
    # (one-MCU intervals: whole windows; 24 frames: beyond the cooperative kernel's launches)
    fused = [(synth.make_jpeg(w, h, seed=1600 + i, kind=i % 3, quality=80, ri=1,
                              tables=SETS[names[i % len(names)]]), False) for i, (w, h) in enumerate(shapes[1:4] * 8)]
    _decode(ca, gpu, fused, "fused", "per-image fused")
    stream = [(synth.make_jpeg(w, h, seed=1700 + i, quality=(70, 85, 90)[i % 3], ri=16,
                               tables=SETS[names[i % len(names)]]), False) for i, (w, h) in enumerate(shapes[:4] * 30)]
    _decode(ca, gpu, stream, "fused_stream", "per-image stream")
    pair = [(synth.make_jpeg(w, h, seed=1800 + i, ri=(3, 5, 4)[i % 3], tables=SETS[names[i % len(names)]]), False)
            for i, (w, h) in enumerate(shapes)]
    _decode(ca, gpu, pair, "pair", "per-image pair")


def test_decoder_alternating_selectors(ca, gpu):
    """One Decoder, one frame size, the selector sets in turn: its walk tables are cached by table contents and
    selectors (runtime.cpp) -- through the cooperative kernel (DRI = 4) and the walk route (DRI = 300)."""
    order = ["default", "swapped", "default", "crossed", "one_table", "crossed", "split_chroma", "default"]
    for w, h, ri, kernel in ((960, 720, 4, "coop_team"), (1280, 720, 300, "walk_mcu")):
        dec = ca.Decoder(gpu)
        for k, name in enumerate(order):
            jpeg = synth.make_jpeg(w, h, seed=1900 + ri + k, ri=ri, tables=SETS[name])
            data = ca.ImageData(jpeg)
            dec.decode_blocking(data)
            assert dec.last_kernel() == kernel, (ri, name, dec.last_kernel())
            _check_slot(dec.read_texture(w, h), _want(jpeg), k, f"decoder DRI={ri} {name}")


def test_three_pairs_falls_back(ca, gpu):
    """Three different (DC, AC) pairs: more than the walk tables hold (mcu_ok false), so the walk route is closed to
    the image -- the streamed batch kernel takes it instead; the cooperative kernel walks it symbol by symbol.  Whatever
    the route, bit-exact."""
    tp = synth.make_jpeg(960, 720, seed=2000, ri=30, tables=SETS["three_pairs"])
    base = [(j, False) for j in _frames(960, 720, 30, 3, 2010)]
    kernels = {}
    for what, items in (("alone", [(tp, False)] * 48), ("look-alike", _look_alikes(base, (tp, False), 48))):
        batch = ca.Batch(gpu)
        batch.upload([ca.ImageData(j) for j, _ in items])
        batch.decode()
        batch.wait()
        kernels[what] = batch.last_kernel()
        for i, (j, s) in enumerate(items):
            _check_slot(batch.read_output(i), _want(j, s), i, f"three_pairs {what}")
    for w, h, ri in ((960, 720, 4), (1280, 720, 300)):
        jpeg = synth.make_jpeg(w, h, seed=2020 + ri, ri=ri, tables=SETS["three_pairs"])
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        kernels[f"decoder DRI={ri}"] = dec.last_kernel()
        _check_slot(dec.read_texture(w, h), _want(jpeg), 0, f"three_pairs decoder DRI={ri}")
    assert kernels == {"alone": "fused_stream", "look-alike": "fused_stream", "decoder DRI=4": "coop_team",
                       "decoder DRI=300": "fused_stream"}, kernels
