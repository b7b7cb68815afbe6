"""Grayscale decode on the card: decode_fused_gray_kernel / decode_fused_gray_single_kernel behind Decoder and uniform
grayscale Batches (`fused_layout`), entropy_samples_kernel + composite_generic_kernel behind batches that mix grayscale
with colour layouts and behind the laboratory library's COMPEG_PIPELINE=split (`generic`).

Expectations are made on the host: gs.expectation (cs.predict -> cs.samples -> the luma replicated; equal to the oracle's
decode of the 4:4:4 twin wherever the twin can serve: tests/test_gray_stream.py) for the coefficient frames, and for real
encoders' files the oracle's own entropy and transform passes over the one-component metadata block, in the reference's
entropy mode, or the restatement over gs.from_jpeg's symbols in the standard one.  Every decode asserts last_kernel()."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import coef_stream as cs
import gray_stream as gs
from oracle import oracle as orc
from test_gray_stream import FIXTURES, fixture, pil_l

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ca():
    import compeg_amd
    return compeg_amd


@pytest.fixture(scope="module")
def gpu(ca):
    return ca.Gpu.open(0)


# ---- expectations ------------------------------------------------------------------------------------------------------

def _replicate(smp, mcus_w, mcus_h, w, h):
    out = np.zeros((mcus_h * 8, mcus_w * 8, 4), dtype=np.uint8)
    for m in range(smp.shape[0]):
        my, mx = divmod(m, mcus_w)
        out[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8, :3] = smp[m][:, :, None]
        out[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8, 3] = 255
    return out[:h, :w]


def file_expectation(ca, jpeg, standard):
    """A real encoder's file.  standard: the restatement over the file's own symbols.  Reference mode: the oracle's
    orc_huffman_pass over the one-component block, LUTs and preprocessed scan (generic over such a block; equal to
    cs.predict on the coefficient frames: test_gray_stream), then cs.samples, the luma replicated."""
    if standard:
        return gs.expectation(gs.from_jpeg(jpeg))
    img = ca.ImageData(jpeg, allow_grayscale=True)
    off, n = img.scan_range()
    sb = orc.ScanBuffer()
    try:
        sb.process(jpeg[off:off + n], img.parallelism())
    except orc.OracleError:
        pass   # (a count mismatch leaves the truncated result in place, as in the reference)
    words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32).copy()
    starts = np.frombuffer(sb.start_positions(), dtype=np.uint32).copy()
    md = np.frombuffer(img.metadata(), dtype=np.uint32)
    mcus = int(md[272]) * int(md[256])
    l2 = img.huffman_l2()
    bufs = [np.frombuffer(b, dtype=np.uint8).copy() for b in (img.metadata(), img.huffman_l1(), l2 or b"\0\0")]
    coef = np.zeros(max(1, mcus * 32), dtype=np.int32)
    orc.lib().orc_huffman_pass(bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, len(l2), words.ctypes.data, words.size,
                               starts.ctypes.data, starts.size, coef.ctypes.data, coef.size)
    full = np.zeros((mcus, 64), dtype=np.int32)
    full[:, :32] = coef[:mcus * 32].reshape(mcus, 32)
    w, h = img.width(), img.height()
    return _replicate(cs.samples(full), int(md[273]), -(-h // 8), w, h)


def noise_256():
    """PIL, 256 x 256 noise at quality 95 without DRI: one interval whose scan is longer than the 6144-word window cap."""
    from PIL import Image
    img = np.random.default_rng(9).integers(0, 256, (256, 256)).astype(np.uint8)
    out = io.BytesIO()
    Image.fromarray(img, "L").save(out, "JPEG", quality=95)
    j = out.getvalue()
    assert len(gs.file_scan(j)) > 6144 * 4
    return j


def coefficient_frames():
    """DRI none, 1, 2, 3 and 7 at widths odd, even and 1, both entropy modes (random_gray); every family at its own
    geometry; 40 x 24 MCUs with DRI 1: 960 intervals, fifteen waves, more than one workgroup."""
    own = {}
    for f in gs.cases():
        if f.family != "random_gray":
            own.setdefault(f.family, f)
    return [f for f in gs.cases() if f.family == "random_gray"] + list(own.values()) + [gs.random_gray(1, 40, False, mcus=960)]


_FILES = None


def files():
    """(name, bytes, entropy mode, expectation) of the real encoders' files: the six fixtures (1 x 1000 and 1000 x 1: one MCU
    across or down; 10 x 10: cut both ways; the two 2x2-sampled ones), PIL's 8 x 8 and the noise image, in both modes."""
    global _FILES
    if _FILES is None:
        import compeg_amd as ca
        named = [(n, fixture(n)) for n in FIXTURES] + [("pil_8x8", pil_l(8, 8, 95, 0)), ("pil_noise_256", noise_256())]
        _FILES = [(n, j, std, file_expectation(ca, j, std)) for n, j in named for std in (False, True)]
    return _FILES


def decode_all_ways(ca, gpu, jpeg, standard, w, h):
    """-> [(how, kernel, pixels)]: host and device preprocessing, blocking and start_decode."""
    out = []
    img = ca.ImageData(jpeg, allow_grayscale=True, standard_entropy=standard)
    assert img.components() == 1
    for device in (False, True):
        dec = ca.Decoder(gpu)
        dec.set_device_preprocess(device)
        for how in ("blocking", "start_decode"):
            if how == "blocking":
                dec.decode_blocking(img)
            else:
                dec.start_decode(img).wait()
            out.append((f"{'device' if device else 'host'} preprocessing, {how}", dec.last_kernel(), dec.read_texture(w, h)))
    return out


# ---- Decoder -----------------------------------------------------------------------------------------------------------

def test_decoder_on_real_files(ca, gpu):
    fails = []
    for name, j, std, want in files():
        for how, kernel, got in decode_all_ways(ca, gpu, j, std, want.shape[1], want.shape[0]):
            what = f"{name} ({'standard' if std else 'reference'} entropy, {how})"
            if kernel != "fused_layout":
                fails.append(f"{what}: last_kernel() = {kernel}")
            if not np.array_equal(got, want):
                fails.append(f"{what}: {int((got != want).any(axis=2).sum())} pixels differ")
    assert not fails, "\n".join(fails)


def test_decoder_on_coefficient_frames(ca, gpu):
    fails = []
    frames = coefficient_frames()
    assert {f.ri for f in frames} >= {0, 1, 2, 3, 7} and {f.mcus_w for f in frames} >= {1, 2, 5, 6, 40}
    assert {f.standard for f in frames} == {False, True}
    for f in frames:
        want = gs.expectation(f)
        for how, kernel, got in decode_all_ways(ca, gpu, f.jpeg(), f.standard, f.w, f.h):
            if kernel != "fused_layout":
                fails.append(f"{f.name} ({how}): last_kernel() = {kernel}")
            if not np.array_equal(got, want):
                fails.append(f"{f.name} ({how}): {int((got != want).any(axis=2).sum())} pixels differ")
    assert not fails, "\n".join(fails)


def test_grayscale_decodes_to_its_twin_on_the_card(ca, gpu):
    """The definition itself, through the two kernels: decode_fused_gray_kernel's pixels of a frame are
    decode_fused_444_kernel's of its twin (frames whose readers never run dry)."""
    dec = ca.Decoder(gpu)
    for f in [f for f in gs.cases() if f.family == "random_gray"]:
        dec.decode_blocking(ca.ImageData(f.jpeg(), **f.image_kw()))
        got, kernel = dec.read_texture(f.w, f.h), dec.last_kernel()
        t = gs.twin(f)
        dec.decode_blocking(ca.ImageData(t.jpeg(), **t.image_kw()))
        assert (kernel, dec.last_kernel()) == ("fused_layout", "fused_layout")
        assert np.array_equal(got, dec.read_texture(t.w, t.h)), f.name


# ---- Batch -------------------------------------------------------------------------------------------------------------

def uniform_batch(standard):
    """Grayscale files of mixed sizes in one entropy mode: (bytes, expectation)."""
    out = [(j, want) for _, j, std, want in files() if std == standard]
    out += [(f.jpeg(), gs.expectation(f)) for f in coefficient_frames() if f.standard == standard and f.mcus <= 64]
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_uniform_grayscale_batches(ca, gpu, mode):
    fails = []
    for standard in (False, True):
        items = uniform_batch(standard)
        assert {w.shape[:2] for _, w in items} >= {(8, 8), (1000, 1), (1, 1000), (10, 10)}
        jpegs = [j for j, _ in items]
        pinned = ca.HostBuffer(sum(len(j) + 64 for j in jpegs))
        for feed in ("images", "pageable", "pinned", "begin", "chunk3"):
            batch = ca.Batch(gpu)
            batch.set_device_preprocess(mode)
            if feed == "images":
                batch.upload([ca.ImageData(j, allow_grayscale=True, standard_entropy=standard) for j in jpegs])
            elif feed == "pinned":
                batch.upload_jpegs(pinned.place(jpegs), allow_grayscale=True, standard_entropy=standard)
            elif feed == "begin":
                batch.upload_jpegs_begin(jpegs, allow_grayscale=True, standard_entropy=standard)
                batch.upload_end()
            else:
                batch.upload_jpegs(jpegs, allow_grayscale=True, standard_entropy=standard)
            if feed == "chunk3":
                batch.set_chunk(3)
            batch.decode()
            batch.wait()
            what = f"mode {mode}, {'standard' if standard else 'reference'} entropy, {feed}"
            if batch.last_kernel() != "fused_layout":
                fails.append(f"{what}: last_kernel() = {batch.last_kernel()}")
            fails += [f"{what}: slot {i}: pixels differ" for i, (_, want) in enumerate(items) if not np.array_equal(batch.read_output(i), want)]
            del batch
        pinned.close()
    assert not fails, "\n".join(fails)


def mixed_batch():
    """Grayscale beside 4:2:2 and 4:2:0: (bytes, expectation), reference entropy."""
    out = [(j, want) for n, j, std, want in files() if not std and n != "pil_noise_256"]
    out += [(f.jpeg(), gs.expectation(f)) for f in coefficient_frames() if not f.standard and f.mcus <= 64][:6]
    for name in ("texture/edge/422/reference/dri4", "texture/edge/420/reference/dri4", "positions/short/422/reference/dri4"):
        c = cs.case(name)
        out.append((c.jpeg(), orc.ImageData(c.jpeg(), **c.image_kw()).decode()))
    return out[::2] + out[1::2]   # (the layouts interleaved)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mixed_batches_take_the_generic_route(ca, gpu, mode):
    items = mixed_batch()
    batch = ca.Batch(gpu)
    batch.set_device_preprocess(mode)
    for feed in ("images", "jpegs"):
        if feed == "images":
            batch.upload([ca.ImageData(j, allow_grayscale=True, allow_sampling=True) for j, _ in items])
        else:
            batch.upload_jpegs([j for j, _ in items], allow_grayscale=True, allow_sampling=True)
        batch.decode()
        batch.wait()
        assert batch.last_kernel() == "generic", (mode, feed)
        bad = [i for i, (_, want) in enumerate(items) if not np.array_equal(batch.read_output(i), want)]
        assert not bad, f"mode {mode}, {feed}: slots {bad} differ"


# ---- the packs read what the decoder wrote -----------------------------------------------------------------------------

_PACK_CODE = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import torch   # (before the library: both bring a HIP runtime and the one loaded first serves both)
import compeg_amd as ca
import coef_stream as cs
import gray_stream as gs
import nhwc_reference as nr
from oracle import oracle as orc
gpu = ca.Gpu.open(0)
f = gs.case("random_gray/short/gray/reference/dri2/w5")
want = gs.expectation(f)
dec = ca.Decoder(gpu)
dec.decode_blocking(ca.ImageData(f.jpeg(), **f.image_kw()))
assert dec.last_kernel() == "fused_layout", dec.last_kernel()
planes = torch.full((3, f.h, f.w), 7, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
dec.pack_tensor(planes, dtype="u8")
dec.decode_blocking(ca.ImageData(f.jpeg(), **f.image_kw()))   # (the next decode runs behind the pack: waits for it)
torch.cuda.synchronize()
got = planes.cpu().numpy()
assert np.array_equal(got[0], want[..., 0]), "plane 0 is not the luma"
assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0]), "the planes differ"
# channels-last over a grayscale and a colour slot
c = cs.case("texture/edge/422/reference/dri4")
colour = orc.ImageData(c.jpeg()).decode()
batch = ca.Batch(gpu)
batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()), ca.ImageData(c.jpeg())])
batch.decode()
assert batch.last_kernel() == "generic", batch.last_kernel()
size = (24, 20)
dst = torch.full((2, size[1], size[0], 3), 7, dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
scale, bias = nr.fr.params("u8")
batch.pack_tensor_nhwc(dst, size, channels=3, dtype="u8", scale=scale, bias=bias)
batch.wait()
torch.cuda.synchronize()
for slot, rgba in enumerate((want, colour)):
    expected = nr.expected(rgba, size, 1, "u8", scale, bias, channels=3)
    assert np.array_equal(dst[slot].cpu().numpy(), np.asarray(expected)), f"channels-last slot {slot} differs"
print("packs done")
'''


def test_tensor_packs_of_grayscale_frames(ca):
    """After a grayscale decode pack_tensor(dtype="u8") gives three equal planes that equal the luma, and
    Batch.pack_tensor_nhwc(channels=3) over a grayscale and a colour slot matches tests/nhwc_reference.py fed the expected
    RGBA.  In a process of its own that imports torch before the library (tests/gpu_nhwc_worker.py: why)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _PACK_CODE, root], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "packs done" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])


# ---- the laboratory library's two-kernel pipeline ----------------------------------------------------------------------

_LAB_CODE = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import compeg_amd as ca
import gray_stream as gs
import test_gpu_gray as t
gpu = ca.Gpu.open(0)
dec = ca.Decoder(gpu)
for f in t.coefficient_frames():
    dec.decode_blocking(ca.ImageData(f.jpeg(), **f.image_kw()))
    print(json.dumps([f.name, dec.last_kernel(), bool(np.array_equal(dec.read_texture(f.w, f.h), gs.expectation(f)))]), flush=True)
for name, j, std, want in t.files():
    dec.decode_blocking(ca.ImageData(j, allow_grayscale=True, standard_entropy=std))
    print(json.dumps([name, dec.last_kernel(), bool(np.array_equal(dec.read_texture(want.shape[1], want.shape[0]), want))]), flush=True)
for std in (False, True):
    items = t.uniform_batch(std)
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j, allow_grayscale=True, standard_entropy=std) for j, _ in items])
    batch.decode()
    batch.wait()
    print(json.dumps(["batch", batch.last_kernel(), all(np.array_equal(batch.read_output(i), w) for i, (_, w) in enumerate(items))]), flush=True)
print("lab done")
'''


def test_lab_split_pipeline_decodes_grayscale_through_the_generic_route(ca, gpu):
    lab = os.path.join(os.path.dirname(ca.LIB_PATH), "libcompeg_hip_lab.so")
    assert os.path.exists(lab), "make -C compeg_amd/csrc lab (__graft_entry__.build() does)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LAB_CODE, root], env=dict(os.environ, COMPEG_LIB=lab, COMPEG_PIPELINE="split"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lab done" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("[")]
    assert len(rows) == len(coefficient_frames()) + len(files()) + 2
    bad = [row for row in rows if row[1] != "generic" or not row[2]]
    assert not bad, bad
