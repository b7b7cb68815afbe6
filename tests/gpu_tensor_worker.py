"""The GPU cases of tests/test_gpu_tensor.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: bench.py has the same order, and
test_zero_copy_consumer_and_caller_stream its own process for the same reason).

    python tests/gpu_tensor_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in, the decodes on the
gpu's own stream or on another one.  Every element is compared with the oracle's RGBA put through the header's
formula (tests/tensor_reference.py).  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

SIZES = ((16, 8), (17, 9), (50, 26), (330, 70))
SENTINEL = 0x5C
ADMISSIBLE = {(w, h): [k for k in (1, 2, 4, 8) if w >= k and h >= k] for w, h in SIZES}

torch = ca = tr = ne = gpu = stream = None   # set by main(): torch first


class Raises:
    """with Raises("words"): the library's INVALID_ARG whose message has the words."""

    def __init__(self, words=""):
        self.words = words

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        assert kind is not None and issubclass(kind, ca.Error), "no error raised"
        assert value.code == ca.E_INVALID_ARG and str(value) and self.words in str(value), (value.code, str(value))
        return True

def _torch_type(dtype):
    return {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dtype]


def _host(t, dtype):
    """A torch tensor's elements as tensor_reference compares them (bf16: the bit patterns)."""
    if dtype == "bf16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _params(dtype, identity=False):
    if identity:
        return tr.IDENTITY
    return (tr.U8_SCALE, tr.U8_BIAS) if dtype == "u8" else (tr.IMAGENET_SCALE, tr.IMAGENET_BIAS)


def _check(got, want, dtype, what):
    assert tr.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


def _pack_and_check(dec, rgba, k, dtype, order, what, identity=False):
    h, w = rgba.shape[:2]
    scale, bias = _params(dtype, identity)
    shape, nbytes = ca.tensor_shape(w, h, dtype=dtype, downscale=k)
    assert shape == (3, h // k, w // k)
    dst = torch.empty(shape, dtype=_torch_type(dtype), device="cuda")
    assert dst.numel() * dst.element_size() == nbytes
    dec.pack_tensor(dst, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(_host(dst, dtype), tr.expected(rgba, k, dtype, scale, bias, order), dtype, what)


def decoder_422_every_dtype(w, h, k):
    jpeg, rgba = tr.frame(w, h)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    kernel = dec.last_kernel()
    for n, dtype in enumerate(tr.DTYPES):
        _pack_and_check(dec, rgba, k, dtype, ("rgb", "bgr")[(n + k) % 2], f"{w}x{h} k={k} {dtype}")
    if k == 1:
        # identity: the oracle's R, G and B planes byte for byte
        _pack_and_check(dec, rgba, 1, "u8", "rgb", f"{w}x{h} identity", identity=True)
    assert dec.last_kernel() == kernel   # (a pack changes nothing the decoder reports)


def decoder_rejections():
    dec = ca.Decoder(gpu)
    dst = torch.empty(3 * 64 * 64, dtype=torch.float16, device="cuda")
    with Raises("nothing decoded"):
        dec.pack_tensor(dst, dtype="f16", hip_stream=stream.cuda_stream)
    jpeg, _ = tr.frame(7, 5)
    dec.decode_blocking(ca.ImageData(jpeg))
    with Raises("7x5"):
        dec.pack_tensor(dst, dtype="f16", downscale=8, hip_stream=stream.cuda_stream)
    # too small by one element; an f16 destination at an odd address
    with Raises("dst_bytes"):
        dec.pack_tensor((dst.data_ptr(), 3 * 5 * 7 * 2 - 2), dtype="f16", hip_stream=stream.cuda_stream)
    with Raises("aligned"):
        dec.pack_tensor((dst.data_ptr() + 1, 4096), dtype="f16", hip_stream=stream.cuda_stream)
    with Raises(""):
        dec.pack_tensor((0, 4096), dtype="f16", hip_stream=stream.cuda_stream)
    dec.pack_tensor((dst.data_ptr(), 3 * 5 * 7 * 2), dtype="f16", hip_stream=stream.cuda_stream)   # exactly enough
    stream.synchronize()


def texture_that_did_not_shrink():
    """330x70, then 50x26 with the same decoder: the texture keeps its extent and pitch, the pack takes the last frame's."""
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(tr.frame(330, 70)[0]))
    jpeg, rgba = tr.frame(50, 26, seed=9)
    op = dec.decode_blocking(ca.ImageData(jpeg))
    assert not op.texture_changed()
    tex = dec.texture()
    assert (tex.width, tex.height) == (330, 70)
    for k, dtype in ((1, "u8"), (2, "f16"), (1, "f32")):
        _pack_and_check(dec, rgba, k, dtype, "rgb", f"50x26 in a 330x70 texture, k={k} {dtype}")


def batch_of_five_frames_inside_sentinels(k):
    """k = 2: planes of 325 elements -- rows, planes and images begin at every alignment; the destination lies one
    element into a sentinel-filled allocation."""
    frames = [tr.frame(50, 26, seed=20 + i) for i in range(5)]
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode()
    kernel = batch.last_kernel()
    for dtype in ("u8", "f16", "f32"):
        scale, bias = _params(dtype)
        shape, per_image = ca.tensor_shape(50, 26, dtype=dtype, downscale=k)
        needed, esize = 5 * per_image, tr.ELEM_BYTES[dtype]
        buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor((buf.data_ptr() + 64 + esize, needed), dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
        batch.wait()   # (covers the pack)
        raw = buf.cpu().numpy().tobytes()
        lo, hi = 64 + esize, 64 + esize + needed
        assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{dtype}: sentinels overwritten"
        got = tr.from_bytes(raw[lo:hi], dtype, (5,) + shape)
        for i, (_, rgba) in enumerate(frames):
            _check(got[i], tr.expected(rgba, k, dtype, scale, bias), dtype, f"k={k} {dtype} slot {i}")
    assert batch.last_kernel() == kernel
    n, total, _, _ = batch.timing()
    assert n == 1   # (one decode; the packs recorded no timing events)


def batch_rejections():
    dst = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(tr.frame(50, 26)[0]), ca.ImageData(tr.frame(50, 26, seed=4)[0])])
    with Raises("nothing decoded"):
        batch.pack_tensor(dst, dtype="u8", hip_stream=stream.cuda_stream)
    mixed = ca.Batch(gpu)
    mixed.upload([ca.ImageData(tr.frame(50, 26)[0]), ca.ImageData(tr.frame(66, 26)[0])])
    mixed.decode()
    with Raises("one size"):
        mixed.pack_tensor(dst, dtype="u8", hip_stream=stream.cuda_stream)
    mixed.wait()


def other_layouts(w, h, sampling):
    jpeg, rgba = tr.frame(w, h, sampling=sampling)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg, allow_sampling=True))
    for k in (1, 2):
        _pack_and_check(dec, rgba, k, "f16", "rgb", f"{w}x{h} {sampling} k={k}")


def wide_row():
    """65528 x 8, k = 8: one output row of 8191 elements -- the widest image the format has."""
    jpeg, rgba = tr.frame(65528, 8)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    _pack_and_check(dec, rgba, 8, "f16", "rgb", "65528x8 k=8")


def decoder_ordering_without_host_waits():
    """enqueue(img1, A), pack(dst1, B), enqueue(img2, A), pack(dst2, B): every pack behind its decode, the second decode
    behind the first pack, with nothing but the streams' own order and the library's events."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    (j1, r1), (j2, r2) = tr.frame(640, 360, seed=31), tr.frame(640, 360, seed=32)
    img1, img2 = ca.ImageData(j1), ca.ImageData(j2)
    scale, bias = tr.IMAGENET_SCALE, tr.IMAGENET_BIAS
    dst1 = torch.zeros((3, 360, 640), dtype=torch.float16, device="cuda")
    dst2 = torch.zeros((3, 360, 640), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    dec = ca.Decoder(gpu)
    dec.enqueue(img1, a.cuda_stream)
    dec.pack_tensor(dst1, dtype="f16", scale=scale, bias=bias, hip_stream=b.cuda_stream)
    dec.enqueue(img2, a.cuda_stream)
    dec.pack_tensor(dst2, dtype="f16", scale=scale, bias=bias, hip_stream=b.cuda_stream)
    a.synchronize()
    b.synchronize()
    _check(dst1.cpu().numpy(), tr.expected(r1, 1, "f16", scale, bias), "f16", "first frame")
    _check(dst2.cpu().numpy(), tr.expected(r2, 1, "f16", scale, bias), "f16", "second frame")


def batch_ordering_across_streams():
    """One batch decoded on A and packed on B, then batch.wait()."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    frames = [tr.frame(640, 360, seed=31), tr.frame(640, 360, seed=32)]
    scale, bias = tr.IMAGENET_SCALE, tr.IMAGENET_BIAS
    dst = torch.zeros((2, 3, 180, 320), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode(a.cuda_stream)
    batch.pack_tensor(dst, dtype="f16", downscale=2, scale=scale, bias=bias, hip_stream=b.cuda_stream)
    batch.wait()
    got = dst.cpu().numpy()
    for i, (_, rgba) in enumerate(frames):
        _check(got[i], tr.expected(rgba, 2, "f16", scale, bias), "f16", f"slot {i}")
    # ... and a decode behind the pack, on the first stream again, still gives the frames
    batch.decode(a.cuda_stream)
    batch.wait()
    assert np.array_equal(batch.read_output(1), frames[1][1])


_decoded = {}


def _edge_decoder(frame):
    """The decoder that holds numeric_edges' frame, decoded once for all the sets."""
    if frame not in _decoded:
        jpeg, rgba = ne.FRAMES[frame]()
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        _decoded[frame] = (dec, rgba)
    return _decoded[frame]


def numeric_edges(name):
    """One (scale, bias) set of tests/numeric_edges.py: the ramp at k = 1, the noisy frame at k = 2 and 8, every element
    against the formula -- ties, subnormals, overflow, infinities, the clamp, denormal float32 on the device's own
    conversions."""
    dtypes, scale, bias = ne.SETS[name]
    n = 0
    for dtype in dtypes:
        for frame, k in ne.PACKS:
            dec, rgba = _edge_decoder(frame)
            h, w = rgba.shape[:2]
            order = ("rgb", "bgr")[n % 2]
            n += 1
            dst = torch.empty((3, h // k, w // k), dtype=_torch_type(dtype), device="cuda")
            dec.pack_tensor(dst, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream)
            stream.synchronize()
            _check(_host(dst, dtype), ne.expected(rgba, k, name, dtype, order), dtype, f"{name} {frame} k={k} {dtype} {order}")


def numeric_edges_batch():
    """The ramp and its mirror image as a batch, f16 subnormals and the u8 clamp, one element into a sentinel buffer."""
    frames = [ne.ramp(), ne.ramp_flipped()]
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode()
    for name in ("f16_subnormal", "u8_clamp"):
        (dtype,), scale, bias = ne.SETS[name]
        shape, per_image = ca.tensor_shape(ne.RAMP_W, ne.RAMP_H, dtype=dtype, downscale=1)
        needed, esize = 2 * per_image, tr.ELEM_BYTES[dtype]
        buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor((buf.data_ptr() + 64 + esize, needed), dtype=dtype, downscale=1, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
        batch.wait()   # (covers the pack)
        raw = buf.cpu().numpy().tobytes()
        lo, hi = 64 + esize, 64 + esize + needed
        assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{name}: sentinels overwritten"
        got = tr.from_bytes(raw[lo:hi], dtype, (2,) + shape)
        for i, (_, rgba) in enumerate(frames):
            _check(got[i], ne.expected(rgba, 1, name, dtype), dtype, f"{name} slot {i}")


# (tests/numeric_edges.py's sets by name: importing it here would bring the oracle and the encoder in front of torch)
EDGE_SETS = ("f16_ties", "f16_overflow", "f16_subnormal", "f16_inf", "bf16_ties", "bf16_overflow", "f32_denormal", "f32_inf", "u8_ties",
             "u8_clamp", "u8_clamp2", "imagenet_f32")


def _cases():
    cases = {}
    for w, h in SIZES:
        for k in ADMISSIBLE[(w, h)]:
            cases[f"decoder_422_every_dtype[{w}x{h}-k{k}]"] = (decoder_422_every_dtype, (w, h, k))
    cases["decoder_rejections"] = (decoder_rejections, ())
    cases["texture_that_did_not_shrink"] = (texture_that_did_not_shrink, ())
    for k in (2, 1):
        cases[f"batch_of_five_frames_inside_sentinels[k{k}]"] = (batch_of_five_frames_inside_sentinels, (k,))
    cases["batch_rejections"] = (batch_rejections, ())
    cases["other_layouts[420]"] = (other_layouts, (33, 17, (2, 2)))
    cases["other_layouts[444]"] = (other_layouts, (24, 24, (1, 1)))
    cases["wide_row"] = (wide_row, ())
    cases["decoder_ordering_without_host_waits"] = (decoder_ordering_without_host_waits, ())
    cases["batch_ordering_across_streams"] = (batch_ordering_across_streams, ())
    for name in EDGE_SETS:
        cases[f"numeric_edges[{name}]"] = (numeric_edges, (name,))
    cases["numeric_edges_batch"] = (numeric_edges_batch, ())
    return cases


CASES = _cases()


def main(out_path):
    global torch, ca, tr, ne, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import tensor_reference as tr
    import numeric_edges as ne
    assert tuple(ne.SETS) == EDGE_SETS and ne.denormals_kept()
    gpu = ca.Gpu.open(0)
    stream = torch.cuda.Stream()
    results = {}
    for name, (fn, args) in CASES.items():
        try:
            fn(*args)
            results[name] = None
        except ca.Error as e:
            results[name] = f"compeg_amd.Error {e.code}: {e}\n{traceback.format_exc()}"
            if e.code == ca.E_HIP:   # the device said no: nothing more is started on it
                break
        except Exception:
            results[name] = traceback.format_exc()
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
