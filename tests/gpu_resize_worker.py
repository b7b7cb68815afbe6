"""The GPU cases of tests/test_gpu_resize.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: tests/gpu_tensor_worker.py has the same order).

    python tests/gpu_resize_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in, the decodes on the
gpu's own stream or on another one.  Every element is compared with the oracle's RGBA put through the header's
formula (tests/resize_reference.py).  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

SIZES = ((16, 8), (17, 9), (50, 26), (330, 70))
FIVE = ((16, 8), (17, 9), (50, 26), (66, 26), (330, 70))
SENTINEL = 0x5C
ADMISSIBLE = {(w, h): [k for k in (1, 2, 4, 8) if w >= k and h >= k] for w, h in SIZES}

torch = ca = rr = ne = gpu = stream = None   # set by main(): torch first


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
    """A torch tensor's elements as the reference compares them (bf16: the bit patterns)."""
    if dtype == "bf16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _check(got, want, dtype, what):
    assert rr.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


def _pack_and_check(dec, rgba, size, k, dtype, order, filter, what, crop=None):
    h, w = rgba.shape[:2]
    scale, bias = rr.params(dtype)
    shape, nbytes, pre = ca.resized_tensor_shape(w, h, size, dtype=dtype, downscale=k, filter=filter, crop=crop)
    assert shape == (3, size[1], size[0]) and pre == rr.pre_extent(w, h, k, crop)[::-1]
    dst = torch.empty(shape, dtype=_torch_type(dtype), device="cuda")
    assert dst.numel() * dst.element_size() == nbytes
    dec.pack_tensor_resized(dst, size, crop=crop, filter=filter, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                            hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(_host(dst, dtype), rr.expected(rgba, size, k, dtype, scale, bias, order, filter, crop), dtype, what)


def decoder_every_dtype_and_filter(w, h, k):
    """The identity extent, one smaller, and 64 x 64 (larger than every prefiltered source here but 330 wide)."""
    jpeg, rgba = rr.frame(w, h)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    kernel = dec.last_kernel()
    pw, ph = rr.pre_extent(w, h, k)
    n = 0
    for size in ((pw, ph), (max(1, pw * 2 // 3), max(1, ph * 2 // 3)), (64, 64)):
        for dtype in rr.DTYPES:
            for filter in rr.FILTERS:
                n += 1
                _pack_and_check(dec, rgba, size, k, dtype, ("rgb", "bgr")[n % 2], filter, f"{w}x{h} k={k} -> {size} {dtype} {filter}")
    # ... and at the identity extent it is pack_tensor itself
    for filter in rr.FILTERS:
        a = torch.empty((3, ph, pw), dtype=torch.float32, device="cuda")
        b = torch.empty((3, ph, pw), dtype=torch.float32, device="cuda")
        dec.pack_tensor(a, dtype="f32", downscale=k, scale=rr.IMAGENET_SCALE, bias=rr.IMAGENET_BIAS, hip_stream=stream.cuda_stream)
        dec.pack_tensor_resized(b, (pw, ph), filter=filter, dtype="f32", downscale=k, scale=rr.IMAGENET_SCALE, bias=rr.IMAGENET_BIAS,
                                hip_stream=stream.cuda_stream)
        stream.synchronize()
        assert torch.equal(a, b), f"{filter}: the identity extent differs from pack_tensor"
    assert dec.last_kernel() == kernel   # (a pack changes nothing the decoder reports)


def decoder_crops():
    """330x70, u8 with a scale and bias that round and clamp."""
    jpeg, rgba = rr.frame(330, 70)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    for k in (1, 2, 8):
        crops = [None, (330 - 97, 70 - 33, 97, 33), (5, 3, 201, 45), (330 - k, 70 - k, k, k)]
        if k == 1:
            crops.append((129, 30, 1, 1))
        for n, crop in enumerate(crops):
            for size in ((17, 9), (64, 64)):
                for filter in rr.FILTERS:
                    _pack_and_check(dec, rgba, size, k, "u8", ("rgb", "bgr")[n % 2], filter, f"crop {crop} k={k} -> {size} {filter}", crop=crop)


def _five():
    frames = [rr.frame(w, h, seed=20 + i) for i, (w, h) in enumerate(FIVE)]
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode()
    return frames, batch


def batch_of_five_sizes_inside_sentinels():
    """The destination lies one element into a sentinel-filled allocation: rows, planes and images begin at every alignment."""
    frames, batch = _five()
    kernel, size = batch.last_kernel(), (24, 20)
    for dtype in ("u8", "f16", "f32"):
        for filter, k in (("bilinear", 1), ("nearest", 1), ("bilinear", 2)):
            scale, bias = rr.params(dtype)
            shape, per_image, _ = ca.resized_tensor_shape(16, 8, size, dtype=dtype, downscale=k, filter=filter)
            needed, esize = 5 * per_image, rr.ELEM_BYTES[dtype]
            buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            batch.pack_tensor_resized((buf.data_ptr() + 64 + esize, needed), size, filter=filter, dtype=dtype, downscale=k, scale=scale, bias=bias,
                                      hip_stream=stream.cuda_stream)
            batch.wait()   # (covers the pack)
            raw = buf.cpu().numpy().tobytes()
            lo, hi = 64 + esize, 64 + esize + needed
            assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{dtype}: sentinels overwritten"
            got = rr.from_bytes(raw[lo:hi], dtype, (5,) + shape)
            for i, (_, rgba) in enumerate(frames):
                _check(got[i], rr.expected(rgba, size, k, dtype, scale, bias, "rgb", filter), dtype, f"{dtype} {filter} k={k} slot {i}")
    assert batch.last_kernel() == kernel
    n, total, _, _ = batch.timing()
    assert n == 1   # (one decode; the packs recorded no timing events)
    with Raises("one size"):
        batch.pack_tensor(torch.empty(1 << 16, dtype=torch.uint8, device="cuda"), dtype="u8", hip_stream=stream.cuda_stream)
    batch.wait()


def batch_two_packs_back_to_back_with_their_own_crops():
    """Two packs recorded one behind the other with different crops and no host wait in between: each sees its own records."""
    frames, batch = _five()
    size, scale, bias = (24, 20), rr.IMAGENET_SCALE, rr.IMAGENET_BIAS
    first = [(1, 1, 15, 7), (0, 0, 17, 9), (3, 1, 45, 21), (2, 0, 64, 26), (101, 3, 200, 64)]
    second = [(0, 0, 8, 8), (5, 2, 12, 7), (25, 13, 25, 13), (1, 1, 33, 17), (0, 0, 330, 70)]
    dst1 = torch.zeros((5, 3, 20, 24), dtype=torch.float16, device="cuda")
    dst2 = torch.zeros((5, 3, 20, 24), dtype=torch.float16, device="cuda")
    dst3 = torch.zeros((5, 3, 20, 24), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    batch.pack_tensor_resized(dst1, size, crops=first, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_resized(dst2, size, crops=second, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_resized(dst3, size, crops=(0, 0, 16, 8), dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)   # one for all
    batch.wait()
    for dst, crops, what in ((dst1, first, "first"), (dst2, second, "second"), (dst3, [(0, 0, 16, 8)] * 5, "third")):
        got = dst.cpu().numpy()
        for i, (_, rgba) in enumerate(frames):
            _check(got[i], rr.expected(rgba, size, 1, "f16", scale, bias, crop=crops[i]), "f16", f"{what} pack, slot {i}")
    with Raises("crop"):
        batch.pack_tensor_resized(dst1, size, crops=(0, 0, 17, 8), dtype="f16", hip_stream=stream.cuda_stream)   # leaves image 0
    with Raises("image 1"):
        batch.pack_tensor_resized(dst1, size, crops=[(0, 0, 16, 8), (0, 0, 17, 10)] + first[2:], dtype="f16", hip_stream=stream.cuda_stream)
    with Raises(""):
        batch.pack_tensor_resized(dst1, size, crops=first[:4], dtype="f16", hip_stream=stream.cuda_stream)
    batch.wait()


def texture_that_did_not_shrink():
    """330x70, then 50x26 with the same decoder: the texture keeps its extent and pitch, the pack takes the last frame's."""
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(rr.frame(330, 70)[0]))
    jpeg, rgba = rr.frame(50, 26, seed=9)
    op = dec.decode_blocking(ca.ImageData(jpeg))
    assert not op.texture_changed()
    tex = dec.texture()
    assert (tex.width, tex.height) == (330, 70)
    for k, dtype, size in ((1, "u8", (64, 64)), (2, "f16", (25, 13)), (1, "f32", (31, 13))):
        _pack_and_check(dec, rgba, size, k, dtype, "rgb", "bilinear", f"50x26 in a 330x70 texture, k={k} {dtype}")
    with Raises("crop"):   # inside the texture, outside the frame
        dec.pack_tensor_resized(torch.empty(3 * 64 * 64, dtype=torch.float16, device="cuda"), (8, 8), crop=(40, 0, 20, 20),
                                hip_stream=stream.cuda_stream)


def other_layouts(w, h, sampling):
    jpeg, rgba = rr.frame(w, h, sampling=sampling)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg, allow_sampling=True))
    for k, size in ((1, (24, 20)), (2, (31, 13))):
        _pack_and_check(dec, rgba, size, k, "f16", "rgb", "bilinear", f"{w}x{h} {sampling} k={k}")


def wide_row():
    """65528 x 8, k = 8: a prefiltered row of 8191 elements -- the widest image the format has."""
    jpeg, rgba = rr.frame(65528, 8)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    for size in ((8191, 1), (4000, 2)):
        _pack_and_check(dec, rgba, size, 8, "f16", "rgb", "bilinear", f"65528x8 k=8 -> {size}")


def decoder_ordering_without_host_waits():
    """enqueue(img1, A), pack(dst1, B), enqueue(img2, A), pack(dst2, B): every pack behind its decode, the second decode
    behind the first pack, with nothing but the streams' own order and the library's events."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    (j1, r1), (j2, r2) = rr.frame(640, 360, seed=31), rr.frame(640, 360, seed=32)
    img1, img2 = ca.ImageData(j1), ca.ImageData(j2)
    scale, bias, size = rr.IMAGENET_SCALE, rr.IMAGENET_BIAS, (224, 224)
    dst1 = torch.zeros((3, 224, 224), dtype=torch.float16, device="cuda")
    dst2 = torch.zeros((3, 224, 224), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    dec = ca.Decoder(gpu)
    dec.enqueue(img1, a.cuda_stream)
    dec.pack_tensor_resized(dst1, size, dtype="f16", scale=scale, bias=bias, hip_stream=b.cuda_stream)
    dec.enqueue(img2, a.cuda_stream)
    dec.pack_tensor_resized(dst2, size, dtype="f16", scale=scale, bias=bias, hip_stream=b.cuda_stream)
    a.synchronize()
    b.synchronize()
    _check(dst1.cpu().numpy(), rr.expected(r1, size, 1, "f16", scale, bias), "f16", "first frame")
    _check(dst2.cpu().numpy(), rr.expected(r2, size, 1, "f16", scale, bias), "f16", "second frame")


def batch_ordering_across_streams():
    """One batch decoded on A and packed on B, then batch.wait()."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    frames = [rr.frame(640, 360, seed=31), rr.frame(640, 360, seed=32)]
    scale, bias, size = rr.IMAGENET_SCALE, rr.IMAGENET_BIAS, (224, 224)
    dst = torch.zeros((2, 3, 224, 224), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode(a.cuda_stream)
    batch.pack_tensor_resized(dst, size, dtype="f16", downscale=2, scale=scale, bias=bias, hip_stream=b.cuda_stream)
    batch.wait()
    got = dst.cpu().numpy()
    for i, (_, rgba) in enumerate(frames):
        _check(got[i], rr.expected(rgba, size, 2, "f16", scale, bias), "f16", f"slot {i}")
    # ... and a decode behind the pack, on the first stream again, still gives the frames
    batch.decode(a.cuda_stream)
    batch.wait()
    assert np.array_equal(batch.read_output(1), frames[1][1])


def rejections():
    dec = ca.Decoder(gpu)
    dst = torch.empty(3 * 64 * 64, dtype=torch.float16, device="cuda")
    with Raises("nothing decoded"):
        dec.pack_tensor_resized(dst, (8, 8), hip_stream=stream.cuda_stream)
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(rr.frame(50, 26)[0]), ca.ImageData(rr.frame(66, 26)[0])])
    with Raises("nothing decoded"):
        batch.pack_tensor_resized(dst, (8, 8), hip_stream=stream.cuda_stream)
    jpeg, _ = rr.frame(7, 5)
    dec.decode_blocking(ca.ImageData(jpeg))
    with Raises("7x5"):
        dec.pack_tensor_resized(dst, (8, 8), downscale=8, hip_stream=stream.cuda_stream)
    with Raises("crop"):
        dec.pack_tensor_resized(dst, (8, 8), crop=(4, 0, 4, 5), hip_stream=stream.cuda_stream)
    with Raises("crop"):
        dec.pack_tensor_resized(dst, (8, 8), crop=(0xffffffff, 0, 2, 2), hip_stream=stream.cuda_stream)
    with Raises("output size"):
        dec.pack_tensor_resized(dst, (0, 8), hip_stream=stream.cuda_stream)
    # too small by one element; an f16 destination at an odd address
    with Raises("dst_bytes"):
        dec.pack_tensor_resized((dst.data_ptr(), 3 * 9 * 11 * 2 - 2), (11, 9), hip_stream=stream.cuda_stream)
    with Raises("aligned"):
        dec.pack_tensor_resized((dst.data_ptr() + 1, 4096), (11, 9), hip_stream=stream.cuda_stream)
    with Raises(""):
        dec.pack_tensor_resized((0, 4096), (11, 9), hip_stream=stream.cuda_stream)
    dec.pack_tensor_resized((dst.data_ptr(), 3 * 9 * 11 * 2), (11, 9), hip_stream=stream.cuda_stream)   # exactly enough
    stream.synchronize()


_decoded = {}


def _edge_decoder(frame):
    """The decoder that holds numeric_edges' frame, decoded once for all the sets."""
    if frame not in _decoded:
        jpeg, rgba = ne.FRAMES[frame]()
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        _decoded[frame] = (dec, rgba)
    return _decoded[frame]


def _edge_pack(name, dtype, frame, k, size, filter, order, crop=None):
    """One resized pack of a set of tests/numeric_edges.py, every element against the formula; the device tensor."""
    _, scale, bias = ne.SETS[name]
    dec, rgba = _edge_decoder(frame)
    dst = torch.empty((3, size[1], size[0]), dtype=_torch_type(dtype), device="cuda")
    dec.pack_tensor_resized(dst, size, crop=crop, filter=filter, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                            hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(_host(dst, dtype), ne.expected_resized(rgba, size, k, name, dtype, order, filter, crop), dtype,
           f"{name} {frame} k={k} crop {crop} -> {size} {dtype} {filter} {order}")
    return dst


def numeric_edges(name):
    """One (scale, bias) set of tests/numeric_edges.py on the device's own conversions and arithmetic: nearest at the
    ramp's identity extent (which is pack_tensor of the set, infinities included), bilinear with taps that straddle the
    ramp's tiles; the ImageNet pair as float32, where a contracted tap or lerp shows."""
    dtypes, scale, bias = ne.SETS[name]
    for n, dtype in enumerate(dtypes):
        order = ("rgb", "bgr")[n % 2]
        dec, _ = _edge_decoder("ramp")
        a = torch.empty((3, ne.RAMP_H, ne.RAMP_W), dtype=_torch_type(dtype), device="cuda")
        dec.pack_tensor(a, dtype=dtype, downscale=1, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream)
        b = _edge_pack(name, dtype, "ramp", 1, (ne.RAMP_W, ne.RAMP_H), "nearest", order)
        assert torch.equal(a, b), f"{name} {dtype}: nearest at the identity extent differs from pack_tensor"   # (no NaN: equal means equal)
        frame, k, size, crop = ne.RESIZE_EDGE
        _edge_pack(name, dtype, frame, k, size, "bilinear", ("bgr", "rgb")[n % 2], crop)
    if name == "imagenet_f32":
        for n, (frame, k, size, crop) in enumerate(ne.RESIZE_CONTRACTION):
            _edge_pack(name, "f32", frame, k, size, "bilinear", ("rgb", "bgr")[n % 2], crop)


# (tests/numeric_edges.py's sets by name: importing it here would bring the oracle and the encoder in front of torch)
EDGE_SETS = ("f16_ties", "f16_overflow", "f16_subnormal", "f16_inf", "bf16_ties", "bf16_overflow", "f32_denormal", "f32_inf", "u8_ties",
             "u8_clamp", "u8_clamp2", "imagenet_f32")


def _cases():
    cases = {}
    for w, h in SIZES:
        for k in ADMISSIBLE[(w, h)]:
            cases[f"decoder_every_dtype_and_filter[{w}x{h}-k{k}]"] = (decoder_every_dtype_and_filter, (w, h, k))
    cases["decoder_crops"] = (decoder_crops, ())
    cases["batch_of_five_sizes_inside_sentinels"] = (batch_of_five_sizes_inside_sentinels, ())
    cases["batch_two_packs_back_to_back_with_their_own_crops"] = (batch_two_packs_back_to_back_with_their_own_crops, ())
    cases["texture_that_did_not_shrink"] = (texture_that_did_not_shrink, ())
    cases["other_layouts[420]"] = (other_layouts, (33, 17, (2, 2)))
    cases["other_layouts[444]"] = (other_layouts, (24, 24, (1, 1)))
    cases["wide_row"] = (wide_row, ())
    cases["decoder_ordering_without_host_waits"] = (decoder_ordering_without_host_waits, ())
    cases["batch_ordering_across_streams"] = (batch_ordering_across_streams, ())
    cases["rejections"] = (rejections, ())
    for name in EDGE_SETS:
        cases[f"numeric_edges[{name}]"] = (numeric_edges, (name,))
    return cases


CASES = _cases()


def main(out_path):
    global torch, ca, rr, ne, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import resize_reference as rr
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
