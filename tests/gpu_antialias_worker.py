"""The GPU cases of tests/test_gpu_antialias.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: tests/gpu_resize_worker.py has the same order).

    python tests/gpu_antialias_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/antialias_reference.py).  RESULTS.json: case
name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

FIVE = ((16, 8), (17, 9), (50, 26), (66, 26), (330, 70))
SENTINEL = 0x5C
# (w, h, k, (ow, oh)): together they take every element type and both orders (see _cases)
SHAPES = ((330, 70, 1, (31, 13)), (330, 70, 2, (31, 13)), (50, 26, 1, (5, 3)), (17, 9, 1, (16, 8)), (50, 26, 1, (1, 1)), (330, 70, 1, (224, 224)))
CONTRACTION = (330, 70, 1, (31, 13))   # tests/test_antialias_api.py: a fused accumulate changes elements here

torch = ca = ar = rr = gpu = stream = None   # set by main(): torch first


class Raises:
    """with Raises("words", ...): the library's INVALID_ARG whose message has the words."""

    def __init__(self, *words):
        self.words = words

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        assert kind is not None and issubclass(kind, ca.Error), "no error raised"
        assert value.code == ca.E_INVALID_ARG and str(value) and all(w in str(value) for w in self.words), (value.code, str(value))
        return True


def _torch_type(dtype):
    return {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[dtype]


def _host(t, dtype):
    """A torch tensor's elements as the reference compares them (bf16: the bit patterns)."""
    if dtype == "bf16":
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _check(got, want, dtype, what):
    assert ar.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


_decoders = {}


def _decoder(w, h, sampling=None):
    """The decoder that holds rr.frame(w, h), decoded once for all the cases that pack it."""
    if (w, h, sampling) not in _decoders:
        jpeg, rgba = rr.frame(w, h) if sampling is None else rr.frame(w, h, sampling=sampling)
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg, allow_sampling=True) if sampling else ca.ImageData(jpeg))
        _decoders[(w, h, sampling)] = (dec, rgba)
    return _decoders[(w, h, sampling)]


def _pack_and_check(dec, rgba, size, k, dtype, order, what, crop=None, params=None):
    h, w = rgba.shape[:2]
    scale, bias = params or rr.params(dtype)
    shape, nbytes, pre = ca.resized_tensor_shape(w, h, size, dtype=dtype, downscale=k, crop=crop, antialias=True)
    assert shape == (3, size[1], size[0]) and pre == rr.pre_extent(w, h, k, crop)[::-1]
    dst = torch.empty(shape, dtype=_torch_type(dtype), device="cuda")
    assert dst.numel() * dst.element_size() == nbytes
    dec.pack_tensor_resized(dst, size, crop=crop, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream,
                            antialias=True)
    stream.synchronize()
    _check(_host(dst, dtype), ar.expected(rgba, size, k, dtype, scale, bias, order, crop), dtype, what)


def shape(w, h, k, size, n):
    """One shape, every element type, the orders in rotation."""
    dec, rgba = _decoder(w, h)
    for d, dtype in enumerate(rr.DTYPES):
        _pack_and_check(dec, rgba, size, k, dtype, ("rgb", "bgr")[(n + d) % 2], f"{w}x{h} k={k} -> {size} {dtype}")


def growing_is_plain_bilinear():
    """17x9 -> 64x64, neither axis shrinks: the flag changes no element of the plain bilinear pack."""
    dec, rgba = _decoder(17, 9)
    for dtype in rr.DTYPES:
        scale, bias = rr.params(dtype)
        a = torch.empty((3, 64, 64), dtype=_torch_type(dtype), device="cuda")
        b = torch.empty((3, 64, 64), dtype=_torch_type(dtype), device="cuda")
        dec.pack_tensor_resized(a, (64, 64), dtype=dtype, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
        dec.pack_tensor_resized(b, (64, 64), dtype=dtype, scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
        stream.synchronize()
        assert torch.equal(a, b), f"{dtype}: differs from the plain bilinear pack"
        _check(_host(b, dtype), ar.expected(rgba, (64, 64), 1, dtype, scale, bias), dtype, f"17x9 -> 64x64 {dtype}")


def identity_extent_is_pack_tensor():
    dec, _ = _decoder(330, 70)
    for k in (1, 2, 8):
        pw, ph = rr.pre_extent(330, 70, k)
        for dtype in ("f32", "u8"):
            scale, bias = rr.params(dtype)
            a = torch.empty((3, ph, pw), dtype=_torch_type(dtype), device="cuda")
            b = torch.empty((3, ph, pw), dtype=_torch_type(dtype), device="cuda")
            dec.pack_tensor(a, dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
            dec.pack_tensor_resized(b, (pw, ph), dtype=dtype, downscale=k, scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
            stream.synchronize()
            assert torch.equal(a, b), f"k={k} {dtype}: the identity extent differs from pack_tensor"


def decoder_crops():
    """330x70, u8 with a scale and bias that round and clamp."""
    dec, rgba = _decoder(330, 70)
    for k in (1, 2, 8):
        crops = [None, (330 - 97, 70 - 33, 97, 33), (5, 3, 201, 45), (330 - k, 70 - k, k, k)]
        if k == 1:
            crops.append((129, 30, 1, 1))
        for n, crop in enumerate(crops):
            for size in ((17, 9), (64, 64)):
                _pack_and_check(dec, rgba, size, k, "u8", ("rgb", "bgr")[n % 2], f"crop {crop} k={k} -> {size}", crop=crop)


def _five():
    frames = [rr.frame(w, h, seed=20 + i) for i, (w, h) in enumerate(FIVE)]
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode()
    return frames, batch


def batch_of_five_sizes_inside_sentinels():
    """The destination lies one element into a sentinel-filled allocation.  16x8 and 17x9 grow to 24x20, 50x26 and 66x26
    shrink one way or both, 330x70 shrinks both ways: five pairs of tables in one launch."""
    frames, batch = _five()
    size = (24, 20)
    for dtype, k in (("u8", 1), ("f16", 1), ("f32", 1), ("bf16", 2)):
        scale, bias = rr.params(dtype)
        shape, per_image, _ = ca.resized_tensor_shape(16, 8, size, dtype=dtype, downscale=k, antialias=True)
        needed, esize = 5 * per_image, rr.ELEM_BYTES[dtype]
        buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor_resized((buf.data_ptr() + 64 + esize, needed), size, dtype=dtype, downscale=k, scale=scale, bias=bias,
                                  hip_stream=stream.cuda_stream, antialias=True)
        batch.wait()   # (covers the pack)
        raw = buf.cpu().numpy().tobytes()
        lo, hi = 64 + esize, 64 + esize + needed
        assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{dtype}: sentinels overwritten"
        got = rr.from_bytes(raw[lo:hi], dtype, (5,) + shape)
        for i, (_, rgba) in enumerate(frames):
            _check(got[i], ar.expected(rgba, size, k, dtype, scale, bias), dtype, f"{dtype} k={k} slot {i}")


def batch_two_packs_back_to_back_with_their_own_crops():
    """Two packs recorded one behind the other with different crops -- so different tables -- and no host wait in between,
    then a plain bilinear one through the same staging: each sees its own records and tables."""
    frames, batch = _five()
    size, scale, bias = (24, 20), rr.IMAGENET_SCALE, rr.IMAGENET_BIAS
    first = [(1, 1, 15, 7), (0, 0, 17, 9), (3, 1, 45, 21), (2, 0, 64, 26), (101, 3, 200, 64)]
    second = [(0, 0, 8, 8), (5, 2, 12, 7), (25, 13, 25, 13), (1, 1, 33, 17), (0, 0, 330, 70)]
    dst = [torch.zeros((5, 3, 20, 24), dtype=torch.float16, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    batch.pack_tensor_resized(dst[0], size, crops=first, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
    batch.pack_tensor_resized(dst[1], size, crops=second, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
    batch.pack_tensor_resized(dst[2], size, crops=second, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.wait()
    for d, crops, what in ((dst[0], first, "first"), (dst[1], second, "second")):
        got = d.cpu().numpy()
        for i, (_, rgba) in enumerate(frames):
            _check(got[i], ar.expected(rgba, size, 1, "f16", scale, bias, crop=crops[i]), "f16", f"{what} pack, slot {i}")
    got = dst[2].cpu().numpy()
    for i, (_, rgba) in enumerate(frames):
        _check(got[i], rr.expected(rgba, size, 1, "f16", scale, bias, crop=second[i]), "f16", f"plain pack behind them, slot {i}")


def wide_row():
    """65528 x 8, k = 8: a prefiltered row of 8191 elements shrinks to 4000, its one row stays one row."""
    dec, rgba = _decoder(65528, 8)
    _pack_and_check(dec, rgba, (4000, 1), 8, "f16", "rgb", "65528x8 k=8 -> 4000x1")


def contraction():
    """The f32 shape on which a fused accumulate changes elements (tests/test_antialias_api.py)."""
    w, h, k, size = CONTRACTION
    dec, rgba = _decoder(w, h)
    for order in ("rgb", "bgr"):
        _pack_and_check(dec, rgba, size, k, "f32", order, f"{w}x{h} -> {size} f32 {order}", params=(rr.IMAGENET_SCALE, rr.IMAGENET_BIAS))


def layout_420():
    dec, rgba = _decoder(33, 17, (2, 2))
    for k, size in ((1, (24, 20)), (1, (11, 5)), (2, (7, 3))):
        _pack_and_check(dec, rgba, size, k, "f16", "rgb", f"33x17 4:2:0 k={k} -> {size}")


def rejections():
    dec, _ = _decoder(330, 70)
    dst = torch.empty(3 * 64 * 64, dtype=torch.float16, device="cuda")
    with Raises("antialias", "330x70", "5x3", "downscale"):
        dec.pack_tensor_resized(dst, (5, 3), hip_stream=stream.cuda_stream, antialias=True)
    dec.pack_tensor_resized(dst, (5, 3), downscale=2, hip_stream=stream.cuda_stream, antialias=True)   # ... and at k = 2 it runs
    with Raises("antialias"):
        dec.pack_tensor_resized(dst, (8, 8), filter="nearest", hip_stream=stream.cuda_stream, antialias=True)
    with Raises("filter 513"):
        dec.pack_tensor_resized(dst, (8, 8), filter=0x201, hip_stream=stream.cuda_stream)
    with Raises("filter 2"):
        dec.pack_tensor_resized(dst, (8, 8), filter=2, hip_stream=stream.cuda_stream, antialias=True)
    with Raises("crop"):
        dec.pack_tensor_resized(dst, (8, 8), crop=(300, 0, 31, 5), hip_stream=stream.cuda_stream, antialias=True)
    with Raises("dst_bytes"):
        dec.pack_tensor_resized((dst.data_ptr(), 3 * 9 * 11 * 2 - 2), (11, 9), hip_stream=stream.cuda_stream, antialias=True)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_resized(dst, (8, 8), hip_stream=stream.cuda_stream, antialias=True)
    frames, batch = _five()
    with Raises("image 4", "antialias", "330x70", "5x1"):   # only the last image is beyond the limit
        batch.pack_tensor_resized(dst, (5, 1), hip_stream=stream.cuda_stream, antialias=True)
    batch.wait()
    stream.synchronize()


def _cases():
    cases = {}
    for n, (w, h, k, size) in enumerate(SHAPES):
        cases[f"shape[{w}x{h}-k{k}-to{size[0]}x{size[1]}]"] = (shape, (w, h, k, size, n))
    cases["growing_is_plain_bilinear"] = (growing_is_plain_bilinear, ())
    cases["identity_extent_is_pack_tensor"] = (identity_extent_is_pack_tensor, ())
    cases["decoder_crops"] = (decoder_crops, ())
    cases["batch_of_five_sizes_inside_sentinels"] = (batch_of_five_sizes_inside_sentinels, ())
    cases["batch_two_packs_back_to_back_with_their_own_crops"] = (batch_two_packs_back_to_back_with_their_own_crops, ())
    cases["wide_row"] = (wide_row, ())
    cases["contraction"] = (contraction, ())
    cases["layout_420"] = (layout_420, ())
    cases["rejections"] = (rejections, ())
    return cases


CASES = _cases()


def main(out_path):
    global torch, ca, ar, rr, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import antialias_reference as ar
    import resize_reference as rr
    gpu = ca.Gpu.open(0)
    stream = torch.cuda.Stream()
    results, device_said_no = {}, False
    for name, (fn, args) in CASES.items():
        try:
            fn(*args)
            results[name] = None
        except ca.Error as e:
            results[name] = f"compeg_amd.Error {e.code}: {e}\n{traceback.format_exc()}"
            device_said_no = e.code == ca.E_HIP
        except Exception:
            results[name] = traceback.format_exc()
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
        if device_said_no:   # nothing more is started on it
            break
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
