"""The GPU cases of tests/test_gpu_region.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: tests/gpu_antialias_worker.py has the same order).

    python tests/gpu_region_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/region_reference.py), or with what
pack_tensor_resized itself stored.  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

SENTINEL = 0x5C
GREY = (114.0, 114.0, 114.0)
COLOURS = (10.0, 114.0, 250.5)

torch = ca = gr = gpu = stream = None   # set by main(): torch first


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


def _bits(t):
    """A torch tensor's elements as integers: bit for bit is what torch.equal then compares."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _check(got, want, dtype, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert gr.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


def _kw(filter):
    return dict(filter="bilinear", antialias=True) if filter == "antialias" else dict(filter=filter)


_decoders = {}


def _decoder(w, h, sampling=None):
    """The decoder that holds gr.frame(w, h), decoded once for all the cases that pack it."""
    if (w, h, sampling) not in _decoders:
        jpeg, rgba = gr.frame(w, h) if sampling is None else gr.frame(w, h, sampling=sampling)
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg, allow_sampling=True) if sampling else ca.ImageData(jpeg))
        _decoders[(w, h, sampling)] = (dec, rgba)
    return _decoders[(w, h, sampling)]


_batch = None


def _five():
    global _batch
    if _batch is None:
        frames = [gr.frame(w, h, seed=20 + i) for i, (w, h) in enumerate(gr.FIVE)]
        batch = ca.Batch(gpu)
        batch.upload([ca.ImageData(j) for j, _ in frames])
        batch.decode()
        _batch = (frames, batch)
    return _batch


def _pack_and_check(dec, rgba, size, regions, k, dtype, order, filter, what, pad=COLOURS, params=None):
    """One decoder pack of `regions`, sentinel-filled first (an element that no lane writes shows), against the reference."""
    scale, bias = params or gr.params(dtype)
    dst = torch.full((len(regions), 3, size[1], size[0]), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")
    torch.cuda.synchronize()
    dec.pack_tensor_regions(dst, size, regions, pad=pad, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream,
                            **_kw(filter))
    stream.synchronize()
    got = _host(dst, dtype)
    for r, (_, src, rect) in enumerate(regions):
        _check(got[r], gr.expected(rgba, size, k, dtype, scale, bias, order, filter, src, rect, pad), dtype, f"{what}, region {r}")


def dst_whole_is_pack_tensor_resized(filter):
    """dst the whole output -- as zeros and named --, every element type: what pack_tensor_resized itself stores, bit for bit."""
    dec, _ = _decoder(330, 70)
    n = 0
    for dtype in gr.DTYPES:
        scale, bias = gr.params(dtype)
        for size in ((31, 13), (64, 64), (24, 20)):
            n += 1
            k = 2 if size == (24, 20) else 1
            order = ("rgb", "bgr")[n % 2]
            crop = (5, 3, 201, 45) if size == (64, 64) else None
            a = torch.zeros((3, size[1], size[0]), dtype=_torch_type(dtype), device="cuda")
            b = torch.ones((2, 3, size[1], size[0]), dtype=_torch_type(dtype), device="cuda")
            torch.cuda.synchronize()
            dec.pack_tensor_resized(a, size, crop=crop, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream,
                                    **_kw(filter))
            dec.pack_tensor_regions(b, size, [(0, crop, None), (0, crop, (0, 0) + size)], pad=GREY, dtype=dtype, downscale=k, scale=scale, bias=bias,
                                    order=order, hip_stream=stream.cuda_stream, **_kw(filter))
            stream.synchronize()
            assert torch.equal(_bits(a), _bits(b[0])) and torch.equal(_bits(a), _bits(b[1])), f"{filter} {dtype} -> {size} k={k}: differs from pack_tensor_resized"


def letterbox():
    """330x70 fitted into 48x40 (region_fit: rows 15 .. 24), grey 114 around it, the ImageNet scale and bias."""
    dec, rgba = _decoder(330, 70)
    dst = ca.region_fit((330, 70), (48, 40))
    assert dst == (0, 15, 48, 10) == gr.fit((330, 70), (48, 40))
    n = 0
    for filter in gr.FILTERS:
        for dtype in gr.DTYPES:
            n += 1
            _pack_and_check(dec, rgba, (48, 40), [(0, None, dst)], 1, dtype, ("rgb", "bgr")[n % 2], filter, f"letterbox {filter} {dtype}", pad=GREY,
                            params=(gr.IMAGENET_SCALE, gr.IMAGENET_BIAS))
    top = ca.region_fit((330, 70), (48, 40), align="top_left")
    _pack_and_check(dec, rgba, (48, 40), [(0, None, top)], 2, "f16", "rgb", "bilinear", "letterbox at the top, k=2", pad=GREY)


def straddling_borders():
    """dst (5, 3, 21, 9) in 33x17: both borders fall inside a run of every element type; a 1x1 dst in the far corner; a dst
    one column wide at a run's last element."""
    dec, rgba = _decoder(330, 70)
    n = 0
    for filter in gr.FILTERS:
        for dtype in gr.DTYPES:
            n += 1
            regions = [(0, None, (5, 3, 21, 9)), (0, (5, 3, 40, 30), (32, 16, 1, 1)), (0, (100, 0, 60, 70), (15, 0, 1, 17))]
            _pack_and_check(dec, rgba, (33, 17), regions, 1, dtype, ("rgb", "bgr")[n % 2], filter, f"borders {filter} {dtype}")


def decoder_crop_list():
    """Six regions of the 330x70 frame, one crop repeated, one of k x k pixels in the far corner, into [6, 3, 20, 24]."""
    dec, rgba = _decoder(330, 70)
    for k in (1, 2, 8):
        crops = [(0, (10, 5, 100, 40), None), (0, (200, 30, 64, 32), None), (0, (10, 5, 100, 40), None), (0, (330 - k, 70 - k, k, k), None),
                 (0, None, gr.fit((330, 70), (24, 20), "top_left")), (0, (129, 30, 9, 24), gr.fit((9, 24), (24, 20)))]
        for n, filter in enumerate(gr.FILTERS):
            _pack_and_check(dec, rgba, (24, 20), crops, k, ("f16", "u8", "f32")[n], "rgb", filter, f"crop list k={k} {filter}")


def batch_gather_inside_sentinels():
    """Seven regions over five images of five sizes, repeated and out of order; the destination lies one element into a
    sentinel-filled allocation."""
    frames, batch = _five()
    size = (24, 20)
    for dtype, k, filter in (("u8", 1, "bilinear"), ("f16", 1, "antialias"), ("f32", 1, "nearest"), ("bf16", 4, "antialias"), ("f16", 2, "bilinear")):
        scale, bias = gr.params(dtype)
        shape, per_slot, _ = ca.region_tensor_shape(16, 8, size, dtype=dtype)
        needed, esize = 7 * per_slot, gr.ELEM_BYTES[dtype]
        buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor_regions((buf.data_ptr() + 64 + esize, needed), size, gr.SEVEN, pad=COLOURS, dtype=dtype, downscale=k, scale=scale, bias=bias,
                                  order="bgr", hip_stream=stream.cuda_stream, **_kw(filter))
        batch.wait()   # (covers the pack)
        raw = buf.cpu().numpy().tobytes()
        lo, hi = 64 + esize, 64 + esize + needed
        assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{dtype}: sentinels overwritten"
        got = gr.from_bytes(raw[lo:hi], dtype, (7,) + shape)
        for r, (image, src, dst) in enumerate(gr.SEVEN):
            _check(got[r], gr.expected(frames[image][1], size, k, dtype, scale, bias, "bgr", filter, src, dst, COLOURS), dtype,
                   f"{dtype} k={k} {filter} region {r}")


def fewer_regions_than_images():
    frames, batch = _five()
    regions = [(3, None, None), (1, (5, 2, 12, 7), (7, 0, 9, 20))]
    for filter in gr.FILTERS:
        dst = torch.zeros((2, 3, 20, 24), dtype=torch.float16, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor_regions(dst, (24, 20), regions, pad=GREY, scale=gr.IMAGENET_SCALE, bias=gr.IMAGENET_BIAS, hip_stream=stream.cuda_stream,
                                  **_kw(filter))
        batch.wait()
        got = dst.cpu().numpy()
        for r, (image, src, rect) in enumerate(regions):
            _check(got[r], gr.expected(frames[image][1], (24, 20), 1, "f16", gr.IMAGENET_SCALE, gr.IMAGENET_BIAS, "rgb", filter, src, rect, GREY), "f16",
                   f"{filter} region {r}")


def record_staging():
    """Two region packs recorded one behind the other with different regions -- so different records and tables -- and no
    host wait in between, then a plain pack_tensor_resized through the same staging: each sees its own."""
    frames, batch = _five()
    size, scale, bias = (24, 20), gr.IMAGENET_SCALE, gr.IMAGENET_BIAS
    first = list(gr.SEVEN)
    second = [(0, (0, 0, 8, 8), (3, 3, 8, 8)), (4, None, (0, 7, 24, 5)), (2, (25, 13, 25, 13), None)]
    crops = [(0, 0, 8, 8), (5, 2, 12, 7), (25, 13, 25, 13), (1, 1, 33, 17), (0, 0, 330, 70)]
    dst = [torch.zeros((n, 3, 20, 24), dtype=torch.float16, device="cuda") for n in (7, 3, 5)]
    torch.cuda.synchronize()
    batch.pack_tensor_regions(dst[0], size, first, pad=GREY, scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
    batch.pack_tensor_regions(dst[1], size, second, pad=COLOURS, scale=scale, bias=bias, hip_stream=stream.cuda_stream, antialias=True)
    batch.pack_tensor_resized(dst[2], size, crops=crops, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.wait()
    for d, regions, pad, what in ((dst[0], first, GREY, "first"), (dst[1], second, COLOURS, "second")):
        got = d.cpu().numpy()
        for r, (image, src, rect) in enumerate(regions):
            _check(got[r], gr.expected(frames[image][1], size, 1, "f16", scale, bias, "rgb", "antialias", src, rect, pad), "f16", f"{what} pack, region {r}")
    got = dst[2].cpu().numpy()
    for i, (_, rgba) in enumerate(frames):
        _check(got[i], gr.inner(rgba, size, 1, "f16", scale, bias, "rgb", "bilinear", crops[i]), "f16", f"plain pack behind them, slot {i}")


def contraction():
    """Antialiased, inner 31x13 of the noisy 330x70 at an offset inside 40x24, f32 with the ImageNet pair, both orders: the
    shape on which a fused accumulate changes elements (tests/test_antialias_api.py)."""
    dec, rgba = _decoder(330, 70)
    for order in ("rgb", "bgr"):
        _pack_and_check(dec, rgba, (40, 24), [(0, None, (6, 7, 31, 13))], 1, "f32", order, "antialias", f"contraction {order}", pad=GREY,
                        params=(gr.IMAGENET_SCALE, gr.IMAGENET_BIAS))


def layout_420():
    dec, rgba = _decoder(33, 17, (2, 2))
    for n, filter in enumerate(gr.FILTERS):
        regions = [(0, None, gr.fit((33, 17), (24, 20))), (0, (16, 8, 17, 9), (1, 2, 11, 5))]
        _pack_and_check(dec, rgba, (24, 20), regions, (1, 2, 1)[n], "f16", "rgb", filter, f"33x17 4:2:0 {filter}")


def pad_edges():
    """Pad values at the u8 ties and clamps, and beyond f16."""
    dec, rgba = _decoder(330, 70)
    for filter in ("bilinear", "antialias"):
        for pad in ((0.5, 1.5, 2.5), (-3.0, 300.0, 254.5)):
            _pack_and_check(dec, rgba, (33, 17), [(0, None, (5, 3, 21, 9))], 1, "u8", "rgb", filter, f"u8 pad {pad} {filter}", pad=pad, params=gr.IDENTITY)
        _pack_and_check(dec, rgba, (33, 17), [(0, None, (5, 3, 21, 9))], 1, "f16", "bgr", filter, f"f16 pad overflow {filter}",
                        pad=(70000.0, -70000.0, 65519.0), params=gr.IDENTITY)
    # pad=None through the binding: NULL, zeros
    dst = torch.ones((1, 3, 17, 33), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.pack_tensor_regions(dst, (33, 17), [(0, None, (5, 3, 21, 9))], pad=None, dtype="f32", scale=(2, 2, 2), bias=(1, 2, 3), hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(dst.cpu().numpy()[0], gr.expected(rgba, (33, 17), 1, "f32", (2, 2, 2), (1, 2, 3), "rgb", "bilinear", None, (5, 3, 21, 9), (0, 0, 0)), "f32", "pad NULL")


def rejections():
    dec, _ = _decoder(330, 70)
    dst = torch.empty(7 * 3 * 64 * 64, dtype=torch.float16, device="cuda")
    s = dict(hip_stream=stream.cuda_stream)
    with Raises("region 1", "antialias", "330x70", "5x3", "downscale"):   # the limit by the inner extent
        dec.pack_tensor_regions(dst, (64, 64), [(0, None, None), (0, None, (8, 8, 5, 3))], antialias=True, **s)
    dec.pack_tensor_regions(dst, (64, 64), [(0, None, None), (0, None, (8, 8, 5, 3))], downscale=2, antialias=True, **s)   # ... and at k = 2 it runs
    dec.pack_tensor_regions(dst, (64, 64), [(0, None, (8, 8, 5, 3))], **s)   # (the limit is the flag's)
    with Raises("region 0", "image 1", "decoder"):
        dec.pack_tensor_regions(dst, (8, 8), [(1, None, None)], **s)
    with Raises("region 2", "reserved"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, None), (0, None, None), ca.Region(0, 1, ca.Rect(0, 0, 0, 0), ca.Rect(0, 0, 0, 0))], **s)
    with Raises("region 1", "crop", "leaves", "330x70"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, None), (0, (300, 0, 31, 5), None)], **s)
    with Raises("region 0", "crop", "side of 0"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, (3, 3, 0, 5), None)], **s)
    with Raises("region 0", "dst", "side of 0"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, (0, 0, 8, 0))], **s)
    with Raises("region 3", "dst 8x8", "leaves", "8x8 output"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, None)] * 3 + [(0, None, (1, 0, 8, 8))], **s)
    with Raises("region 0", "4x3", "downscale factor 4"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, (0, 0, 4, 3), None)], downscale=4, **s)
    with Raises("region count of 0"):
        dec.pack_tensor_regions(dst, (8, 8), [], **s)
    with Raises("pad", "channel 1", "finite"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, None)], pad=(0, float("inf"), 0), **s)
    with Raises("dst_bytes", str(2 * 3 * 9 * 11 * 2)):
        dec.pack_tensor_regions((dst.data_ptr(), 2 * 3 * 9 * 11 * 2 - 2), (11, 9), [(0, None, None)] * 2, **s)
    with Raises("aligned"):
        dec.pack_tensor_regions((dst.data_ptr() + 1, 4096), (8, 8), [(0, None, None)], **s)
    with Raises("filter 2"):
        dec.pack_tensor_regions(dst, (8, 8), [(0, None, None)], filter=2, **s)
    with Raises("output size"):
        dec.pack_tensor_regions(dst, (0, 8), [(0, None, None)], **s)
    # a grid that does not fit: 4096 slots of 65535 x 65535.  In u8 a slot is 1 048 560 workgroups of 256 runs, antialiased
    # (a lane per element) 16 776 705: 4.3e9 and 6.9e10 workgroups against the limit of 2^31 - 1, which 2048 and 128 slots still
    # meet (tests/test_region_emulation.py asks the planner the same).  The destination is given as what it is, far too
    # small: the grid is checked in front of it, so the message is the grid's, and a call that got past that check would
    # be rejected for its dst_bytes -- whatever the library says here, nothing is launched.
    many = [(0, None, None)] * 4096
    for kw in (dict(filter="nearest"), dict(filter="bilinear"), dict(antialias=True)):
        with Raises("grid", "does not fit"):
            dec.pack_tensor_regions(dst, (65535, 65535), many, dtype="u8", **kw, **s)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_regions(dst, (8, 8), [(0, None, None)], **s)
    frames, batch = _five()
    with Raises("region 1", "image 5", "5 images"):
        batch.pack_tensor_regions(dst, (8, 8), [(4, None, None), (5, None, None)], **s)
    with Raises("region 2", "antialias", "330x70", "5x1"):   # only the region of the last image is beyond the limit
        batch.pack_tensor_regions(dst, (5, 1), [(0, None, None), (3, None, None), (4, None, None)], antialias=True, **s)
    with Raises("region 0", "crop", "leaves", "16x8"):
        batch.pack_tensor_regions(dst, (8, 8), [(0, (0, 0, 17, 8), None)], **s)
    for kw in (dict(filter="bilinear"), dict(antialias=True)):
        with Raises("grid", "does not fit"):
            batch.pack_tensor_regions(dst, (65535, 65535), [(r % 5, None, None) for r in range(4096)], dtype="u8", **kw, **s)
    empty = ca.Batch(gpu)
    with Raises("nothing decoded"):
        empty.pack_tensor_regions(dst, (8, 8), [(0, None, None)], **s)
    batch.wait()
    stream.synchronize()


def _cases():
    cases = {}
    for filter in ("nearest", "bilinear", "antialias"):
        cases[f"dst_whole_is_pack_tensor_resized[{filter}]"] = (dst_whole_is_pack_tensor_resized, (filter,))
    cases["letterbox"] = (letterbox, ())
    cases["straddling_borders"] = (straddling_borders, ())
    cases["decoder_crop_list"] = (decoder_crop_list, ())
    cases["batch_gather_inside_sentinels"] = (batch_gather_inside_sentinels, ())
    cases["fewer_regions_than_images"] = (fewer_regions_than_images, ())
    cases["record_staging"] = (record_staging, ())
    cases["contraction"] = (contraction, ())
    cases["layout_420"] = (layout_420, ())
    cases["pad_edges"] = (pad_edges, ())
    cases["rejections"] = (rejections, ())
    return cases


CASES = _cases()


def main(out_path):
    global torch, ca, gr, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import region_reference as gr
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
