"""The GPU cases of tests/test_gpu_orient.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: tests/gpu_filter_worker.py has the same order).

    python tests/gpu_orient_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/orient_reference.py), bit for bit, or with
what pack_tensor_filtered itself stored for (dst', T), put through torch's flip and transpose.  No shape is larger than
330 x 70.  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

from gpu_filter_worker import COLOURS, GREY, SENTINEL, SIX

torch = ca = fr = orf = gpu = stream = None   # set by main(): torch first


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


def _bits(t):
    """A torch tensor's elements as integers: bit for bit is what torch.equal then compares."""
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _want(a, dtype):
    if dtype == "bf16":
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(np.ascontiguousarray(a))


def _check(got, want, dtype, what):
    """torch.equal on the values: -0 and +0 are one (the library is built -fno-signed-zeros), everything else its bits."""
    want = _want(want, dtype)
    got = got.cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert not torch.isnan(got.float()).any(), f"{what}: elements that no lane wrote"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"


def _fresh(n, size, dtype):
    """A destination of NaNs (u8: sentinels): an element that nobody writes shows."""
    return torch.full((n, 3, size[1], size[0]), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")


def _torch_orient(t, o):
    """orient_reference.orient with torch's own transpose and flip."""
    if o >= 5:
        t = t.transpose(-1, -2)
    if o in (2, 3, 6, 7):
        t = t.flip(-1)
    if o in (3, 4, 7, 8):
        t = t.flip(-2)
    return t.contiguous()


_decoder_330 = None


def _decoder():
    """The decoder that holds fr.frame(330, 70), decoded once for all the cases that pack it."""
    global _decoder_330
    if _decoder_330 is None:
        jpeg, rgba = fr.frame(330, 70)
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        _decoder_330 = (dec, rgba, jpeg)
    return _decoder_330


_batch = None


def _five():
    global _batch
    if _batch is None:
        frames = [fr.frame(w, h, seed=20 + i) for i, (w, h) in enumerate(fr.gr.FIVE)]
        batch = ca.Batch(gpu)
        batch.upload([ca.ImageData(j) for j, _ in frames])
        batch.decode()
        _batch = (frames, batch)
    return _batch


def _pack_and_check(obj, rgba_of, size, regions, k, dtype, order, kernel, what, pad=COLOURS, params=None, wait=None):
    """One oriented pack of `regions` = (image, src, dst, o) into a fresh destination, against the reference."""
    scale, bias = params or fr.params(dtype)
    dst = _fresh(len(regions), size, dtype)
    torch.cuda.synchronize()
    obj.pack_tensor_oriented(dst, size, regions, kernel=kernel, pad=pad, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                             hip_stream=stream.cuda_stream)
    (wait or stream.synchronize)()
    for r, (image, src, rect, o) in enumerate(regions):
        _check(dst[r], orf.expected(rgba_of(image), size, k, dtype, scale, bias, order, kernel, src, rect, pad, o), dtype, f"{what}, region {r} (o={o})")
    return dst


def every_orientation():
    """o = 1 .. 8 of the 330x70 frame into the upright (31, 13), bicubic, f16 and f32, rgb and bgr: against the reference, and
    against the card's own filtered pack of (dst', T) put through torch's flip and transpose."""
    dec, rgba, _ = _decoder()
    params = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    for o in orf.ORIENTATIONS:
        for dtype, order in (("f16", "rgb"), ("f32", "bgr"), ("f32", "rgb"), ("f16", "bgr")):
            got = _pack_and_check(dec, lambda i: rgba, (31, 13), [(0, None, None, o)], 1, dtype, order, "bicubic", f"o={o} {dtype} {order}", params=params)
            t = _fresh(1, orf.slot_extent((31, 13), o), dtype)
            torch.cuda.synchronize()
            dec.pack_tensor_filtered(t, orf.slot_extent((31, 13), o), kernel="bicubic", pad=COLOURS, dtype=dtype, scale=params[0], bias=params[1], order=order,
                                     hip_stream=stream.cuda_stream)
            stream.synchronize()
            turned = _torch_orient(t, o)
            assert torch.equal(_bits(got), _bits(turned)), f"o={o} {dtype} {order}: {int((_bits(got) != _bits(turned)).sum())} elements differ from the turned filtered pack"


def orientation_1_is_the_filtered_pack():
    """All four kernels on SIX over the batch of five: bit for bit what pack_tensor_filtered stores."""
    frames, batch = _five()
    for n, kernel in enumerate(fr.KERNELS):
        dtype = fr.DTYPES[n]
        scale, bias = fr.params(dtype)
        a, b = _fresh(6, (24, 20), dtype), _fresh(6, (24, 20), dtype)
        torch.cuda.synchronize()
        batch.pack_tensor_filtered(a, (24, 20), SIX, kernel=kernel, pad=COLOURS, dtype=dtype, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
        batch.pack_tensor_oriented(b, (24, 20), SIX, orientation=1, kernel=kernel, pad=COLOURS, dtype=dtype, scale=scale, bias=bias,
                                   hip_stream=stream.cuda_stream)
        batch.wait()
        assert torch.equal(_bits(a), _bits(b)), f"{kernel} {dtype}: {int((_bits(a) != _bits(b)).sum())} elements differ from the filtered pack"


def eight_on_a_batch_of_five():
    """EIGHT: every orientation once, over five images of five sizes; every element type with bicubic, Lanczos in f32, k = 2 in f16."""
    frames, batch = _five()
    for dtype, k, kernel in (("u8", 1, "bicubic"), ("f16", 1, "bicubic"), ("bf16", 1, "bicubic"), ("f32", 1, "bicubic"), ("f32", 1, "lanczos3"),
                             ("f16", 2, "bicubic")):
        _pack_and_check(batch, lambda i: frames[i][1], orf.SLOT, list(orf.EIGHT), k, dtype, ("rgb", "bgr")[k % 2], kernel, f"EIGHT {dtype} k={k} {kernel}",
                        params=(fr.IMAGENET_SCALE, fr.IMAGENET_BIAS) if dtype != "u8" else None, wait=batch.wait)


def run_edges():
    """o = 5 .. 8: runs of 1, 7, 8, 9 and 13 elements, at every byte alignment (u8, odd ow, the tensor one byte into its
    allocation) and two vectors a run (f32); inner rectangles at dx = 0, 3, 8 that end a band early, pad in front and behind."""
    frames, batch = _five()
    rgba = frames[1][1]   # 17x9
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f32", "f16"):
                size, esize = (ow, 5), fr.ELEM_BYTES[dtype]
                scale, bias = fr.params(dtype)
                needed = 3 * 5 * ow * esize
                buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                batch.pack_tensor_oriented((buf.data_ptr() + 64 + esize, needed), size, [(1, None, None, o)], kernel="bicubic", pad=COLOURS, dtype=dtype,
                                           scale=scale, bias=bias, hip_stream=stream.cuda_stream)
                batch.wait()
                raw = buf.cpu().numpy().tobytes()
                lo, hi = 64 + esize, 64 + esize + needed
                assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"o={o} ow={ow} {dtype}: sentinels overwritten"
                got = fr.from_bytes(raw[lo:hi], dtype, (3, 5, ow))
                want = orf.expected(rgba, size, 1, dtype, scale, bias, "rgb", "bicubic", None, None, COLOURS, o)
                assert fr.same(got, want, dtype), f"o={o} ow={ow} {dtype}: {int((got != want).sum())} of {want.size} elements differ"
        for dx, dw in ((0, 5), (3, 7), (8, 4), (3, 2)):
            for dtype in ("u8", "f32", "bf16"):
                _pack_and_check(batch, lambda i: rgba, (13, 5), [(1, (1, 0, 15, 9), (dx, 1, dw, 3), o)], 1, dtype, "bgr", "triangle",
                                f"o={o} dx={dx} dw={dw} {dtype}", wait=batch.wait)


def portrait_letterbox():
    """The 330x70 frame at o = 6 is 70x330 upright: fitted into 48x40 with grey 114 around it -- and the same dst under every
    other orientation, at the smallest downscale at which its preimage lies within bicubic's tap limit."""
    dec, rgba, _ = _decoder()
    dst = ca.region_fit((70, 330), (48, 40))
    assert dst == (20, 0, 8, 40)
    for n, o in enumerate(orf.ORIENTATIONS):
        _, _, dw, dh = orf.preimage(dst, o, (48, 40))
        k = next(k for k in (1, 2, 4, 8) if fr.axis_ok("bicubic", 330 // k, dw) and fr.axis_ok("bicubic", 70 // k, dh))
        assert k == (2 if o < 5 else 1)
        dtype = fr.DTYPES[n % 4]
        _pack_and_check(dec, lambda i: rgba, (48, 40), [(0, None, dst, o)], k, dtype, ("rgb", "bgr")[n % 2], "bicubic", f"letterbox o={o} {dtype}", pad=GREY,
                        params=(fr.IMAGENET_SCALE, fr.IMAGENET_BIAS) if dtype != "u8" else None)


def more_than_one_workgroup_per_band():
    """o = 6 into (ow, oh) = (11, 257): T is 257 columns wide."""
    dec, rgba, _ = _decoder()
    _pack_and_check(dec, lambda i: rgba, (11, 257), [(0, None, None, 6), (0, (10, 0, 300, 64), (2, 0, 9, 257), 6)], 1, "f16", "rgb", "bicubic", "257 rows of U")
    _pack_and_check(dec, lambda i: rgba, (11, 257), [(0, None, None, 7)], 1, "u8", "bgr", "box", "257 rows of U, u8")


def the_tag():
    """A frame with orientation 6 spliced in behind SOI: ImageData.orientation, "exif" on a decoder, and on a batch through
    upload and through upload_jpegs, mixed with frames that carry no tag."""
    _, rgba, jpeg = _decoder()
    tagged = orf.splice(jpeg, orf.exif_app1(6))
    image = ca.ImageData(tagged)
    assert image.orientation == 6 and ca.ImageData(jpeg).orientation == 1
    dec = ca.Decoder(gpu)
    dec.decode_blocking(image)
    a, b = _fresh(1, (13, 31), "f16"), _fresh(1, (13, 31), "f16")
    torch.cuda.synchronize()
    dec.pack_tensor_oriented(a, (13, 31), orientation="exif", hip_stream=stream.cuda_stream)
    dec.pack_tensor_oriented(b, (13, 31), orientation=6, hip_stream=stream.cuda_stream)
    stream.synchronize()
    assert torch.equal(_bits(a), _bits(b)), "exif differs from 6 on a decoder"
    _check(a[0], orf.expected(rgba, (13, 31), 1, "f16", (1, 1, 1), (0, 0, 0), o=6), "f16", "decoder, exif")
    # a decoder remembers the tag of the image it decoded last
    dec.decode_blocking(ca.ImageData(jpeg))
    dec.pack_tensor_oriented(a, (31, 13), hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(a.view(1, 3, 13, 31)[0], orf.expected(rgba, (31, 13), 1, "f16", (1, 1, 1), (0, 0, 0), o=1), "f16", "decoder, no tag")
    small_jpeg, small = fr.frame(66, 26, seed=23)
    files = [small_jpeg, tagged, orf.splice(small_jpeg, orf.exif_app1(3, little=False, where="last")), jpeg]
    tags, sources = [1, 6, 3, 1], [small, rgba, small, rgba]
    for road in ("upload", "upload_jpegs"):
        batch = ca.Batch(gpu)
        if road == "upload":
            batch.upload([ca.ImageData(f) for f in files])
        else:
            batch.upload_jpegs(files)
        assert [batch.orientation(i) for i in range(4)] == tags, road
        with Raises("image 4", "4 images"):
            batch.orientation(4)
        batch.decode()
        # (a 13 x 13 slot: whole images under either shape of T)
        a, b = _fresh(4, (13, 13), "f32"), _fresh(4, (13, 13), "f32")
        torch.cuda.synchronize()
        batch.pack_tensor_oriented(a, (13, 13), dtype="f32", hip_stream=stream.cuda_stream)   # regions=None, orientation="exif"
        batch.pack_tensor_oriented(b, (13, 13), [(i, None, None, tags[i]) for i in range(4)], dtype="f32", hip_stream=stream.cuda_stream)
        batch.wait()
        assert torch.equal(_bits(a), _bits(b)), f"{road}: exif differs from the explicit orientations"
        for i in range(4):
            _check(a[i], orf.expected(sources[i], (13, 13), 1, "f32", (1, 1, 1), (0, 0, 0), o=tags[i]), "f32", f"{road}, image {i}")


def rejections():
    """Nothing here launches."""
    dec, _, _ = _decoder()
    dst = torch.empty(8 * 3 * 24 * 20, dtype=torch.float16, device="cuda")
    s = dict(hip_stream=stream.cuda_stream)
    with Raises("region 1", "orientation 9"):
        dec.pack_tensor_oriented(dst, (24, 20), [(0, None, None, 1), (0, None, None, 9)], **s)
    bad = ca.OrientedRegion()
    bad.orientation, bad.reserved = 6, 1
    with Raises("region 0", "reserved must be 0"):
        dec.pack_tensor_oriented(dst, (24, 20), [bad], **s)
    # 200 columns into 20 at o = 1; into 6 at o = 6: 200 * 4 > 128 * 6 on T's x axis
    dec.pack_tensor_oriented(dst, (24, 20), [(0, (101, 3, 200, 64), (2, 4, 20, 6), 1)], **s)
    with Raises("region 0", "bicubic", "200x64", "6x20", "orientation 6 transposes"):
        dec.pack_tensor_oriented(dst, (24, 20), [(0, (101, 3, 200, 64), (2, 4, 20, 6), 6)], **s)
    with Raises("region 0", "dst 20x24", "leaves", "24x20 output"):
        dec.pack_tensor_oriented(dst, (24, 20), [(0, None, (0, 0, 20, 24), 5)], **s)
    with Raises("region 0", "image 1", "decoder"):
        dec.pack_tensor_oriented(dst, (24, 20), [(1, None, None, 6)], **s)
    with Raises("dst_bytes"):
        dec.pack_tensor_oriented((dst.data_ptr(), 3 * 24 * 20 * 2 - 2), (24, 20), orientation=8, **s)
    with Raises("grid", "does not fit"):   # (in front of the destination and the list: nothing is allocated, nothing launched)
        dec.pack_tensor_oriented(dst, (65535, 65535), [(0, None, None, 6)] * 4096, dtype="u8", **s)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_oriented(dst, (24, 20), **s)
    frames, batch = _five()
    with Raises("region 1", "image 5", "5 images"):
        batch.pack_tensor_oriented(dst, (24, 20), [(4, None, None, 2), (5, None, None, 2)], **s)
    batch.wait()
    stream.synchronize()


def back_to_back():
    """Two oriented packs with different lists and a filtered pack behind them, recorded on one stream without a wait: each
    sees its own records and tables."""
    frames, batch = _five()
    size, scale, bias = orf.SLOT, fr.IMAGENET_SCALE, fr.IMAGENET_BIAS
    first = list(orf.EIGHT)
    second = [(0, (0, 0, 8, 8), (3, 3, 8, 8), 7), (4, None, (0, 7, 24, 5), 2), (2, (25, 13, 25, 13), None, 5)]
    dst = [_fresh(n, size, "f16") for n in (8, 3, 6)]
    torch.cuda.synchronize()
    batch.pack_tensor_oriented(dst[0], size, first, kernel="bicubic", pad=GREY, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_oriented(dst[1], size, second, kernel="lanczos3", pad=COLOURS, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_filtered(dst[2], size, SIX, kernel="triangle", pad=GREY, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.wait()
    for d, regions, pad, kernel, what in ((dst[0], first, GREY, "bicubic", "first"), (dst[1], second, COLOURS, "lanczos3", "second")):
        for r, (image, src, rect, o) in enumerate(regions):
            _check(d[r], orf.expected(frames[image][1], size, 1, "f16", scale, bias, "rgb", kernel, src, rect, pad, o), "f16", f"{what} pack, region {r}")
    for r, (image, src, rect) in enumerate(SIX):
        _check(dst[2][r], fr.expected(frames[image][1], size, 1, "f16", scale, bias, "rgb", "triangle", src, rect, GREY), "f16", f"filtered pack behind them, region {r}")


# two slots of (13, 5) out of a 17x9 frame, FIVE's smallest with a picture in it (synth's 16x8 is black, as fresh memory may be)
ACROSS = ((0, None, None, 6), (0, (1, 0, 15, 8), (2, 1, 9, 3), 3))


def _check_across(dst, rgba, what):
    for r, (_, src, rect, o) in enumerate(ACROSS):
        _check(dst[r], orf.expected(rgba, (13, 5), 1, "f32", (1, 1, 1), (0, 0, 0), "rgb", "bicubic", src, rect, COLOURS, o), "f32", f"{what}, region {r}")


def decoder_ordering_without_host_waits():
    """enqueue(img1, A), pack(dst1, B), enqueue(img2, A), pack(dst2, B) on a new decoder, two 17x9 frames: every pack behind
    its decode, the second decode behind the first pack, with nothing but the streams' own order and the library's events."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    (j1, r1), (j2, r2) = fr.frame(17, 9, seed=21), fr.frame(17, 9, seed=31)
    img1, img2 = ca.ImageData(j1), ca.ImageData(j2)
    dst1, dst2 = _fresh(2, (13, 5), "f32"), _fresh(2, (13, 5), "f32")
    torch.cuda.synchronize()
    dec = ca.Decoder(gpu)
    dec.enqueue(img1, a.cuda_stream)
    dec.pack_tensor_oriented(dst1, (13, 5), ACROSS, pad=COLOURS, dtype="f32", hip_stream=b.cuda_stream)
    dec.enqueue(img2, a.cuda_stream)
    dec.pack_tensor_oriented(dst2, (13, 5), ACROSS, pad=COLOURS, dtype="f32", hip_stream=b.cuda_stream)
    a.synchronize()
    b.synchronize()
    _check_across(dst1, r1, "first frame")
    _check_across(dst2, r2, "second frame")


def batch_ordering_without_host_waits():
    """The same on a new batch of one 17x9 frame: decode(A), pack(dst1, B), decode(A), pack(dst2, B) and one wait().  The
    first pack stands behind the first decode -- the batch's output holds nothing before it --, the second decode behind
    the first pack, the second pack behind the second decode."""
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    jpeg, rgba = fr.frame(17, 9, seed=21)
    dst1, dst2 = _fresh(2, (13, 5), "f32"), _fresh(2, (13, 5), "f32")
    torch.cuda.synchronize()
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(jpeg)])
    batch.decode(hip_stream=a.cuda_stream)
    batch.pack_tensor_oriented(dst1, (13, 5), ACROSS, pad=COLOURS, dtype="f32", hip_stream=b.cuda_stream)
    batch.decode(hip_stream=a.cuda_stream)
    batch.pack_tensor_oriented(dst2, (13, 5), ACROSS, pad=COLOURS, dtype="f32", hip_stream=b.cuda_stream)
    batch.wait()
    a.synchronize()
    _check_across(dst1, rgba, "first pack")
    _check_across(dst2, rgba, "second pack")


CASES = {fn.__name__: (fn, ()) for fn in (every_orientation, orientation_1_is_the_filtered_pack, eight_on_a_batch_of_five, run_edges, portrait_letterbox,
                                          more_than_one_workgroup_per_band, the_tag, rejections, back_to_back,
                                          decoder_ordering_without_host_waits, batch_ordering_without_host_waits)}


def main(out_path):
    global torch, ca, fr, orf, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import orient_reference as orf
    fr = orf.fr
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
        except AssertionError:
            results[name] = traceback.format_exc()
        except Exception:   # (torch's own errors come from the device as well)
            results[name] = traceback.format_exc()
            device_said_no = True
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
        if device_said_no:   # nothing more is started on it
            break
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
