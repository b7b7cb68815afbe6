"""The GPU cases of tests/test_gpu_nhwc.py, run in one process of their own that imports torch before the library (both
bring a HIP runtime and the one loaded first serves both: tests/gpu_orient_worker.py has the same order).

    python tests/gpu_nhwc_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/nhwc_reference.py), bit for bit, or with what
pack_tensor_oriented itself stored for the same arguments, permuted by torch.  No shape is larger than 330 x 70.
RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

from gpu_filter_worker import COLOURS, GREY, SENTINEL
from gpu_orient_worker import Raises, _bits, _torch_type, _want

torch = ca = fr = orf = nr = gpu = stream = None   # set by main(): torch first
FILL = {"u8": 127.5, "f16": 0.1, "bf16": 0.1, "f32": 0.1}   # a tie in u8 (128); rounds in f16 and bf16


def _check(got, want, dtype, what):
    """torch.equal on the values: -0 and +0 are one (the library is built -fno-signed-zeros), everything else its bits."""
    want = _want(want, dtype)
    got = got.cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert not torch.isnan(got.float()).any(), f"{what}: elements that no lane wrote"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"


def _fresh(n, size, dtype, channels):
    """A channels-last destination [n, oh, ow, C] of NaNs (u8: sentinels): an element that nobody writes shows."""
    return torch.full((n, size[1], size[0], channels), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")


def _fresh_planar(n, size, dtype):
    return torch.full((n, 3, size[1], size[0]), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")


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


def _pack_and_check(obj, rgba_of, size, regions, k, dtype, order, kernel, channels, what, pad=COLOURS, params=None, wait=None, fill=None):
    """One channels-last pack of `regions` = (image, src, dst, o) into a fresh destination, against the reference."""
    scale, bias = params or fr.params(dtype)
    fill = FILL[dtype] if fill is None else fill
    dst = _fresh(len(regions), size, dtype, channels)
    torch.cuda.synchronize()
    obj.pack_tensor_nhwc(dst, size, regions, channels=channels, fill=fill, kernel=kernel, pad=pad, dtype=dtype, downscale=k, scale=scale, bias=bias,
                         order=order, hip_stream=stream.cuda_stream)
    (wait or stream.synchronize)()
    for r, (image, src, rect, o) in enumerate(regions):
        want = nr.expected(rgba_of(image), size, k, dtype, scale, bias, order, kernel, src, rect, pad, o, channels, fill)
        _check(dst[r], want, dtype, f"{what}, region {r} (o={o}, C={channels})")
    return dst


def letterbox_every_orientation_type_and_channel_count():
    """The 330x70 frame into the 48x40 letterbox (20, 0, 8, 40): o = 1 .. 8 x element type x C, at the smallest downscale at
    which the preimage lies within bicubic's tap limit."""
    dec, rgba, _ = _decoder()
    dst = ca.region_fit((70, 330), (48, 40))
    assert dst == (20, 0, 8, 40)
    n = 0
    for o in orf.ORIENTATIONS:
        _, _, dw, dh = orf.preimage(dst, o, (48, 40))
        k = next(k for k in (1, 2, 4, 8) if fr.axis_ok("bicubic", 330 // k, dw) and fr.axis_ok("bicubic", 70 // k, dh))
        for dtype in fr.DTYPES:
            for channels in nr.CHANNELS:
                n += 1
                _pack_and_check(dec, lambda i: rgba, (48, 40), [(0, None, dst, o)], k, dtype, ("rgb", "bgr")[n // 2 % 2], "bicubic", channels,
                                f"letterbox o={o} {dtype}", pad=GREY if n % 3 else COLOURS,
                                params=(fr.IMAGENET_SCALE, fr.IMAGENET_BIAS) if dtype != "u8" and n % 2 else None)


def run_edges():
    """o = 5 .. 8: runs of 1, 7, 8, 9 and 13 pixels of 3 and 4 elements, the tensor one element into its allocation so that
    the pieces are misaligned; the sentinels on both sides survive."""
    frames, batch = _five()
    rgba = frames[1][1]   # 17x9
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f16", "f32"):
                for channels in nr.CHANNELS:
                    size, esize = (ow, 5), fr.ELEM_BYTES[dtype]
                    scale, bias = fr.params(dtype)
                    needed = 5 * ow * channels * esize
                    buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    batch.pack_tensor_nhwc((buf.data_ptr() + 64 + esize, needed), size, [(1, None, None, o)], channels=channels, fill=FILL[dtype],
                                           kernel="bicubic", pad=COLOURS, dtype=dtype, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
                    batch.wait()
                    raw = buf.cpu().numpy().tobytes()
                    lo, hi = 64 + esize, 64 + esize + needed
                    what = f"o={o} ow={ow} {dtype} C={channels}"
                    assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{what}: sentinels overwritten"
                    got = fr.from_bytes(raw[lo:hi], dtype, (5, ow, channels))
                    want = nr.expected(rgba, size, 1, dtype, scale, bias, "rgb", "bicubic", None, None, COLOURS, o, channels, FILL[dtype])
                    assert fr.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


def eight_on_a_batch_of_five():
    """EIGHT's mixed orientations over five images of five sizes, every kernel, k = 1 and 2, the ImageNet pair, BGR for half:
    against the reference, and against the card's own pack_tensor_oriented for the same arguments, permuted to NHWC."""
    frames, batch = _five()
    params = (fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)
    n = 0
    for kernel in fr.KERNELS:
        for k in (1, 2):
            dtype, order, channels = ("f16", "f32", "bf16", "f16")[n % 4], ("rgb", "bgr")[n % 2], nr.CHANNELS[n // 2 % 2]
            n += 1
            use = params
            got = _pack_and_check(batch, lambda i: frames[i][1], orf.SLOT, list(orf.EIGHT), k, dtype, order, kernel, channels,
                                  f"EIGHT {kernel} k={k} {dtype} {order}", params=use, wait=batch.wait)
            planar = _fresh_planar(8, orf.SLOT, dtype)
            torch.cuda.synchronize()
            batch.pack_tensor_oriented(planar, orf.SLOT, list(orf.EIGHT), kernel=kernel, pad=COLOURS, dtype=dtype, downscale=k, scale=use[0], bias=use[1],
                                       order=order, hip_stream=stream.cuda_stream)
            batch.wait()
            a, b = _bits(got[..., :3]), _bits(planar.permute(0, 2, 3, 1))
            assert torch.equal(a, b), f"EIGHT {kernel} k={k} {dtype} {order}: {int((a != b).sum())} elements differ from the oriented pack, permuted"


def a_channels_last_torch_tensor_as_it_is():
    """torch.empty(N, 3, oh, ow).contiguous(memory_format=torch.channels_last) handed over: read as NCHW afterwards it is the
    oriented pack's output.  A planar tensor is refused before anything is launched."""
    frames, batch = _five()
    regions, (ow, oh) = list(orf.EIGHT), orf.SLOT
    dst = torch.full((8, 3, oh, ow), float("nan"), dtype=torch.float16, device="cuda").contiguous(memory_format=torch.channels_last)
    assert not dst.is_contiguous() and dst.stride() == (oh * ow * 3, 1, ow * 3, 3)
    planar = _fresh_planar(8, orf.SLOT, "f16")
    torch.cuda.synchronize()
    batch.pack_tensor_nhwc(dst, orf.SLOT, regions, pad=GREY, scale=fr.IMAGENET_SCALE, bias=fr.IMAGENET_BIAS, hip_stream=stream.cuda_stream)
    batch.pack_tensor_oriented(planar, orf.SLOT, regions, pad=GREY, scale=fr.IMAGENET_SCALE, bias=fr.IMAGENET_BIAS, hip_stream=stream.cuda_stream)
    batch.wait()
    assert not torch.isnan(dst.float()).any(), "elements that no lane wrote"
    assert dst.shape == planar.shape and torch.equal(_bits(dst), _bits(planar)), "read as NCHW, the tensor differs from the oriented pack"
    assert dst.is_contiguous(memory_format=torch.channels_last)
    with Raises("planar"):
        batch.pack_tensor_nhwc(planar, orf.SLOT, regions, hip_stream=stream.cuda_stream)
    batch.wait()


def four_u8_channels_with_255_and_more_than_one_workgroup_per_band():
    """C = 4, u8, fill = 255 into a slot of 257 columns: element 3 is 255 in every pixel, the pad's included; the three
    others are the C = 3 pack.  o = 3 keeps T 257 columns wide, o = 6 gives U's rows runs along them."""
    dec, rgba, _ = _decoder()
    scale, bias = fr.params("u8")
    for size, regions in (((257, 11), [(0, None, (0, 2, 257, 9), 3), (0, None, None, 2)]), ((11, 257), [(0, None, (2, 0, 9, 257), 6)])):
        four = _pack_and_check(dec, lambda i: rgba, size, regions, 1, "u8", "rgb", "bicubic", 4, f"257 columns {size}", pad=GREY, fill=255.0)
        three = _pack_and_check(dec, lambda i: rgba, size, regions, 1, "u8", "rgb", "bicubic", 3, f"257 columns {size}", pad=GREY)
        assert bool((four[..., 3] == 255).all()), "element 3 is not 255 everywhere"
        assert torch.equal(four[..., :3], three), "RGB differs between C = 4 and C = 3"


def two_packs_behind_a_decode_and_a_decode_behind_them():
    """On one stream without a wait in between: a decode, two channels-last packs with different lists and layouts, and the
    decode again; one wait() covers them all.  Each pack saw its own records and tables and the decoded pixels; a pack
    behind the second decode sees them too."""
    frames = [fr.frame(w, h, seed=20 + i) for i, (w, h) in enumerate(fr.gr.FIVE)]
    batch = ca.Batch(gpu)
    size, scale, bias = orf.SLOT, fr.IMAGENET_SCALE, fr.IMAGENET_BIAS
    first = list(orf.EIGHT)
    second = [(0, (0, 0, 8, 8), (3, 3, 8, 8), 7), (4, None, (0, 7, 24, 5), 2), (2, (25, 13, 25, 13), None, 5)]
    dst = [_fresh(8, size, "f16", 3), _fresh(3, size, "f16", 4), _fresh(3, size, "f16", 4)]
    torch.cuda.synchronize()
    batch.upload([ca.ImageData(j) for j, _ in frames])
    batch.decode(hip_stream=stream.cuda_stream)
    batch.pack_tensor_nhwc(dst[0], size, first, channels=3, kernel="bicubic", pad=GREY, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_nhwc(dst[1], size, second, channels=4, fill=1.0, kernel="lanczos3", pad=COLOURS, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.decode(hip_stream=stream.cuda_stream)
    batch.wait()
    batch.pack_tensor_nhwc(dst[2], size, second, channels=4, fill=1.0, kernel="lanczos3", pad=COLOURS, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.wait()
    for d, regions, pad, kernel, channels, what in ((dst[0], first, GREY, "bicubic", 3, "first"), (dst[1], second, COLOURS, "lanczos3", 4, "second"),
                                                    (dst[2], second, COLOURS, "lanczos3", 4, "behind the second decode")):
        for r, (image, src, rect, o) in enumerate(regions):
            want = nr.expected(frames[image][1], size, 1, "f16", scale, bias, "rgb", kernel, src, rect, pad, o, channels, 1.0)
            _check(d[r], want, "f16", f"{what} pack, region {r}")


def rejections():
    """Nothing here launches."""
    dec, _, _ = _decoder()
    dst = torch.empty(8 * 4 * 24 * 20, dtype=torch.float16, device="cuda")
    whole = (dst.data_ptr(), dst.numel() * 2)
    s = dict(hip_stream=stream.cuda_stream)
    with Raises("channels 2"):
        dec.pack_tensor_nhwc(whole, (24, 20), channels=2, **s)
    with Raises("fill", "not finite"):
        dec.pack_tensor_nhwc(whole, (24, 20), channels=4, fill=float("inf"), **s)
    with Raises("region 1", "orientation 9"):
        dec.pack_tensor_nhwc(whole, (24, 20), [(0, None, None, 1), (0, None, None, 9)], **s)
    with Raises("region 0", "bicubic", "200x64", "6x20", "orientation 6 transposes"):
        dec.pack_tensor_nhwc(whole, (24, 20), [(0, (101, 3, 200, 64), (2, 4, 20, 6), 6)], **s)
    # dst_bytes below count * bytes_per_slot: both numbers; four channels need a third more than three
    three, four = 2 * 24 * 20 * 3 * 2, 2 * 24 * 20 * 4 * 2
    two = [(0, None, None, 6), (0, None, None, 1)]
    with Raises("dst_bytes", str(three - 2), str(three)):
        dec.pack_tensor_nhwc((dst.data_ptr(), three - 2), (24, 20), two, channels=3, **s)
    with Raises("dst_bytes", str(three), str(four)):
        dec.pack_tensor_nhwc((dst.data_ptr(), three), (24, 20), two, channels=4, **s)
    with Raises("aligned"):
        dec.pack_tensor_nhwc((dst.data_ptr() + 1, four), (24, 20), two, channels=4, **s)
    with Raises("grid", "does not fit"):   # (in front of the destination and the list: nothing is allocated, nothing launched)
        dec.pack_tensor_nhwc(whole, (65535, 65535), [(0, None, None, 6)] * 4096, dtype="u8", **s)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_nhwc(whole, (24, 20), **s)
    frames, batch = _five()
    with Raises("region 1", "image 5", "5 images"):
        batch.pack_tensor_nhwc(whole, (24, 20), [(4, None, None, 2), (5, None, None, 2)], **s)
    batch.wait()
    stream.synchronize()


CASES = {fn.__name__: (fn, ()) for fn in (letterbox_every_orientation_type_and_channel_count, run_edges, eight_on_a_batch_of_five,
                                          a_channels_last_torch_tensor_as_it_is, four_u8_channels_with_255_and_more_than_one_workgroup_per_band,
                                          two_packs_behind_a_decode_and_a_decode_behind_them, rejections)}


def main(out_path):
    global torch, ca, fr, orf, nr, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import gpu_orient_worker
    import nhwc_reference as nr
    orf, fr = nr.orf, nr.fr
    gpu_orient_worker.torch, gpu_orient_worker.ca = torch, ca   # (its helpers look their modules up there)
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
