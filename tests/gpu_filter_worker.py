"""The GPU cases of tests/test_gpu_filter.py, run in one process of their own that imports torch before the library
(both bring a HIP runtime and the one loaded first serves both: tests/gpu_region_worker.py has the same order).

    python tests/gpu_filter_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/filter_reference.py), bit for bit, or with
what pack_tensor_regions and pack_tensor themselves stored.  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

SENTINEL = 0x5C
GREY = (114.0, 114.0, 114.0)
COLOURS = (10.0, 114.0, 250.5)
BAND = 8   # kFilterBand (compeg_amd/csrc/kernels.h): the rows of a lane
# six regions over five images of five sizes (tests/test_filter_emulation.py: SIX): images 4 and 2 twice, image 0 not at all
SIX = ((4, (101, 3, 200, 64), (2, 4, 20, 6)), (2, (3, 1, 45, 21), (0, 3, 24, 11)), (4, None, (0, 7, 24, 5)),
       (2, (3, 1, 45, 21), (0, 3, 24, 11)), (1, (5, 2, 12, 7), (7, 0, 9, 20)), (3, (2, 0, 20, 16), (23, 19, 1, 1)))

torch = ca = fr = gpu = stream = None   # set by main(): torch first


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
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _want(a, dtype):
    """The reference's array as a torch tensor of the destination's type (bf16: from its bit patterns)."""
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


_decoders = {}


def _decoder(w, h):
    """The decoder that holds fr.frame(w, h), decoded once for all the cases that pack it."""
    if (w, h) not in _decoders:
        jpeg, rgba = fr.frame(w, h)
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        _decoders[(w, h)] = (dec, rgba)
    return _decoders[(w, h)]


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


def _pack_and_check(dec, rgba, size, regions, k, dtype, order, kernel, what, pad=COLOURS, params=None):
    """One decoder pack of `regions` into a destination of NaNs (u8: sentinels), against the reference."""
    scale, bias = params or fr.params(dtype)
    dst = torch.full((len(regions), 3, size[1], size[0]), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")
    torch.cuda.synchronize()
    dec.pack_tensor_filtered(dst, size, regions, kernel=kernel, pad=pad, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                             hip_stream=stream.cuda_stream)
    stream.synchronize()
    for r, (_, src, rect) in enumerate(regions):
        _check(dst[r], fr.expected(rgba, size, k, dtype, scale, bias, order, kernel, src, rect, pad), dtype, f"{what}, region {r}")


def every_kernel(kernel):
    """330x70 -> 31x13 (both axes shrink) and -> 224x224 (x shrinks, y grows), k = 1 and 2, f32 and f16, the ImageNet pair."""
    dec, rgba = _decoder(330, 70)
    n = 0
    for size in ((31, 13), (224, 224)):
        for k in (1, 2):
            for dtype in ("f32", "f16"):
                n += 1
                _pack_and_check(dec, rgba, size, [(0, None, None)], k, dtype, ("rgb", "bgr")[n % 2], kernel, f"{kernel} -> {size} k={k} {dtype}",
                                params=(fr.IMAGENET_SCALE, fr.IMAGENET_BIAS))


def output_heights():
    """oh of 1, one fewer than a band, a band, one more, 13 -- of a crop 20 rows high, which every kernel takes down to 1."""
    dec, rgba = _decoder(330, 70)
    for n, kernel in enumerate(fr.KERNELS):
        for oh in (1, BAND - 1, BAND, BAND + 1, 13):
            _pack_and_check(dec, rgba, (31, oh), [(0, (0, 3 + n, 330, 20), None)], 1, ("f32", "f16", "bf16", "u8")[n], "rgb", kernel, f"{kernel} oh={oh}")


def output_widths():
    """ow of 1, 63, 65 and 257: one lane, a wave less one and more one, a workgroup more one (ow = 1: of a crop 20 wide)."""
    dec, rgba = _decoder(330, 70)
    for n, kernel in enumerate(fr.KERNELS):
        for ow in (1, 63, 65, 257):
            src = (7 + n, 0, 20, 70) if ow == 1 else None
            _pack_and_check(dec, rgba, (ow, 11), [(0, src, None)], 1, ("f16", "f32", "u8", "bf16")[n], "bgr", kernel, f"{kernel} ow={ow}")


def mixed_axes():
    """One axis shrinks, the other grows, both ways round."""
    dec, rgba = _decoder(330, 70)
    for n, kernel in enumerate(fr.KERNELS):
        _pack_and_check(dec, rgba, (40, 100), [(0, None, None)], 1, "f32", ("rgb", "bgr")[n % 2], kernel, f"{kernel} 330x70 -> 40x100")
        _pack_and_check(dec, rgba, (100, 9), [(0, (10, 0, 40, 70), None)], 1, "f16", "rgb", kernel, f"{kernel} 40x70 -> 100x9")


def tap_limits():
    """Each kernel at its tap limit on one axis, x and then y: box 128 -> 1, triangle 128 -> 2, bicubic 64 -> 2, Lanczos 64 -> 3."""
    dec, rgba = _decoder(640, 360)
    for kernel, n_in, n_out in (("box", 128, 1), ("triangle", 128, 2), ("bicubic", 64, 2), ("lanczos3", 64, 3)):
        _pack_and_check(dec, rgba, (n_out, 9), [(0, (33, 5, n_in, 18), None)], 1, "f32", "rgb", kernel, f"{kernel} {n_in} -> {n_out} on x")
        _pack_and_check(dec, rgba, (17, n_out), [(0, (5, 33, 34, n_in), None)], 1, "f16", "bgr", kernel, f"{kernel} {n_in} -> {n_out} on y")
        _pack_and_check(dec, rgba, (n_out, 9), [(0, (32, 4, 2 * n_in + 1, 37), None)], 2, "f32", "rgb", kernel, f"{kernel} {n_in} -> {n_out} on x, k=2")


def letterbox():
    """330x70 fitted into 48x40 (region_fit: rows 15 .. 24, a multiple of the band neither in dy nor in dh), grey 114 around it: the
    pad outside, the filtered bits inside."""
    dec, rgba = _decoder(330, 70)
    dst = ca.region_fit((330, 70), (48, 40))
    assert dst == (0, 15, 48, 10) and dst[1] % BAND and dst[3] % BAND
    n = 0
    for kernel in fr.KERNELS:
        for dtype in fr.DTYPES:
            n += 1
            _pack_and_check(dec, rgba, (48, 40), [(0, None, dst)], 1, dtype, ("rgb", "bgr")[n % 2], kernel, f"letterbox {kernel} {dtype}", pad=GREY,
                            params=(fr.IMAGENET_SCALE, fr.IMAGENET_BIAS) if dtype != "u8" else None)
    _pack_and_check(dec, rgba, (33, 17), [(0, None, (5, 3, 21, 9)), (0, (5, 3, 20, 16), (32, 16, 1, 1)), (0, (100, 0, 20, 70), (15, 0, 1, 17))], 1, "f16",
                    "rgb", "bicubic", "inner rectangles off every border")


def batch_crop_list_inside_sentinels():
    """Six regions over five images of five sizes, one image twice with the same crop, one not at all; the
    destination lies one element into a sentinel-filled allocation."""
    frames, batch = _five()
    size = (24, 20)
    for dtype, k, kernel in (("u8", 1, "bicubic"), ("f16", 1, "lanczos3"), ("f32", 1, "box"), ("bf16", 2, "triangle"), ("f16", 2, "bicubic")):
        regions = SIX if k == 1 else SIX[:5]
        scale, bias = fr.params(dtype)
        shape, per_slot, _ = ca.filtered_tensor_shape(16, 8, size, kernel=kernel, dtype=dtype)
        needed, esize = len(regions) * per_slot, fr.ELEM_BYTES[dtype]
        buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        batch.pack_tensor_filtered((buf.data_ptr() + 64 + esize, needed), size, regions, kernel=kernel, pad=COLOURS, dtype=dtype, downscale=k, scale=scale,
                                   bias=bias, order="bgr", hip_stream=stream.cuda_stream)
        batch.wait()   # (covers the pack)
        raw = buf.cpu().numpy().tobytes()
        lo, hi = 64 + esize, 64 + esize + needed
        assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{dtype}: sentinels overwritten"
        got = fr.from_bytes(raw[lo:hi], dtype, (len(regions),) + shape)
        for r, (image, src, dst) in enumerate(regions):
            want = fr.expected(frames[image][1], size, k, dtype, scale, bias, "bgr", kernel, src, dst, COLOURS)
            assert fr.same(got[r], want, dtype), f"{dtype} k={k} {kernel} region {r}: {int((got[r] != want).sum())} of {want.size} elements differ"


def regions_none():
    """regions=None: the whole image into the whole output, one slot per image."""
    frames, batch = _five()
    dst = torch.full((5, 3, 6, 8), float("nan"), dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    batch.pack_tensor_filtered(dst, (8, 6), kernel="box", hip_stream=stream.cuda_stream)
    batch.wait()
    for i, (_, rgba) in enumerate(frames):
        _check(dst[i], fr.expected(rgba, (8, 6), 1, "f16", (1, 1, 1), (0, 0, 0), kernel="box"), "f16", f"batch, image {i}")
    dec, rgba = _decoder(330, 70)
    one = torch.full((1, 3, 13, 31), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    dec.pack_tensor_filtered(one, (31, 13), dtype="f32", hip_stream=stream.cuda_stream)
    stream.synchronize()
    _check(one[0], fr.expected(rgba, (31, 13), 1, "f32", (1, 1, 1), (0, 0, 0)), "f32", "decoder")


def u8_overshoot_clamps():
    """Bicubic and Lanczos on a frame of hard edges -- squares of 0 and 255 --, enlarged: the lobes overshoot below 0 and above
    255 (the reference's f32 values say so) and u8 clamps."""
    tr = fr.gr.rr.tr
    rgb = np.zeros((26, 50, 3), np.uint8)
    rgb[(np.arange(26)[:, None] // 8 + np.arange(50)[None, :] // 8) % 2 == 1] = 255
    jpeg = tr.synth.encode(rgb, quality=95)
    rgba = tr.orc.ImageData(jpeg).decode()
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(jpeg))
    for kernel in ("bicubic", "lanczos3"):
        for size in ((224, 224), (31, 13)):
            m = fr.inner(rgba, size, 1, "f32", *fr.IDENTITY, "rgb", kernel)
            if size == (224, 224):
                assert m.min() < -1.0 and m.max() > 256.0, (kernel, float(m.min()), float(m.max()))
            _pack_and_check(dec, rgba, size, [(0, None, None)], 1, "u8", "rgb", kernel, f"hard edges {kernel} -> {size}", params=fr.IDENTITY)


def triangle_is_the_antialiased_bilinear():
    """Where both axes shrink, triangle is pack_tensor_regions with bilinear and the antialias flag of the same regions, bit for bit."""
    frames, batch = _five()
    # (every axis shrinks at k = 1 and at k = 2: where one does not, the flag falls back to plain bilinear and triangle does not)
    regions = [(4, (101, 3, 200, 64), (2, 4, 20, 6)), (2, (3, 1, 45, 21), (0, 3, 20, 9)), (4, None, (0, 7, 24, 5)), (3, None, (0, 0, 24, 11))]
    for n, dtype in enumerate(fr.DTYPES):
        for k in (1, 2):
            scale, bias = fr.params(dtype)
            order = ("rgb", "bgr")[n % 2]
            a = torch.zeros((4, 3, 20, 24), dtype=_torch_type(dtype), device="cuda")
            b = torch.ones((4, 3, 20, 24), dtype=_torch_type(dtype), device="cuda")
            torch.cuda.synchronize()
            batch.pack_tensor_regions(a, (24, 20), regions, pad=COLOURS, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                                      hip_stream=stream.cuda_stream, antialias=True)
            batch.pack_tensor_filtered(b, (24, 20), regions, kernel="triangle", pad=COLOURS, dtype=dtype, downscale=k, scale=scale, bias=bias, order=order,
                                       hip_stream=stream.cuda_stream)
            batch.wait()
            assert torch.equal(_bits(a), _bits(b)), f"{dtype} k={k}: {int((_bits(a) != _bits(b)).sum())} elements differ from the antialiased pack"


def box_is_the_block_mean_and_the_identity_is_pack_tensor():
    """Box at 1/2, 1/4, 1/8 of 640x360 is pack_tensor at that downscale; box, triangle and bicubic at the frame's own extent are
    pack_tensor at downscale 1: bit for bit."""
    dec, _ = _decoder(640, 360)
    for n, dtype in enumerate(fr.DTYPES):
        scale, bias = fr.params(dtype)
        order = ("rgb", "bgr")[n % 2]
        for kernel, factor in (("box", 2), ("box", 4), ("box", 8), ("box", 1), ("triangle", 1), ("bicubic", 1)):
            size = (640 // factor, 360 // factor)
            a = torch.zeros((3, size[1], size[0]), dtype=_torch_type(dtype), device="cuda")
            b = torch.ones((1, 3, size[1], size[0]), dtype=_torch_type(dtype), device="cuda")
            torch.cuda.synchronize()
            dec.pack_tensor(a, dtype=dtype, downscale=factor, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream)
            dec.pack_tensor_filtered(b, size, kernel=kernel, dtype=dtype, scale=scale, bias=bias, order=order, hip_stream=stream.cuda_stream)
            stream.synchronize()
            assert torch.equal(_bits(a), _bits(b[0])), f"{kernel} {dtype} 1/{factor}: {int((_bits(a) != _bits(b[0])).sum())} elements differ from pack_tensor"


def record_staging():
    """Two filtered packs recorded one behind the other with different regions and kernels -- so different records and tables
    -- and no host wait in between, then a plain pack_tensor_resized through the same staging: each sees its own."""
    frames, batch = _five()
    size, scale, bias = (24, 20), fr.IMAGENET_SCALE, fr.IMAGENET_BIAS
    first = list(SIX)
    second = [(0, (0, 0, 8, 8), (3, 3, 8, 8)), (4, None, (0, 7, 24, 5)), (2, (25, 13, 25, 13), None)]
    crops = [(0, 0, 8, 8), (5, 2, 12, 7), (25, 13, 25, 13), (1, 1, 33, 17), (0, 0, 330, 70)]
    dst = [torch.zeros((n, 3, 20, 24), dtype=torch.float16, device="cuda") for n in (6, 3, 5)]
    torch.cuda.synchronize()
    batch.pack_tensor_filtered(dst[0], size, first, kernel="bicubic", pad=GREY, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_filtered(dst[1], size, second, kernel="lanczos3", pad=COLOURS, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.pack_tensor_resized(dst[2], size, crops=crops, dtype="f16", scale=scale, bias=bias, hip_stream=stream.cuda_stream)
    batch.wait()
    for d, regions, pad, kernel, what in ((dst[0], first, GREY, "bicubic", "first"), (dst[1], second, COLOURS, "lanczos3", "second")):
        for r, (image, src, rect) in enumerate(regions):
            _check(d[r], fr.expected(frames[image][1], size, 1, "f16", scale, bias, "rgb", kernel, src, rect, pad), "f16", f"{what} pack, region {r}")
    for i, (_, rgba) in enumerate(frames):
        _check(dst[2][i], fr.gr.inner(rgba, size, 1, "f16", scale, bias, "rgb", "bilinear", crops[i]), "f16", f"plain pack behind them, slot {i}")


def rejections():
    """A shrink beyond the tap limit is rejected, not served; nothing here launches."""
    dec, _ = _decoder(330, 70)
    dst = torch.empty(7 * 3 * 64 * 64, dtype=torch.float16, device="cuda")
    s = dict(hip_stream=stream.cuda_stream)
    with Raises("region 1", "bicubic", "by 32 at the most", "330x70", "5x3", "downscale"):   # the limit by the inner extent
        dec.pack_tensor_filtered(dst, (64, 64), [(0, None, None), (0, None, (8, 8, 5, 3))], **s)
    with Raises("region 0", "lanczos3", "330x70", "15x64"):   # 22 times on x
        dec.pack_tensor_filtered(dst, (15, 64), kernel="lanczos3", **s)
    with Raises("kernel 4"):
        dec.pack_tensor_filtered(dst, (8, 8), kernel=4, downscale=2, **s)
    with Raises("region 0", "image 1", "decoder"):
        dec.pack_tensor_filtered(dst, (8, 8), [(1, None, None)], downscale=2, **s)
    with Raises("region 1", "crop", "leaves", "330x70"):
        dec.pack_tensor_filtered(dst, (8, 8), [(0, None, None), (0, (300, 0, 31, 5), None)], downscale=2, **s)
    with Raises("pad", "channel 1", "finite"):
        dec.pack_tensor_filtered(dst, (8, 8), pad=(0, float("inf"), 0), downscale=2, **s)
    with Raises("dst_bytes", str(2 * 3 * 9 * 11 * 2)):
        dec.pack_tensor_filtered((dst.data_ptr(), 2 * 3 * 9 * 11 * 2 - 2), (11, 9), [(0, None, None)] * 2, downscale=2, **s)
    with Raises("aligned"):
        dec.pack_tensor_filtered((dst.data_ptr() + 1, 4096), (8, 8), downscale=2, **s)
    with Raises("grid", "does not fit"):   # (checked in front of the destination: nothing is launched)
        dec.pack_tensor_filtered(dst, (65535, 65535), [(0, None, None)] * 4096, dtype="u8", **s)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_filtered(dst, (8, 8), **s)
    frames, batch = _five()
    with Raises("region 1", "image 5", "5 images"):
        batch.pack_tensor_filtered(dst, (8, 8), [(4, None, None), (5, None, None)], kernel="box", **s)
    with Raises("region 2", "triangle", "330x70", "5x1"):   # only the region of the last image is beyond the limit
        batch.pack_tensor_filtered(dst, (5, 1), [(0, None, None), (3, None, None), (4, None, None)], kernel="triangle", **s)
    batch.wait()
    stream.synchronize()


def _cases():
    cases = {}
    for kernel in ("box", "triangle", "bicubic", "lanczos3"):
        cases[f"every_kernel[{kernel}]"] = (every_kernel, (kernel,))
    for fn in (output_heights, output_widths, mixed_axes, tap_limits, letterbox, batch_crop_list_inside_sentinels, regions_none, u8_overshoot_clamps,
               triangle_is_the_antialiased_bilinear, box_is_the_block_mean_and_the_identity_is_pack_tensor, record_staging, rejections):
        cases[fn.__name__] = (fn, ())
    return cases


CASES = _cases()


def main(out_path):
    global torch, ca, fr, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import filter_reference as fr
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
