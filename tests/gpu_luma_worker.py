"""The GPU cases of tests/test_gpu_luma.py, run in one process of their own that imports torch before the library (both
bring a HIP runtime and the one loaded first serves both: tests/gpu_nhwc_worker.py has the same order).

    python tests/gpu_luma_worker.py RESULTS.json

Destinations are torch CUDA tensors; the packs run on a torch stream whose handle is passed in.  Every element is
compared with the oracle's RGBA put through the header's contract (tests/luma_reference.py), bit for bit, or with plane 0
of what pack_tensor_oriented itself stored for the same arguments.  No frame is larger than 330 x 70 (the numeric ramp is
tests/numeric_edges.py's 256 x 128).  RESULTS.json: case name -> null, or what went wrong."""
import json
import os
import sys
import traceback

import numpy as np

from gpu_filter_worker import SENTINEL
from gpu_orient_worker import Raises, _bits, _torch_type, _want

torch = ca = fr = orf = lr = gpu = stream = None   # set by main(): torch first
PAD = 114.0


def _check(got, want, dtype, what):
    """torch.equal on the values: -0 and +0 are one (the library is built -fno-signed-zeros), everything else its bits."""
    want = _want(want, dtype)
    got = got.cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert not torch.isnan(got.float()).any(), f"{what}: elements that no lane wrote"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"


def _fresh(n, size, dtype, form="n1hw"):
    """A destination of NaNs (u8: sentinels) -- an element that nobody writes shows -- as [n, 1, oh, ow], [n, oh, ow, 1] or
    [n, oh, ow]."""
    shape = {"n1hw": (n, 1, size[1], size[0]), "nhw1": (n, size[1], size[0], 1), "nhw": (n, size[1], size[0])}[form]
    return torch.full(shape, SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")


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


def _pack_and_check(obj, rgba_of, size, regions, k, dtype, weights, kernel, what, pad=PAD, scale=1.0, bias=0.0, wait=None):
    """One luma pack of `regions` = (image, src, dst, o) into a fresh destination, against the reference."""
    dst = _fresh(len(regions), size, dtype)
    torch.cuda.synchronize()
    obj.pack_tensor_luma(dst, size, regions, weights=weights, kernel=kernel, pad=pad, dtype=dtype, downscale=k, scale=scale, bias=bias,
                         hip_stream=stream.cuda_stream)
    (wait or stream.synchronize)()
    for r, (image, src, rect, o) in enumerate(regions):
        with np.errstate(over="ignore"):
            want = lr.expected(rgba_of(image), size, k, dtype, scale, bias, weights, kernel, src, rect, pad, o)
        _check(dst[r, 0], want, dtype, f"{what}, region {r} (o={o})")
    return dst


def letterbox_every_orientation_and_type():
    """The 330x70 colour frame into the 48x40 letterbox (20, 0, 8, 40): o = 1 .. 8 x element type, BT.601 and BT.709
    alternating, the ImageNet pair's first component for the float types, at the smallest downscale at which the preimage
    lies within bicubic's tap limit."""
    dec, rgba, _ = _decoder()
    dst = ca.region_fit((70, 330), (48, 40))
    assert dst == (20, 0, 8, 40)
    n = 0
    for o in orf.ORIENTATIONS:
        _, _, dw, dh = orf.preimage(dst, o, (48, 40))
        k = next(k for k in (1, 2, 4, 8) if fr.axis_ok("bicubic", 330 // k, dw) and fr.axis_ok("bicubic", 70 // k, dh))
        for dtype in fr.DTYPES:
            n += 1
            scale, bias = (fr.IMAGENET_SCALE[0], fr.IMAGENET_BIAS[0]) if dtype != "u8" else (fr.U8_SCALE[0], fr.U8_BIAS[0])
            _pack_and_check(dec, lambda i: rgba, (48, 40), [(0, None, dst, o)], k, dtype, ("bt601", "bt709")[n % 2], "bicubic",
                            f"letterbox o={o} {dtype}", pad=(PAD, 250.5)[n // 2 % 2], scale=scale, bias=bias)


def run_edges():
    """o = 5 .. 8: runs of 1, 7, 8, 9 and 13 elements, the tensor one element into its allocation so that the pieces are
    misaligned; the sentinels on both sides survive."""
    frames, batch = _five()
    rgba = frames[1][1]   # 17x9
    for o in (5, 6, 7, 8):
        for ow in (1, 7, 8, 9, 13):
            for dtype in ("u8", "f16", "f32"):
                size, esize = (ow, 5), fr.ELEM_BYTES[dtype]
                scale, bias = fr.params(dtype)
                needed = 5 * ow * esize
                buf = torch.full((64 + esize + needed + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                batch.pack_tensor_luma((buf.data_ptr() + 64 + esize, needed), size, [(1, None, None, o)], kernel="bicubic", pad=PAD, dtype=dtype,
                                       scale=scale[0], bias=bias[0], hip_stream=stream.cuda_stream)
                batch.wait()
                raw = buf.cpu().numpy().tobytes()
                lo, hi = 64 + esize, 64 + esize + needed
                what = f"o={o} ow={ow} {dtype}"
                assert raw[:lo] == bytes([SENTINEL]) * lo and raw[hi:] == bytes([SENTINEL]) * 64, f"{what}: sentinels overwritten"
                got = fr.from_bytes(raw[lo:hi], dtype, (5, ow))
                want = lr.expected(rgba, size, 1, dtype, scale[0], bias[0], "bt601", "bicubic", None, None, PAD, o)
                assert fr.same(got, want, dtype), f"{what}: {int((got != want).sum())} of {want.size} elements differ"


def eight_on_a_batch_of_five():
    """EIGHT's mixed orientations over five images of five sizes, every kernel, k = 1 and 2: against the reference; and with
    weights="r" against plane 0 of the card's own pack_tensor_oriented(order="rgb") for the same arguments -- the two kernel
    families agree with each other, not only with numpy."""
    frames, batch = _five()
    scale, bias = fr.IMAGENET_SCALE, fr.IMAGENET_BIAS
    n = 0
    for kernel in fr.KERNELS:
        for k in (1, 2):
            dtype, weights = ("f16", "f32", "bf16", "u8")[n % 4], ("bt601", "bt709", "g", "b")[n // 2 % 4]
            n += 1
            s, b = (scale[0], bias[0]) if dtype != "u8" else (fr.U8_SCALE[0], fr.U8_BIAS[0])
            what = f"EIGHT {kernel} k={k} {dtype}"
            _pack_and_check(batch, lambda i: frames[i][1], orf.SLOT, list(orf.EIGHT), k, dtype, weights, kernel, f"{what} {weights}", scale=s, bias=b,
                            wait=batch.wait)
            red = _pack_and_check(batch, lambda i: frames[i][1], orf.SLOT, list(orf.EIGHT), k, dtype, "r", kernel, f"{what} r", scale=s, bias=b,
                                  wait=batch.wait)
            planar = torch.full((8, 3, orf.SLOT[1], orf.SLOT[0]), SENTINEL if dtype == "u8" else float("nan"), dtype=_torch_type(dtype), device="cuda")
            torch.cuda.synchronize()
            batch.pack_tensor_oriented(planar, orf.SLOT, list(orf.EIGHT), kernel=kernel, pad=(PAD,) * 3, dtype=dtype, downscale=k,
                                       scale=(s,) * 3, bias=(b,) * 3, order="rgb", hip_stream=stream.cuda_stream)
            batch.wait()
            x, y = _bits(red[:, 0]), _bits(planar[:, 0])
            assert torch.equal(x, y), f"{what}: {int((x != y).sum())} elements differ from plane 0 of the oriented pack"


def grayscale_frames():
    """A decoder on a one-component frame, and a batch that mixes it with a colour 4:2:2 frame: u8 at the identity extent
    with triangle, scale 1, bias 0.  The gray slot is the frame's luma byte for byte under "bt601", "bt709" and "g" alike;
    the colour slot (a crop of the gray frame's extent) equals the reference.  [N, 1, oh, ow], [N, oh, ow, 1] and
    [N, oh, ow] destinations receive the same bytes."""
    import coef_stream as cs
    import gray_stream as gs
    from oracle import oracle as orc
    f = gs.case("random_gray/short/gray/reference/dri2/w5")
    c = cs.case("texture/edge/422/reference/dri4")
    luma, colour = gs.expectation(f), orc.ImageData(c.jpeg()).decode()
    assert not np.array_equal(lr.luma(colour, "bt601"), lr.luma(colour, "bt709")), "the colour frame does not tell the weights apart"
    size, crop = (f.w, f.h), (8, 4, f.w, f.h)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(f.jpeg(), **f.image_kw()))
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()), ca.ImageData(c.jpeg())])
    batch.decode()
    batch.wait()
    regions = [(0, None, None, 1), (1, crop, None, 1)]
    first = None
    for weights in ("bt601", "bt709", "g"):
        one = _fresh(1, size, "u8")
        torch.cuda.synchronize()
        dec.pack_tensor_luma(one, size, weights=weights, kernel="triangle", dtype="u8", hip_stream=stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(one[0, 0].cpu().numpy(), luma[..., 0]), f"decoder, {weights}: the slot is not the frame's luma"
        for form in ("n1hw", "nhw1", "nhw"):
            dst = _fresh(2, size, "u8", form)
            torch.cuda.synchronize()
            batch.pack_tensor_luma(dst, size, regions, weights=weights, kernel="triangle", dtype="u8", hip_stream=stream.cuda_stream)
            batch.wait()
            got = dst.reshape(2, f.h, f.w).cpu().numpy()
            assert np.array_equal(got[0], luma[..., 0]), f"batch, {weights}, {form}: the gray slot is not the frame's luma"
            want = lr.expected(colour, size, 1, "u8", 1.0, 0.0, weights, "triangle", crop)
            assert np.array_equal(got[1], want), f"batch, {weights}, {form}: {int((got[1] != want).sum())} elements of the colour slot differ"
            if form == "n1hw":
                first = dst
            else:
                assert dst.cpu().numpy().tobytes() == first.cpu().numpy().tobytes(), f"{weights}: {form} received other bytes than [N, 1, oh, ow]"


_ramp = None


def numeric_edges():
    """Component 0 of each (scale, bias) set of tests/numeric_edges.py on its ramp frame at the identity extent (triangle):
    ties, subnormals, infinities, the u8 clamp.  As f32 the ramp goes to 257 x 129 with bicubic as well, where a fused
    multiply-add would show."""
    global _ramp
    import numeric_edges as ne
    assert ne.denormals_kept()
    if _ramp is None:
        jpeg, rgba = ne.ramp()
        dec = ca.Decoder(gpu)
        dec.decode_blocking(ca.ImageData(jpeg))
        _ramp = (dec, rgba)
    dec, rgba = _ramp
    for name, (dtypes, scale, bias) in ne.SETS.items():
        for n, dtype in enumerate(dtypes):
            weights = ("bt601", "bt709")[n % 2]
            _pack_and_check(dec, lambda i: rgba, (ne.RAMP_W, ne.RAMP_H), [(0, None, None, 1)], 1, dtype, weights, "triangle", f"{name} {dtype}",
                            scale=scale[0], bias=bias[0])
            if dtype == "f32":
                _pack_and_check(dec, lambda i: rgba, (257, 129), [(0, None, None, 1)], 1, dtype, weights, "bicubic", f"{name} {dtype} 257x129",
                                scale=scale[0], bias=bias[0])


def ordered_behind_a_stalled_decode():
    """stall(A), the decode of a new frame on A, the luma pack on B, the decode of the old frame again on A, no host wait:
    the destination holds the new frame's values (a pack that overtook its decode, or was overtaken by the next one, would
    hold the old frame's), and the texture then reads back as the old frame.  The window was open: the pack was issued while
    the stalled stream had not drained."""
    import stream_stall as ss
    A, B = ss.independent_pair()
    spare = torch.cuda.Stream()
    (old_jpeg, old), (new_jpeg, new) = fr.frame(50, 26, seed=5), fr.frame(50, 26, seed=6)
    size, regions = (24, 20), [(0, None, None, 6), (0, (3, 1, 45, 21), (1, 3, 11, 13), 3)]
    args = dict(weights="bt709", kernel="bicubic", pad=PAD, dtype="f32", scale=fr.IMAGENET_SCALE[0], bias=fr.IMAGENET_BIAS[0])

    def want(rgba):
        return np.stack([lr.expected(rgba, size, 1, "f32", args["scale"], args["bias"], "bt709", "bicubic", src, rect, PAD, o)
                         for _, src, rect, o in regions])
    assert not np.array_equal(want(new), want(old)), "the two outcomes this case must tell apart are the same"
    dec = ca.Decoder(gpu)
    # (its buffers, record block and pinned slot get their sizes now: nothing is allocated inside the window)
    for jpeg in (new_jpeg, old_jpeg):
        dec.decode_blocking(ca.ImageData(jpeg))
    dec.pack_tensor_luma(_fresh(2, size, "f32"), size, regions, hip_stream=spare.cuda_stream, **args)
    spare.synchronize()
    dst = _fresh(2, size, "f32")
    staged_new, staged_old = ca.ImageData(new_jpeg), ca.ImageData(old_jpeg)
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    dec.pack_tensor_luma(dst, size, regions, hip_stream=B.cuda_stream, **args)
    dec.enqueue(staged_old, A.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, "the stalled stream had drained before the consumer was issued: the case did not test the ordering"
    _check(dst[:, 0], want(new), "f32", "the pack between the stalled decode and the next one")
    assert np.array_equal(dec.read_texture(50, 26), old), "the decode behind the pack did not leave the old frame"


def rejections_on_the_card():
    """Nothing here launches."""
    dec, _, _ = _decoder()
    dst = torch.empty(8 * 24 * 20, dtype=torch.float16, device="cuda")
    whole = (dst.data_ptr(), dst.numel() * 2)
    s = dict(hip_stream=stream.cuda_stream)
    two = [(0, None, None, 6), (0, None, None, 1)]
    need = 2 * 24 * 20 * 2
    with Raises("dst_bytes", str(need - 1), str(need)):
        dec.pack_tensor_luma((dst.data_ptr(), need - 1), (24, 20), two, **s)
    with Raises("aligned"):
        dec.pack_tensor_luma((dst.data_ptr() + 1, need), (24, 20), two, **s)
    with Raises("holds 6 slots", "packs 2"):   # (Python's own: the oriented pack's tensor is no luma destination)
        dec.pack_tensor_luma(torch.empty(2, 3, 20, 24, dtype=torch.float16, device="cuda"), (24, 20), two, **s)
    with Raises("sum 65535"):
        dec.pack_tensor_luma(whole, (24, 20), two, weights=(19595, 38470, 7470), **s)
    with Raises("pad", "not finite"):
        dec.pack_tensor_luma(whole, (24, 20), two, pad=float("nan"), **s)
    with Raises("region 1", "orientation 9"):
        dec.pack_tensor_luma(whole, (24, 20), [(0, None, None, 1), (0, None, None, 9)], **s)
    with Raises("region 0", "bicubic", "200x64", "6x20", "orientation 6 transposes"):
        dec.pack_tensor_luma(whole, (24, 20), [(0, (101, 3, 200, 64), (2, 4, 20, 6), 6)], **s)
    fresh = ca.Decoder(gpu)
    with Raises("nothing decoded"):
        fresh.pack_tensor_luma(whole, (24, 20), **s)
    frames, batch = _five()
    with Raises("nothing decoded"):
        ca.Batch(gpu).pack_tensor_luma(whole, (24, 20), [(0, None, None, 1)], **s)
    with Raises("region 1", "image 5", "5 images"):
        batch.pack_tensor_luma(whole, (24, 20), [(4, None, None, 2), (5, None, None, 2)], **s)
    batch.wait()
    stream.synchronize()


CASES = {fn.__name__: (fn, ()) for fn in (letterbox_every_orientation_and_type, run_edges, eight_on_a_batch_of_five, grayscale_frames, numeric_edges,
                                          ordered_behind_a_stalled_decode, rejections_on_the_card)}


def main(out_path):
    global torch, ca, fr, orf, lr, gpu, stream
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import gpu_orient_worker
    import luma_reference as lr
    orf, fr = lr.orf, lr.fr
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
