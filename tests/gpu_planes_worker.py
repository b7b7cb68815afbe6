"""The GPU cases of tests/test_gpu_planes.py: Decoder.decode_planes / Batch.decode_planes into torch memory, every byte
against tests/planes_stream.py -- the destination between sentinels and over a pre-fill, so that what must not be written
shows.  Run in one process of their own that imports torch before the library (tests/gpu_luma_worker.py: why).

    python tests/gpu_planes_worker.py RESULTS.json [substring of the case names to run]

Every decode asserts last_kernel() == "planes".  RESULTS.json: case name -> null, or what went wrong; "wall_s"."""
import io
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ps = cs = gs = orc = ss = gpu = None   # set by main(): torch first
GUARD, SENTINEL, PREFILL = 256, 0x5C, 0x3C
ALL_422 = (("planar", "coded"), ("semiplanar", "coded"), ("yuyv", "coded"), ("uyvy", "coded"), ("planar", "420"), ("semiplanar", "420"))
FORMATS_OF = {"422": ALL_422, "444": ALL_422[:2], "440": ALL_422[:2], "420": ALL_422[:2], "gray": ALL_422[:1]}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Dest:
    """n images' worth of destination inside one torch block: sentinels, `shift` bytes, the planes over a pre-fill, sentinels."""

    def __init__(self, total, n=1, shift=0):
        self.total, self.n, self.shift = total, n, shift
        self.block = torch.full((GUARD + shift + total * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.block[GUARD + shift:GUARD + shift + total * n] = PREFILL
        torch.cuda.synchronize()

    @property
    def range(self):
        return (self.block.data_ptr() + GUARD + self.shift, self.total * self.n)

    def read(self, what):
        """[n, total] bytes; the sentinels checked."""
        torch.cuda.synchronize()
        host = self.block.cpu().numpy()
        body = host[GUARD + self.shift:GUARD + self.shift + self.total * self.n]
        assert (host[:GUARD + self.shift] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), f"{what}: a sentinel was written"
        return body.reshape(self.n, self.total)


def _geometry(f, format, chroma, pitched):
    comps, hs, vs = ps.sampling_of(f)
    pitch = None
    if pitched:
        rows = [p[2] for p in ps.layout(f.w, f.h, comps, hs, vs, format, chroma)[0]]
        pitch = ((rows[0] + 15) // 16 * 16 + 16, (rows[-1] + 15) // 16 * 16 + 32 if len(rows) > 1 else 0)
    lay, total = ps.layout(f.w, f.h, comps, hs, vs, format, chroma, pitch)
    mine, total_lib = ca.planes_shape(f.w, f.h, (hs, vs), comps, format, chroma, pitch)
    assert total_lib == total and [(p["offset"], p["pitch"], p["row_bytes"]) for p in mine] == [p[:3] for p in lay]
    return (comps, hs, vs), pitch, total


def _want(planes, f, format, chroma, pitch, total):
    comps, hs, vs = ps.sampling_of(f)
    return ps.destination(planes, f.w, f.h, comps, hs, vs, format, chroma, pitch, before=np.full(total, PREFILL, dtype=np.uint8))


def _compare(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def _planes_of(f):
    """(MCUs behind the last complete interval: what the reference makes of the file's extra segment is the oracle's to say)"""
    return ps.file_planes(ca, f.jpeg(), **f.image_kw())[0] if "/short" in f.name else ps.frame_planes(f)


def decoder_case(f, format="planar", chroma="coded", pitched=False, shift=0, device=False, planes=None, dec=None, blocking=True):
    planes = planes if planes is not None else _planes_of(f)
    _, pitch, total = _geometry(f, format, chroma, pitched)
    dec = dec or ca.Decoder(gpu)
    dec.set_device_preprocess(device)
    dst = Dest(total, 1, shift)
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    if blocking:
        dec.decode_planes(img, dst.range, format, chroma, pitch, blocking=True)
    else:
        s = torch.cuda.Stream()
        dec.decode_planes(img, dst.range, format, chroma, pitch, hip_stream=s.cuda_stream)
        s.synchronize()
    what = f"{f.name}: Decoder, {format}/{chroma}, {'pitched' if pitched else 'tight'}, shift {shift}, {'device' if device else 'host'} preprocessing"
    assert dec.last_kernel() == "planes", f"{what}: last_kernel() = {dec.last_kernel()}"
    _compare(dst.read(what)[0], _want(planes, f, format, chroma, pitch, total), what)
    return dec


def batch_case(frames, format="planar", chroma="coded", pitched=False, shift=0, mode=0, chunk=0, planes=None, batch=None):
    f = frames[0]
    _, pitch, total = _geometry(f, format, chroma, pitched)
    if batch is None:
        batch = ca.Batch(gpu)
        batch.set_device_preprocess(mode)
        batch.upload([ca.ImageData(x.jpeg(), **x.image_kw()) for x in frames])
        batch.set_chunk(chunk)
    dst = Dest(total, len(frames), shift)
    batch.decode_planes(dst.range, format, chroma, pitch)
    batch.wait()
    what = f"{f.name} x{len(frames)}: Batch, {format}/{chroma}, {'pitched' if pitched else 'tight'}, shift {shift}, mode {mode}, chunk {chunk}"
    assert batch.last_kernel() == "planes", f"{what}: last_kernel() = {batch.last_kernel()}"
    got = dst.read(what)
    for i, x in enumerate(frames):
        _compare(got[i], _want(planes[i] if planes else _planes_of(x), x, format, chroma, pitch, total), f"{what}, image {i}")
    return batch


# ---- the cases -------------------------------------------------------------------------------------------------------

def _sizes(layout):
    """(w, h, DRIs): one MCU, one MCU plus a pixel (2 x 2 MCUs), three MCUs less a pixel (3 x 3), and seven MCUs across."""
    hs, vs = ps.SAMPLINGS[layout]
    mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
    return ((mw, mh, (0, 1)), (mw + 1, mh + 1, (0, 1, 2, 4)), (3 * mw - 1, 3 * mh - 1, (0, 1, 3)), (7 * mw - 5, mh - 3, (7,)))


def geometry_and_intervals(layout):
    seen, n = set(), 0
    dec = ca.Decoder(gpu)
    for w, h, dris in _sizes(layout):
        for ri in dris:
            seen.add(ri)
            n += 1
            std = n % 2 == 0
            format, chroma = FORMATS_OF[layout][n % len(FORMATS_OF[layout])]
            f = ps.sized(layout, w, h, ri, standard=std, seed=n)
            planes = ps.frame_planes(f)
            decoder_case(f, format, chroma, pitched=n % 3 == 0, shift=n % 2, device=n % 4 == 1, planes=planes, dec=dec)
            frames = [f, ps.sized(layout, w, h, ri, standard=std, seed=n + 50), ps.sized(layout, w, h, ri, standard=std, seed=n + 90)]
            batch_case(frames, format, chroma, pitched=n % 3 != 0, shift=(n + 1) % 2, mode=n % 3)
    assert seen == {0, 1, 2, 3, 4, 7}


def many_intervals():
    """40 x 24 MCUs at DRI 1: 960 intervals, fifteen waves, more than one workgroup."""
    for layout in ("422", "420", "gray"):
        hs, vs = ps.SAMPLINGS[layout]
        f = ps.sized(layout, 40 * 8 * hs - 3, 24 * 8 * (vs if layout != "gray" else 1) - 1, 1, seed=11)
        assert f.intervals == 960
        planes = ps.frame_planes(f)
        for format, chroma in FORMATS_OF[layout]:
            decoder_case(f, format, chroma, pitched=True, planes=planes, blocking=False)
        decoder_case(f, pitched=False, shift=1, planes=planes, device=True)
        batch_case([f, f], planes=[planes, planes], pitched=True, chunk=1)


def _noise(mode):
    from PIL import Image
    rng = np.random.default_rng(9)
    out = io.BytesIO()
    if mode == "L":
        Image.fromarray(rng.integers(0, 256, (256, 256)).astype(np.uint8), "L").save(out, "JPEG", quality=95)
    else:
        Image.fromarray(rng.integers(0, 256, (256, 256, 3)).astype(np.uint8), "RGB").save(out, "JPEG", quality=95, subsampling=1)
    j = out.getvalue()
    assert len(gs.file_scan(j)) > 6144 * 4, "the one interval must be longer than the window cap"
    return j


def _file_case(name, j, kw, formats, dec=None):
    planes, (w, h, comps, hs, vs) = ps.file_planes(ca, j, **kw)
    img = ca.ImageData(j, **kw)
    dec = dec or ca.Decoder(gpu)
    for format, chroma in formats:
        _, total = ps.layout(w, h, comps, hs, vs, format, chroma)
        dst = Dest(total)
        dec.decode_planes(img, dst.range, format, chroma, blocking=True)
        assert dec.last_kernel() == "planes", name
        want = ps.destination(planes, w, h, comps, hs, vs, format, chroma, None, before=np.full(total, PREFILL, dtype=np.uint8))
        _compare(dst.read(name)[0], want, f"{name}: {format}/{chroma}, {kw}")
    return dec, img, (w, h, comps, hs, vs)


def interval_longer_than_the_window():
    """PIL's 256 x 256 noise without DRI, grayscale and 4:2:2: one lane, global reads beyond the window cap; both entropy modes."""
    for std in (False, True):
        _file_case("noise_256 L", _noise("L"), dict(allow_grayscale=True, standard_entropy=std), ALL_422[:1])
        _file_case("noise_256 RGB 4:2:2", _noise("RGB"), dict(standard_entropy=std), (ALL_422[0], ALL_422[2], ALL_422[5]))


def families_that_break_readers():
    frames = [f for f in cs.cases() if f.family in ("q1_underflow", "dc_hostile", "positions", "dc_wrap")]
    frames += [f for f in gs.cases() if f.family in ("q1_underflow", "dc_hostile", "positions", "dc_wrap")]
    assert {f.family for f in frames} == {"q1_underflow", "dc_hostile", "positions", "dc_wrap"} and {f.standard for f in frames} == {False, True}
    dec = ca.Decoder(gpu)
    for i, f in enumerate(frames):
        layout = "gray" if isinstance(f, gs.GrayFrame) else f.layout
        format, chroma = FORMATS_OF[layout][i % len(FORMATS_OF[layout])]
        planes = ps.frame_planes(f)
        decoder_case(f, format, chroma, planes=planes, dec=dec, device=i % 2 == 1)
        batch_case([f], format, chroma, planes=[planes], pitched=True)


def formats_on_422():
    """Every format and the 4:2:0 option, tight and pitched, aligned and one byte off; a truncated last interval."""
    frames = [ps.sized("422", 16, 8, 0), ps.sized("422", 17, 9, 2, seed=4), ps.sized("422", 47, 23, 3, standard=True, seed=8),
              ps.sized("422", 48, 23, 4, seed=2, short=3)]
    dec = ca.Decoder(gpu)
    for f in frames:
        planes = _planes_of(f)
        if "/short" in f.name:
            assert not planes[3][0].all(), "the frame must have MCUs behind its last complete interval"
        for format, chroma in ALL_422:
            for pitched, shift in ((False, 0), (False, 1), (True, 0), (True, 3)):
                decoder_case(f, format, chroma, pitched, shift, planes=planes, dec=dec)
        if "/short" not in f.name:
            for format, chroma in ALL_422:
                batch_case([f, f, f], format, chroma, pitched=True, planes=[planes] * 3, chunk=2)


def consistency_with_the_rgba_decode():
    """Every golden file the decoder accepts: the card's planes through the host colour step are the card's own RGBA."""
    files = ps.golden_files(ca, GOLDEN)
    assert len(files) >= 6
    dec = ca.Decoder(gpu)
    for name, j, kw in files:
        img = ca.ImageData(j, **kw)
        w, h, comps, (hs, vs) = img.width(), img.height(), img.components(), img.sampling()
        dec.decode_blocking(img)
        rgba = dec.read_texture(w, h)
        lay, total = ps.layout(w, h, comps, hs, vs)
        dst = Dest(total)
        dec.decode_planes(img, dst.range, blocking=True)
        assert dec.last_kernel() == "planes", name
        assert np.array_equal(dec.read_texture(w, h), rgba), f"{name}: the planes decode touched the texture"
        got = dst.read(name)[0]
        y, cb, cr = (ps.views(got, w, h, comps, hs, vs) + [None, None])[:3]
        # (a pixel no complete interval covers: RGBA zero there, the plane's pre-fill here)
        covered = rgba[..., 3] == 255
        assert np.array_equal(ps.colour(y, cb, cr, hs, vs, w, h, covered), rgba), f"{name}: planes and RGBA disagree"
        if not covered.all():
            assert (y[~covered] == PREFILL).all(), f"{name}: luma was written where nothing was decoded"


def batches():
    """Three images of one size and different content: chunks of two, the three preprocessing modes, RGBA decodes before and
    after with their outputs unchanged, two specs one after the other."""
    for layout, (w, h, ri) in (("422", (63, 33, 4)), ("420", (47, 31, 3)), ("gray", (23, 17, 1))):
        frames = [ps.sized(layout, w, h, ri, seed=s) for s in (1, 30, 77)]
        planes = [ps.frame_planes(f) for f in frames]
        rgba = [gs.expectation(f) if layout == "gray" else orc.ImageData(f.jpeg(), **f.image_kw()).decode() for f in frames]
        for mode in (0, 1, 2):
            batch = ca.Batch(gpu)
            batch.set_device_preprocess(mode)
            batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in frames])
            batch.set_chunk(2)
            batch.decode()
            batch.wait()
            first = batch.last_kernel()
            assert first != "planes"
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} before"
            specs = FORMATS_OF[layout]
            batch_case(frames, *specs[0], planes=planes, batch=batch, mode=mode, chunk=2)
            batch_case(frames, *specs[-1], pitched=True, shift=1, planes=planes, batch=batch, mode=mode, chunk=2)
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} after the planes decodes"
            batch.decode()
            batch.wait()
            assert batch.last_kernel() == first
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} decoded again"
            batch_case(frames, *specs[0], planes=planes, batch=batch, mode=mode, chunk=2)


class Raises:
    def __init__(self, code, *words):
        self.code, self.words = code, words

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        assert kind is not None and issubclass(kind, ca.Error), f"no error where {self.words} was expected"
        assert e.code == self.code and all(w in str(e) for w in self.words) and "COMPEG_" not in str(e), (e.code, str(e))
        return True


def refusals_on_the_card():
    """Nothing here launches; the destination keeps its pre-fill."""
    f = ps.sized("422", 33, 17, 0)
    img = ca.ImageData(f.jpeg())
    total = ps.layout(33, 17, 3, 2, 1)[1]
    dst = Dest(total * 3, 1)
    addr = dst.range[0]
    dec = ca.Decoder(gpu)
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(total - 1), str(total)):
        dec.decode_planes(img, (addr, total - 1))
    with Raises(ca.E_INVALID_ARG, "device_dst is NULL"):
        dec.decode_planes(img, (0, total))
    with Raises(ca.E_INVALID_ARG, "luma_pitch 32", "33 bytes"):
        dec.decode_planes(img, (addr, total * 3), pitch=32)
    with Raises(ca.E_INVALID_ARG, "chroma 1 (4:2:0)", "packed"):
        dec.decode_planes(img, (addr, total * 3), "yuyv", "420")
    img444 = ca.ImageData(ps.sized("444", 33, 17, 0).jpeg(), allow_sampling=True)
    with Raises(ca.E_UNSUPPORTED, "4:2:2 files only", "4:4:4"):
        dec.decode_planes(img444, (addr, total * 3), "uyvy")
    with Raises(ca.E_UNSUPPORTED, "from 4:2:2 files only", "4:4:4"):
        dec.decode_planes(img444, (addr, total * 3), "planar", "420")
    assert dec.last_kernel() == "none"
    batch = ca.Batch(gpu)
    with Raises(ca.E_INVALID_ARG, "nothing uploaded"):
        batch.decode_planes((addr, total * 3))
    batch.upload([img, img, img])
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(3 * total - 1), str(3 * total), "3 image"):
        batch.decode_planes((addr, 3 * total - 1))
    batch.upload([img, ca.ImageData(ps.sized("422", 33, 9, 0).jpeg())])
    with Raises(ca.E_INVALID_ARG, "not all of one size", "image 1", "33x9", "33x17"):
        batch.decode_planes((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("440", 33, 17, 0).jpeg(), allow_sampling=True)])
    with Raises(ca.E_INVALID_ARG, "not all of one sampling", "image 1", "4:4:0", "4:2:2"):
        batch.decode_planes((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("gray", 33, 17, 0).jpeg(), allow_grayscale=True)])
    with Raises(ca.E_INVALID_ARG, "not all of one sampling", "grayscale"):
        batch.decode_planes((addr, total * 3))
    assert (dst.read("refusals") == PREFILL).all()


WINDOW = "the stalled stream had drained before the consumer was issued: the case did not test the ordering"


def _u8_pack_want(rgba):
    return np.ascontiguousarray(rgba[..., :3].transpose(2, 0, 1))


def ordering_batch():
    """stall(A); RGBA decode on A; planes decode on B; pack of the RGBA outputs on C, with nothing but the library's events
    between them: the pack reads the new frames only if the planes decode waited for the decode and the pack for the planes
    decode (it orders itself behind the batch's last stream, B).  The planes are the new frames' too."""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    rgba = {id(f): orc.ImageData(f.jpeg()).decode() for f in old + new}
    want_new, want_old = np.stack([_u8_pack_want(rgba[id(f)]) for f in new]), np.stack([_u8_pack_want(rgba[id(f)]) for f in old])
    assert not np.array_equal(want_new, want_old), "the two outcomes this case must tell apart are the same"
    _, pitch, total = _geometry(new[0], "semiplanar", "420", False)
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(f.jpeg()) for f in old])
    batch.decode()
    batch.pack_tensor(torch.empty((2, 3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")   # (everything gets its size now)
    batch.decode_planes(Dest(total, 2).range, "semiplanar", "420")
    batch.wait()
    batch.upload([ca.ImageData(f.jpeg()) for f in new])   # (the outputs still hold the old frames)
    dst = Dest(total, 2)
    packed = torch.full((2, 3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode(A.cuda_stream)
    batch.decode_planes(dst.range, "semiplanar", "420", hip_stream=B.cuda_stream)
    batch.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert batch.last_kernel() == "planes"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(ps.frame_planes(f), f, "semiplanar", "420", pitch, total), f"ordering, batch: planes of image {i}")
    assert np.array_equal(packed.cpu().numpy(), want_new), "the pack on the third stream did not read the decode on the first"


def ordering_decoder():
    """stall(A); enqueue(new) on A; decode_planes(other) on B -- it rewrites the decoder's one set of input buffers, so it must
    not run before the decode on A has read them; a pack of the texture on C.  The texture and the pack are the new frame's
    only if the planes decode waited for the decode, the planes are the other frame's, and a decode on C afterwards
    leaves them alone.  (The window is looked at before the planes decode is issued: an upload waits on the host for the
    previous one's staging.)"""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    rgba_new, rgba_old = orc.ImageData(new.jpeg()).decode(), orc.ImageData(old.jpeg()).decode()
    assert not np.array_equal(rgba_new, rgba_old)
    _, pitch, total = _geometry(other, "yuyv", "coded", False)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dec.pack_tensor(torch.empty((3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    dec.decode_planes(ca.ImageData(other.jpeg()), Dest(total).range, "yuyv", blocking=True)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dst = Dest(total)
    packed = torch.full((3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    staged_new, staged_other, staged_old = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg()), ca.ImageData(old.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    open_ = ss.window_open(A)
    dec.decode_planes(staged_other, dst.range, "yuyv", hip_stream=B.cuda_stream)
    assert dec.last_kernel() == "planes"
    dec.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert np.array_equal(dec.read_texture(48, 32), rgba_new), "the decode on the first stream did not decode its own frame"
    assert np.array_equal(packed.cpu().numpy(), _u8_pack_want(rgba_new)), "the pack on the third stream did not read the decode on the first"
    want = _want(ps.frame_planes(other), other, "yuyv", "coded", pitch, total)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the planes")
    dec.enqueue(staged_old, Cs.cuda_stream)
    Cs.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dec.read_texture(48, 32), rgba_old)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the planes after the next decode")


def tables_beyond_the_lds_share():
    """Frames whose Huffman tables outgrow their share of LDS (cs.wide_cases, gs.wide_cases; cs.table_regime): every regime-B
    and regime-C frame of every sampling through the Decoder -- the direct tables staged in part, L2 lookups from global
    memory beyond entry 12288 --, and batches of images of one size whose regimes are A, B and C: planned with the largest
    image's tables while each image stages its own."""
    import wide_emul as we
    for layout in we.SAMPLINGS:
        dec = ca.Decoder(gpu)
        for i, f in enumerate(x for x in we.frames((layout,)) if we.regime(x) != "A"):
            format, chroma = FORMATS_OF[layout][i % len(FORMATS_OF[layout])]
            decoder_case(f, format, chroma, pitched=i % 3 == 0, shift=i % 2, device=i % 4 == 1, planes=ps.frame_planes(f), dec=dec, blocking=i % 5 != 0)
        for n, frames in enumerate(we.same_size_batches(layout)):
            format, chroma = FORMATS_OF[layout][n % len(FORMATS_OF[layout])]
            batch_case(frames, format, chroma, pitched=n == 0, shift=n, mode=n * 2, chunk=2, planes=[ps.frame_planes(f) for f in frames])


CASES = {f"geometry_and_intervals[{lay}]": (geometry_and_intervals, (lay,)) for lay in ("422", "444", "440", "420", "gray")}
CASES.update({fn.__name__: (fn, ()) for fn in (many_intervals, interval_longer_than_the_window, families_that_break_readers, formats_on_422,
                                               consistency_with_the_rgba_decode, batches, refusals_on_the_card, tables_beyond_the_lds_share, ordering_batch, ordering_decoder)})


def main(out_path, only=""):
    global torch, ca, ps, cs, gs, orc, ss, gpu
    t0 = time.time()
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import coef_stream as cs
    import gray_stream as gs
    import planes_stream as ps
    import stream_stall as ss
    from oracle import oracle as orc
    gpu = ca.Gpu.open(0)
    results, device_said_no = {}, False
    for name, (fn, args) in CASES.items():
        if only not in name:
            continue
        t1 = time.time()
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
        print(f"{name}: {'ok' if results[name] is None else 'FAILED'} in {time.time() - t1:.2f} s", flush=True)
        results["wall_s"] = round(time.time() - t0, 2)
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
        if device_said_no:   # nothing more is started on it
            break
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
