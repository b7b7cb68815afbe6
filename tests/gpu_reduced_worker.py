"""The GPU cases of tests/test_gpu_reduced.py: Decoder.decode_reduced / Batch.decode_reduced into torch memory, every byte
against tests/reduced_stream.py -- the destination between sentinels and over a pre-fill, so that what must not be written
shows.  Run in one process of their own that imports torch before the library (tests/gpu_luma_worker.py: why).

    python tests/gpu_reduced_worker.py RESULTS.json [substring of the case names to run]

Every decode asserts last_kernel() == "reduced".  RESULTS.json: case name -> null, or what went wrong; "wall_s"."""
import io
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ps = rs = cs = gs = orc = ss = gpu = None   # set by main(): torch first
GUARD, SENTINEL, PREFILL = 256, 0x5C, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 324 x 70: ceil(324 / 8) = 41 is odd where 4:2:2 and 4:2:0 have 21 MCUs = 42 pixels a row, and 4:2:0 / 4:4:0 have 5 MCU
# rows = 10 for oh = 9: both edges cut an MCU.  The DRIs divide the MCU counts (189, 105, 369, 205, 369); 0: no DRI, one lane.
DRIS = {"422": (1, 3, 21, 0), "420": (3, 5), "444": (3, 41), "440": (5,), "gray": (3,)}
FAMILIES = ("dc_cats", "dc_hostile", "q1_underflow", "dc_wrap", "dc_sweep", "saturated", "gamut", "random_dense")


class Dest:
    """n images' worth of destination inside one torch block: sentinels, `shift` bytes, the images over a pre-fill, sentinels."""

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


def _geometry(w, h, format, pitched):
    ow = -(-w // 8)
    pitch = (4 * ow + 15) // 16 * 16 + 16 if pitched and format == "rgba" else None
    mine = rs.shape(w, h, format, pitch)
    assert ca.reduced_shape(w, h, format, pitch) == mine
    return pitch, mine[3]


def _want(red, f, format, pitch, total):
    comps, hs, vs = ps.sampling_of(f)
    return rs.destination(red, f.w, f.h, hs, vs, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8))


def _compare(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def _shift(format, odd):
    """Bytes behind the 256-byte guard: the rgba destination needs a multiple of 4, the planar one takes any address."""
    return (4 if format == "rgba" else 1) if odd else 0


def decoder_case(f, format="rgba", pitched=False, odd=False, device=False, red=None, dec=None, blocking=True):
    red = red if red is not None else rs.frame_reduced(f, ca=ca)
    pitch, total = _geometry(f.w, f.h, format, pitched)
    dec = dec or ca.Decoder(gpu)
    dec.set_device_preprocess(device)
    dst = Dest(total, 1, _shift(format, odd))
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    if blocking:
        dec.decode_reduced(img, dst.range, format, pitch, blocking=True)
    else:
        s = torch.cuda.Stream()
        dec.decode_reduced(img, dst.range, format, pitch, hip_stream=s.cuda_stream)
        s.synchronize()
    what = f"{f.name}: Decoder, {format}, {'pitched' if pitched else 'tight'}, {'odd' if odd else 'aligned'}, {'device' if device else 'host'} preprocessing"
    assert dec.last_kernel() == "reduced", f"{what}: last_kernel() = {dec.last_kernel()}"
    _compare(dst.read(what)[0], _want(red, f, format, pitch, total), what)
    return dec


def batch_case(frames, format="rgba", pitched=False, odd=False, mode=0, chunk=0, reds=None, batch=None):
    f = frames[0]
    pitch, total = _geometry(f.w, f.h, format, pitched)
    if batch is None:
        batch = ca.Batch(gpu)
        batch.set_device_preprocess(mode)
        batch.upload([ca.ImageData(x.jpeg(), **x.image_kw()) for x in frames])
        batch.set_chunk(chunk)
    # (image i lies at i * total: with an rgba destination every image's base is a multiple of 4, since the pitch is)
    dst = Dest(total, len(frames), _shift(format, odd))
    batch.decode_reduced(dst.range, format, pitch)
    batch.wait()
    what = f"{f.name} x{len(frames)}: Batch, {format}, {'pitched' if pitched else 'tight'}, {'odd' if odd else 'aligned'}, mode {mode}, chunk {chunk}"
    assert batch.last_kernel() == "reduced", f"{what}: last_kernel() = {batch.last_kernel()}"
    got = dst.read(what)
    for i, x in enumerate(frames):
        _compare(got[i], _want(reds[i] if reds else rs.frame_reduced(x, ca=ca), x, format, pitch, total), f"{what}, image {i}")
    return batch


# ---- the cases -------------------------------------------------------------------------------------------------------

def cut_edges_and_intervals(layout):
    """324 x 70 at every DRI of the table: one decoder for all, both formats, tight and pitched, aligned and not, host and
    device preprocessing; and a batch of three at every DRI in the three preprocessing modes."""
    dec = ca.Decoder(gpu)
    n = 0
    for ri in DRIS[layout]:
        for format in rs.FORMATS:
            n += 1
            f = ps.sized(layout, 324, 70, ri, standard=n % 2 == 0, seed=n)
            red = rs.frame_reduced(f)
            assert red[3].all() and red[0].shape[1] >= 41
            decoder_case(f, format, pitched=n % 3 == 0, odd=n % 2 == 1, device=n % 4 == 1, red=red, dec=dec)
            decoder_case(f, format, pitched=n % 3 != 0, odd=n % 2 == 0, device=n % 4 != 1, red=red, dec=dec)
            frames = [f, ps.sized(layout, 324, 70, ri, standard=n % 2 == 0, seed=n + 50), ps.sized(layout, 324, 70, ri, standard=n % 2 == 0, seed=n + 90)]
            batch_case(frames, format, pitched=n % 2 == 0, odd=n % 3 == 0, mode=n % 3, chunk=n % 2 * 2)


def many_intervals():
    """640 x 192 4:2:2 at DRI 1: 960 intervals, fifteen waves, beyond one workgroup's."""
    f = ps.sized("422", 640, 192, 1, seed=11)
    assert f.intervals == 960
    red = rs.frame_reduced(f)
    for format in rs.FORMATS:
        decoder_case(f, format, pitched=True, red=red, blocking=False)
        decoder_case(f, format, odd=True, red=red, device=True)
    batch_case([f, f], reds=[red, red], pitched=True, chunk=1)
    batch_case([f, f, f], "rgb_planar", reds=[red] * 3, mode=2)


def undecoded_tail():
    """Nine MCUs at DRI 4 in every sampling: the ninth lies behind the last complete interval and keeps the pre-fill."""
    for layout in ps.SAMPLINGS:
        hs, vs = ps.SAMPLINGS[layout]
        mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
        f = ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3)
        red = rs.frame_reduced(f, ca=ca)
        assert not red[3].all(), "the frame must have MCUs behind its last complete interval"
        for format in rs.FORMATS:
            decoder_case(f, format, pitched=True, red=red)
            want = _want(red, f, format, None, _geometry(f.w, f.h, format, False)[1])
            assert (want == PREFILL).sum() >= (4 if format == "rgba" else 3)


def tiny_frames():
    """8 x 8 and 1 x 1: one pixel."""
    for layout in ps.SAMPLINGS:
        for w, h in ((8, 8), (1, 1)):
            f = ps.sized(layout, w, h, 0, seed=w)
            for format in rs.FORMATS:
                assert _geometry(w, h, format, False)[1] == (4 if format == "rgba" else 3)
                decoder_case(f, format, odd=format == "rgb_planar")
            batch_case([f, f], "rgba")


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


def _file_case(name, j, kw, dec=None):
    red, (w, h, comps, hs, vs) = rs.file_reduced(ca, j, **kw)
    img = ca.ImageData(j, **kw)
    dec = dec or ca.Decoder(gpu)
    for format in rs.FORMATS:
        total = rs.shape(w, h, format)[3]
        dst = Dest(total)
        dec.decode_reduced(img, dst.range, format, blocking=True)
        assert dec.last_kernel() == "reduced", name
        want = rs.destination(red, w, h, hs, vs, format, None, before=np.full(total, PREFILL, dtype=np.uint8))
        _compare(dst.read(name)[0], want, f"{name}: {format}, {kw}")
    return dec


def interval_longer_than_the_window():
    """PIL's 256 x 256 noise without DRI, grayscale and 4:2:2: one lane, global reads beyond the window cap; both entropy modes."""
    for std in (False, True):
        _file_case("noise_256 L", _noise("L"), dict(allow_grayscale=True, standard_entropy=std))
        _file_case("noise_256 RGB 4:2:2", _noise("RGB"), dict(standard_entropy=std))


def coefficient_families():
    """dc_cats, dc_hostile, q1_underflow, dc_wrap, dc_sweep, saturated, gamut, random_dense: every frame of cs.cases() in them
    -- both entropy modes where the family has them, every sampling -- and the grayscale ones, through one decoder."""
    frames = [f for f in cs.cases() if f.family in FAMILIES] + [f for f in gs.cases() if f.family in FAMILIES]
    assert {f.family for f in frames} == set(FAMILIES) and {f.standard for f in frames} == {False, True}
    dec = ca.Decoder(gpu)
    for i, f in enumerate(frames):
        red = rs.frame_reduced(f)
        decoder_case(f, rs.FORMATS[i % 2], pitched=i % 3 == 0, odd=i % 4 == 1, red=red, dec=dec, device=i % 2 == 1)
        if i % 5 == 0:
            batch_case([f], rs.FORMATS[(i + 1) % 2], reds=[red], pitched=True)


def golden_files():
    """Every golden file the decoder accepts, against the expectation."""
    files = ps.golden_files(ca, GOLDEN)
    assert len(files) >= 6
    dec = ca.Decoder(gpu)
    for name, j, kw in files:
        _file_case(name, j, kw, dec)


def identity_with_the_cards_own_rgba():
    """Frames written with DC terms only, every sampling: the reduced RGBA is [::8, ::8] of the decoder's own RGBA read-back
    of the same file.  (The card against itself: no host arithmetic in between.)"""
    dec = ca.Decoder(gpu)
    for f in [cs.dc_sweep(lay) for lay in ("422", "444", "440", "420")] + [cs.gamut()]:
        img = ca.ImageData(f.jpeg(), **f.image_kw())
        dec.decode_blocking(img)
        full = dec.read_texture(f.w, f.h)
        total = rs.shape(f.w, f.h)[3]
        dst = Dest(total)
        dec.decode_reduced(img, dst.range, blocking=True)
        assert dec.last_kernel() == "reduced"
        assert np.array_equal(dec.read_texture(f.w, f.h), full), f"{f.name}: the reduced decode touched the texture"
        got = rs.view(dst.read(f.name)[0], f.w, f.h)
        assert np.array_equal(got, full[::8, ::8]), f"{f.name}: {int((got != full[::8, ::8]).any(axis=2).sum())} pixels differ from the RGBA decode's"


def batches():
    """Three images of one size and different content: chunks of two, the three preprocessing modes, RGBA decodes and packs
    before and after with their results unchanged, both formats one after the other, last_kernel before, between and after."""
    for layout, (w, h, ri) in (("422", (63, 33, 4)), ("420", (47, 31, 3)), ("gray", (23, 17, 1))):
        frames = [ps.sized(layout, w, h, ri, seed=s) for s in (1, 30, 77)]
        reds = [rs.frame_reduced(f) for f in frames]
        rgba = [gs.expectation(f) if layout == "gray" else orc.ImageData(f.jpeg(), **f.image_kw()).decode() for f in frames]
        packed_want = np.stack([np.ascontiguousarray(x[..., :3].transpose(2, 0, 1)) for x in rgba])
        for mode in (0, 1, 2):
            batch = ca.Batch(gpu)
            batch.set_device_preprocess(mode)
            batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in frames])
            batch.set_chunk(2)
            batch.decode()
            batch.wait()
            first = batch.last_kernel()
            assert first != "reduced"
            packed = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack before"
            batch_case(frames, "rgba", reds=reds, batch=batch, mode=mode, chunk=2)
            batch_case(frames, "rgb_planar", odd=True, reds=reds, batch=batch, mode=mode, chunk=2)
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} after the reduced decodes"
            packed.zero_()
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack after the reduced decodes"
            batch.decode()
            batch.wait()
            assert batch.last_kernel() == first
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} decoded again"
            batch_case(frames, "rgba", pitched=True, reds=reds, batch=batch, mode=mode, chunk=2)


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
    total = rs.shape(33, 17)[3]
    assert total == 5 * 4 * 3
    dst = Dest(total * 3, 1)
    addr = dst.range[0]
    dec = ca.Decoder(gpu)
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(total - 1), str(total)):
        dec.decode_reduced(img, (addr, total - 1))
    with Raises(ca.E_INVALID_ARG, "device_dst is NULL"):
        dec.decode_reduced(img, (0, total))
    with Raises(ca.E_INVALID_ARG, "address", "multiple of 4"):
        dec.decode_reduced(img, (addr + 2, total))
    with Raises(ca.E_INVALID_ARG, "pitch 16", "20 bytes"):
        dec.decode_reduced(img, (addr, total * 3), pitch=16)
    with Raises(ca.E_INVALID_ARG, "pitch 22", "multiple of 4"):
        dec.decode_reduced(img, (addr, total * 3), pitch=22)
    with Raises(ca.E_INVALID_ARG, "pitch 24", "planar"):
        dec.decode_reduced(img, (addr, total * 3), "rgb_planar", pitch=24)
    with Raises(ca.E_INVALID_ARG, "format 5"):
        dec.decode_reduced(img, (addr, total * 3), 5)
    assert dec.last_kernel() == "none"
    batch = ca.Batch(gpu)
    with Raises(ca.E_INVALID_ARG, "nothing uploaded"):
        batch.decode_reduced((addr, total * 3))
    batch.upload([img, img, img])
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(3 * total - 1), str(3 * total), "3 image"):
        batch.decode_reduced((addr, 3 * total - 1))
    batch.upload([img, ca.ImageData(ps.sized("422", 33, 9, 0).jpeg())])
    with Raises(ca.E_INVALID_ARG, "not all of one size", "image 1", "33x9", "33x17"):
        batch.decode_reduced((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("440", 33, 17, 0).jpeg(), allow_sampling=True)])
    with Raises(ca.E_INVALID_ARG, "not all of one sampling", "image 1", "4:4:0", "4:2:2"):
        batch.decode_reduced((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("gray", 33, 17, 0).jpeg(), allow_grayscale=True)])
    with Raises(ca.E_INVALID_ARG, "not all of one sampling", "grayscale"):
        batch.decode_reduced((addr, total * 3))
    assert (dst.read("refusals") == PREFILL).all()


WINDOW = "the stalled stream had drained before the consumer was issued: the case did not test the ordering"


def _u8_pack_want(rgba):
    return np.ascontiguousarray(rgba[..., :3].transpose(2, 0, 1))


def _batch_for_ordering(old, total):
    """A batch that has done everything once with the old frames: every buffer has its size."""
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(f.jpeg()) for f in old])
    batch.decode()
    batch.pack_tensor(torch.empty((2, 3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    batch.decode_reduced(Dest(total, 2).range, "rgb_planar")
    batch.wait()
    return batch


def ordering_batch_reduced_behind_a_stalled_decode():
    """stall(A); RGBA decode on A; reduced decode on B; pack of the RGBA outputs on C, with nothing but the library's events
    between them: the pack reads the new frames only if the reduced decode waited for the decode and the pack for the
    reduced decode (it orders itself behind the batch's last stream, B).  The reduced images are the new frames' too."""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    rgba = {id(f): orc.ImageData(f.jpeg()).decode() for f in old + new}
    want_new, want_old = np.stack([_u8_pack_want(rgba[id(f)]) for f in new]), np.stack([_u8_pack_want(rgba[id(f)]) for f in old])
    assert not np.array_equal(want_new, want_old), "the two outcomes this case must tell apart are the same"
    pitch, total = _geometry(48, 32, "rgb_planar", False)
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])   # (the outputs still hold the old frames)
    dst = Dest(total, 2)
    packed = torch.full((2, 3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode(A.cuda_stream)
    batch.decode_reduced(dst.range, "rgb_planar", hip_stream=B.cuda_stream)
    batch.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert batch.last_kernel() == "reduced"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(rs.frame_reduced(f), f, "rgb_planar", pitch, total), f"ordering, batch: reduced image {i}")
    assert np.array_equal(packed.cpu().numpy(), want_new), "the pack on the third stream did not read the decode on the first"


def ordering_batch_decode_behind_a_stalled_reduced():
    """stall(A); reduced decode on A; RGBA decode on B.  The decode on B orders itself behind the batch's last stream: while
    A's stall runs, B has not finished.  (B's state is read first, then A's: if A was still stalled at the second look, the
    first look was inside the stall.)  Then both results are the new frames'."""
    A, B = ss.independent_pair()
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    pitch, total = _geometry(48, 32, "rgba", False)
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])
    dst = Dest(total, 2)
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode_reduced(dst.range, "rgba", hip_stream=A.cuda_stream)
    batch.decode(B.cuda_stream)
    b_done = B.query()
    open_ = ss.window_open(A)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert not b_done, "the RGBA decode on the second stream finished while the reduced decode's stream was stalled"
    assert batch.last_kernel() != "reduced"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(rs.frame_reduced(f), f, "rgba", pitch, total), f"ordering, batch: reduced image {i}")
        assert np.array_equal(batch.read_output(i), orc.ImageData(f.jpeg()).decode()), f"ordering, batch: RGBA {i}"


def ordering_decoder_reduced_behind_a_stalled_decode():
    """stall(A); enqueue(new) on A; decode_reduced(other) on B -- it rewrites the decoder's one set of input buffers, so it
    must not run before the decode on A has read them; a pack of the texture on C.  The texture and the pack are the new
    frame's only if the reduced decode waited for the decode, the reduced image is the other frame's, and a decode on C
    afterwards leaves it alone.  (The window is looked at before the reduced decode is issued: an upload waits on the
    host for the previous one's staging.)"""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    rgba_new, rgba_old = orc.ImageData(new.jpeg()).decode(), orc.ImageData(old.jpeg()).decode()
    assert not np.array_equal(rgba_new, rgba_old)
    pitch, total = _geometry(48, 32, "rgba", False)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dec.pack_tensor(torch.empty((3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    dec.decode_reduced(ca.ImageData(other.jpeg()), Dest(total).range, blocking=True)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dst = Dest(total)
    packed = torch.full((3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    staged_new, staged_other, staged_old = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg()), ca.ImageData(old.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    open_ = ss.window_open(A)
    dec.decode_reduced(staged_other, dst.range, hip_stream=B.cuda_stream)
    assert dec.last_kernel() == "reduced"
    dec.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert np.array_equal(dec.read_texture(48, 32), rgba_new), "the decode on the first stream did not decode its own frame"
    assert np.array_equal(packed.cpu().numpy(), _u8_pack_want(rgba_new)), "the pack on the third stream did not read the decode on the first"
    want = _want(rs.frame_reduced(other), other, "rgba", pitch, total)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the reduced image")
    dec.enqueue(staged_old, Cs.cuda_stream)
    Cs.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dec.read_texture(48, 32), rgba_old)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the reduced image after the next decode")


def ordering_decoder_decode_behind_a_stalled_reduced():
    """stall(A); decode_reduced(other) on A; enqueue(new) on B -- the enqueue rewrites the input buffers the reduced decode
    on A has yet to read.  The reduced image is the other frame's only if the enqueue waited; the texture is the new
    frame's, and last_kernel names an RGBA kernel again."""
    A, B = ss.independent_pair()
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    pitch, total = _geometry(48, 32, "rgb_planar", False)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    rgba_kernel = dec.last_kernel()
    dec.decode_reduced(ca.ImageData(other.jpeg()), Dest(total).range, "rgb_planar", blocking=True)
    dst = Dest(total)
    staged_new, staged_other = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.decode_reduced(staged_other, dst.range, "rgb_planar", hip_stream=A.cuda_stream)
    assert dec.last_kernel() == "reduced"
    open_ = ss.window_open(A)
    dec.enqueue(staged_new, B.cuda_stream)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert dec.last_kernel() == rgba_kernel != "reduced"
    _compare(dst.read("ordering, decoder")[0], _want(rs.frame_reduced(other), other, "rgb_planar", pitch, total), "ordering, decoder: the reduced image")
    assert np.array_equal(dec.read_texture(48, 32), orc.ImageData(new.jpeg()).decode()), "the decode on the second stream did not decode its own frame"


def tables_beyond_the_lds_share():
    """Frames whose Huffman tables outgrow their share of LDS (cs.wide_cases, gs.wide_cases; cs.table_regime): every regime-B
    and regime-C frame of every sampling through the Decoder -- the direct tables staged in part, L2 lookups from global
    memory beyond entry 12288 --, and batches of images of one size whose regimes are A, B and C: planned with the largest
    image's tables while each image stages its own."""
    import wide_emul as we
    for layout in we.SAMPLINGS:
        dec = ca.Decoder(gpu)
        for i, f in enumerate(x for x in we.frames((layout,)) if we.regime(x) != "A"):
            decoder_case(f, rs.FORMATS[i % 2], pitched=i % 3 == 0, odd=i % 4 == 1, red=rs.frame_reduced(f), dec=dec, device=i % 2 == 1, blocking=i % 5 != 0)
        for n, frames in enumerate(we.same_size_batches(layout)):
            batch_case(frames, rs.FORMATS[n % 2], pitched=n == 0, mode=n * 2, chunk=2, reds=[rs.frame_reduced(f) for f in frames])


CASES = {f"cut_edges_and_intervals[{lay}]": (cut_edges_and_intervals, (lay,)) for lay in ("422", "444", "440", "420", "gray")}
CASES.update({fn.__name__: (fn, ()) for fn in (many_intervals, undecoded_tail, tiny_frames, interval_longer_than_the_window, coefficient_families,
                                               golden_files, identity_with_the_cards_own_rgba, batches, refusals_on_the_card, tables_beyond_the_lds_share,
                                               ordering_batch_reduced_behind_a_stalled_decode, ordering_batch_decode_behind_a_stalled_reduced,
                                               ordering_decoder_reduced_behind_a_stalled_decode, ordering_decoder_decode_behind_a_stalled_reduced)})


def main(out_path, only=""):
    global torch, ca, ps, rs, cs, gs, orc, ss, gpu
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
    import reduced_stream as rs
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
