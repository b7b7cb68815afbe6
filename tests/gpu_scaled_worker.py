"""The GPU cases of tests/test_gpu_scaled.py: Decoder.decode_scaled / Batch.decode_scaled into torch memory, every byte
against tests/scaled_stream.py -- the destination between sentinels and over a pre-fill, so that what must not be written
shows.  Run in one process of their own that imports torch before the library (tests/gpu_luma_worker.py: why).

    python tests/gpu_scaled_worker.py RESULTS.json [substring of the case names to run]

Every case runs at denominators 2 and 4 and every such decode asserts last_kernel() == "scaled"; denominator 8 has a case of
its own.  A frame's coefficients are predicted once and serve both scales.  RESULTS.json: case name -> null, or what went
wrong; "wall_s"."""
import io
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ps = rs = cs = gs = orc = ss = sc = gpu = None   # set by main(): torch first (sc: scaled_stream, ss: stream_stall)
GUARD, SENTINEL, PREFILL = 256, 0x5C, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DENS = (2, 4)
# 324 x 70 is 162 x 35 at 1/2 and 81 x 18 at 1/4: the right edge cuts an MCU in every sampling at both scales, the bottom
# edge too except at 1/4 where vs = 1 (tests/test_scaled_emulation.py has the sums).  The DRIs divide the MCU counts
# (189, 105, 369, 205, 369); 0: no DRI, one lane.
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


class Expect:
    """A frame's coefficients, predicted once; its planes at a denominator on demand."""

    def __init__(self, f):
        self.f, self.coef, self.planes = f, sc.frame_coefficients(f, ca=ca), {}

    def at(self, den):
        if den not in self.planes:
            comps, hs, vs = ps.sampling_of(self.f)
            self.planes[den] = sc.scaled_planes(self.coef, den, self.f.dus_per_mcu, hs, vs, self.f.mcus_w, self.f.mcus_h)
        return self.planes[den]


def _geometry(w, h, den, format, pitched):
    ow = -(-w // den)
    pitch = (4 * ow + 15) // 16 * 16 + 16 if pitched and format == "rgba" else None
    mine = sc.shape(w, h, den, format, pitch)
    assert ca.scaled_shape(w, h, den, format, pitch) == mine
    return pitch, mine[3]


def _want(planes, f, den, format, pitch, total):
    comps, hs, vs = ps.sampling_of(f)
    return sc.destination(planes, f.w, f.h, den, hs, vs, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8))


def _compare(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def _shift(format, odd):
    """Bytes behind the 256-byte guard: the rgba destination needs a multiple of 4, the planar one takes any address."""
    return (4 if format == "rgba" else 1) if odd else 0


def decoder_case(x, den, format="rgba", pitched=False, odd=False, device=False, dec=None, blocking=True):
    f = x.f
    pitch, total = _geometry(f.w, f.h, den, format, pitched)
    dec = dec or ca.Decoder(gpu)
    dec.set_device_preprocess(device)
    dst = Dest(total, 1, _shift(format, odd))
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    if blocking:
        dec.decode_scaled(img, dst.range, den, format, pitch, blocking=True)
    else:
        s = torch.cuda.Stream()
        dec.decode_scaled(img, dst.range, den, format, pitch, hip_stream=s.cuda_stream)
        s.synchronize()
    what = (f"{f.name}: Decoder, 1/{den}, {format}, {'pitched' if pitched else 'tight'}, {'odd' if odd else 'aligned'}, "
            f"{'device' if device else 'host'} preprocessing")
    assert dec.last_kernel() == "scaled", f"{what}: last_kernel() = {dec.last_kernel()}"
    _compare(dst.read(what)[0], _want(x.at(den), f, den, format, pitch, total), what)
    return dec


def batch_case(xs, den, format="rgba", pitched=False, odd=False, mode=0, chunk=0, batch=None):
    f = xs[0].f
    pitch, total = _geometry(f.w, f.h, den, format, pitched)
    if batch is None:
        batch = ca.Batch(gpu)
        batch.set_device_preprocess(mode)
        batch.upload([ca.ImageData(x.f.jpeg(), **x.f.image_kw()) for x in xs])
        batch.set_chunk(chunk)
    # (image i lies at i * total: with an rgba destination every image's base is a multiple of 4, since the pitch is)
    dst = Dest(total, len(xs), _shift(format, odd))
    batch.decode_scaled(dst.range, den, format, pitch)
    batch.wait()
    what = f"{f.name} x{len(xs)}: Batch, 1/{den}, {format}, {'pitched' if pitched else 'tight'}, {'odd' if odd else 'aligned'}, mode {mode}, chunk {chunk}"
    assert batch.last_kernel() == "scaled", f"{what}: last_kernel() = {batch.last_kernel()}"
    got = dst.read(what)
    for i, x in enumerate(xs):
        _compare(got[i], _want(x.at(den), x.f, den, format, pitch, total), f"{what}, image {i}")
    return batch


# ---- the cases -------------------------------------------------------------------------------------------------------

def cut_edges_and_intervals(layout):
    """324 x 70 at every DRI of the table, both scales: one decoder for all, both formats, tight and pitched, aligned and
    not, host and device preprocessing; and a batch of three at every DRI in the three preprocessing modes."""
    dec = ca.Decoder(gpu)
    n = 0
    for ri in DRIS[layout]:
        for format in sc.FORMATS:
            n += 1
            xs = [Expect(ps.sized(layout, 324, 70, ri, standard=n % 2 == 0, seed=n + s)) for s in (0, 50, 90)]
            for den in DENS:
                n += 1
                planes = xs[0].at(den)
                assert planes[3].all() and planes[0].shape[1] >= -(-324 // den)
                decoder_case(xs[0], den, format, pitched=n % 3 == 0, odd=n % 2 == 1, device=n % 4 == 1, dec=dec)
                decoder_case(xs[0], den, format, pitched=n % 3 != 0, odd=n % 2 == 0, device=n % 4 != 1, dec=dec)
                batch_case(xs, den, format, pitched=n % 2 == 0, odd=n % 3 == 0, mode=n % 3, chunk=n % 2 * 2)


def many_intervals():
    """640 x 192 4:2:2 at DRI 1: 960 intervals, fifteen waves, beyond one workgroup's."""
    x = Expect(ps.sized("422", 640, 192, 1, seed=11))
    assert x.f.intervals == 960
    for den in DENS:
        for format in sc.FORMATS:
            decoder_case(x, den, format, pitched=True, blocking=False)
            decoder_case(x, den, format, odd=True, device=True)
        batch_case([x, x], den, pitched=True, chunk=1)
        batch_case([x, x, x], den, "rgb_planar", mode=2)


def undecoded_tail():
    """Nine MCUs at DRI 4 in every sampling: the ninth lies behind the last complete interval and keeps the pre-fill."""
    for layout in ps.SAMPLINGS:
        hs, vs = ps.SAMPLINGS[layout]
        mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
        x = Expect(ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3))
        for den in DENS:
            assert not x.at(den)[3].all(), "the frame must have MCUs behind its last complete interval"
            for format in sc.FORMATS:
                decoder_case(x, den, format, pitched=True)
                want = _want(x.at(den), x.f, den, format, None, _geometry(x.f.w, x.f.h, den, format, False)[1])
                assert (want == PREFILL).sum() >= (4 if format == "rgba" else 3)


def tiny_frames():
    """8 x 8 (N x N pixels) and 1 x 1 (one pixel of an MCU's N hs x N vs)."""
    for layout in ps.SAMPLINGS:
        for w, h in ((8, 8), (1, 1)):
            x = Expect(ps.sized(layout, w, h, 0, seed=w))
            for den in DENS:
                side = -(-w // den)
                for format in sc.FORMATS:
                    assert _geometry(w, h, den, format, False)[1] == (4 if format == "rgba" else 3) * side * side
                    decoder_case(x, den, format, odd=format == "rgb_planar")
                batch_case([x, x], den, "rgba")


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
    coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), _ = rs.file_coefficients(ca, j, **kw)
    img = ca.ImageData(j, **kw)
    dec = dec or ca.Decoder(gpu)
    for den in DENS:
        planes = sc.scaled_planes(coef, den, dpm, hs, vs, mcus_w, mcus_h)
        for format in sc.FORMATS:
            total = sc.shape(w, h, den, format)[3]
            dst = Dest(total)
            dec.decode_scaled(img, dst.range, den, format, blocking=True)
            assert dec.last_kernel() == "scaled", name
            want = sc.destination(planes, w, h, den, hs, vs, format, None, before=np.full(total, PREFILL, dtype=np.uint8))
            _compare(dst.read(name)[0], want, f"{name}: 1/{den}, {format}, {kw}")
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
        x = Expect(f)
        for den in DENS:
            i += 1
            decoder_case(x, den, sc.FORMATS[i % 2], pitched=i % 3 == 0, odd=i % 4 == 1, dec=dec, device=i % 2 == 1)
            if i % 5 == 0:
                batch_case([x], den, sc.FORMATS[(i + 1) % 2], pitched=True)


def golden_files():
    """Every golden file the decoder accepts, against the expectation."""
    files = ps.golden_files(ca, GOLDEN)
    assert len(files) >= 6
    dec = ca.Decoder(gpu)
    for name, j, kw in files:
        _file_case(name, j, kw, dec)


def dc_only_identity_with_the_cards_own_reduced():
    """Frames written with DC terms only, every sampling and grayscale: every N x N block of the scaled decode is the pixel
    of the card's own decode_reduced of the same file.  (The card against itself: no host arithmetic in between.)"""
    dec = ca.Decoder(gpu)
    frames = [cs.dc_sweep(lay) for lay in ("422", "444", "440", "420")] + [cs.gamut()] + [f for f in gs.cases() if f.family == "dc_sweep"][:1]
    assert len(frames) == 6
    for f in frames:
        coef = cs.predict(f)
        assert np.array_equal(rs.zero_ac(coef), coef), f"{f.name}: not a DC-only frame"
        img = ca.ImageData(f.jpeg(), **f.image_kw())
        total = rs.shape(f.w, f.h)[3]
        red = Dest(total)
        dec.decode_reduced(img, red.range, blocking=True)
        assert dec.last_kernel() == "reduced"
        small = rs.view(red.read(f.name)[0], f.w, f.h)
        for den in DENS:
            n = 8 // den
            dst = Dest(sc.shape(f.w, f.h, den)[3])
            dec.decode_scaled(img, dst.range, den, blocking=True)
            assert dec.last_kernel() == "scaled"
            got = sc.view(dst.read(f.name)[0], f.w, f.h, den)
            want = np.repeat(np.repeat(small, n, axis=0), n, axis=1)[:got.shape[0], :got.shape[1]]
            assert np.array_equal(got, want), f"{f.name}: 1/{den}: {int((got != want).any(axis=2).sum())} pixels differ from decode_reduced's, repeated"


def denominator_8_is_the_reduced_decode():
    """decode_scaled(.., 8, ..) writes decode_reduced's bytes, pre-fill and all, and says "reduced": decoders and batches."""
    dec = ca.Decoder(gpu)
    for layout, ri in (("422", 3), ("420", 5), ("444", 41), ("440", 5), ("gray", 3)):
        frames = [ps.sized(layout, 324, 70, ri, seed=s) for s in (4, 44)]
        tail = ps.sized("422", 48, 23, 4, seed=2, short=3) if layout == "422" else None   # (nine MCUs, the ninth undecoded)
        for format in sc.FORMATS:
            for pitched in (False, True):
                if pitched and format != "rgba":
                    continue
                for f in frames[:1] + ([tail] if tail else []):
                    pitch, total = _geometry(f.w, f.h, 8, format, pitched)
                    assert rs.shape(f.w, f.h, format, pitch)[3] == total
                    img = ca.ImageData(f.jpeg(), **f.image_kw())
                    a, b = Dest(total, 1, _shift(format, True)), Dest(total, 1, _shift(format, True))
                    dec.decode_reduced(img, a.range, format, pitch, blocking=True)
                    dec.decode_scaled(img, b.range, 8, format, pitch, blocking=True)
                    assert dec.last_kernel() == "reduced", dec.last_kernel()
                    want = a.read(f.name)[0]
                    assert (want != PREFILL).any()
                    _compare(b.read(f.name)[0], want, f"{f.name}: Decoder, 1/8, {format}, pitch {pitch}")
                pitch, total = _geometry(324, 70, 8, format, pitched)
                batch = ca.Batch(gpu)
                batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in frames])
                a, b = Dest(total, 2), Dest(total, 2)
                batch.decode_reduced(a.range, format, pitch)
                batch.decode_scaled(b.range, 8, format, pitch)
                batch.wait()
                assert batch.last_kernel() == "reduced", batch.last_kernel()
                _compare(b.read("batch").ravel(), a.read("batch").ravel(), f"{layout}: Batch, 1/8, {format}, pitch {pitch}")


def batches():
    """Three images of one size and different content: chunks of two, the three preprocessing modes, RGBA decodes and packs
    before and after with their results unchanged, both formats and both scales one after the other, last_kernel before,
    between and after."""
    for layout, (w, h, ri) in (("422", (63, 33, 4)), ("420", (47, 31, 3)), ("gray", (23, 17, 1))):
        frames = [ps.sized(layout, w, h, ri, seed=s) for s in (1, 30, 77)]
        xs = [Expect(f) for f in frames]
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
            assert first not in ("scaled", "reduced")
            packed = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack before"
            batch_case(xs, 2, "rgba", batch=batch, mode=mode, chunk=2)
            batch_case(xs, 4, "rgb_planar", odd=True, batch=batch, mode=mode, chunk=2)
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} after the scaled decodes"
            packed.zero_()
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack after the scaled decodes"
            batch.decode()
            batch.wait()
            assert batch.last_kernel() == first
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} decoded again"
            batch_case(xs, 4, "rgba", pitched=True, batch=batch, mode=mode, chunk=2)
            batch_case(xs, 2, "rgb_planar", batch=batch, mode=mode, chunk=2)


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
    dec = ca.Decoder(gpu)
    batch = ca.Batch(gpu)
    with Raises(ca.E_INVALID_ARG, "nothing uploaded"):
        batch.decode_scaled((256, 1 << 20), 4)
    for den in DENS + (8,):
        ow, oh, _, total = sc.shape(33, 17, den)
        dst = Dest(total * 3, 1)
        addr = dst.range[0]
        with Raises(ca.E_INVALID_ARG, "dst_bytes", str(total - 1), str(total)):
            dec.decode_scaled(img, (addr, total - 1), den)
        with Raises(ca.E_INVALID_ARG, "device_dst is NULL"):
            dec.decode_scaled(img, (0, total), den)
        with Raises(ca.E_INVALID_ARG, "address", "multiple of 4"):
            dec.decode_scaled(img, (addr + 2, total), den)
        with Raises(ca.E_INVALID_ARG, f"pitch {4 * ow - 4}", f"{4 * ow} bytes"):
            dec.decode_scaled(img, (addr, total * 3), den, pitch=4 * ow - 4)
        with Raises(ca.E_INVALID_ARG, f"pitch {4 * ow + 2}", "multiple of 4"):
            dec.decode_scaled(img, (addr, total * 3), den, pitch=4 * ow + 2)
        with Raises(ca.E_INVALID_ARG, f"pitch {4 * ow + 4}", "planar"):
            dec.decode_scaled(img, (addr, total * 3), den, "rgb_planar", pitch=4 * ow + 4)
        with Raises(ca.E_INVALID_ARG, "format 5"):
            dec.decode_scaled(img, (addr, total * 3), den, 5)
        assert dec.last_kernel() == "none"
        batch.upload([img, img, img])
        with Raises(ca.E_INVALID_ARG, "dst_bytes", str(3 * total - 1), str(3 * total), "3 image"):
            batch.decode_scaled((addr, 3 * total - 1), den)
        batch.upload([img, ca.ImageData(ps.sized("422", 33, 9, 0).jpeg())])
        with Raises(ca.E_INVALID_ARG, "scaled", "not all of one size", "image 1", "33x9", "33x17"):
            batch.decode_scaled((addr, total * 3), den)
        batch.upload([img, ca.ImageData(ps.sized("440", 33, 17, 0).jpeg(), allow_sampling=True)])
        with Raises(ca.E_INVALID_ARG, "not all of one sampling", "image 1", "4:4:0", "4:2:2"):
            batch.decode_scaled((addr, total * 3), den)
        batch.upload([img, ca.ImageData(ps.sized("gray", 33, 17, 0).jpeg(), allow_grayscale=True)])
        with Raises(ca.E_INVALID_ARG, "not all of one sampling", "grayscale"):
            batch.decode_scaled((addr, total * 3), den)
        assert batch.last_kernel() == "none"
        assert (dst.read("refusals") == PREFILL).all()
    dst = Dest(1 << 16)
    for den in (0, 1, 3, 16):
        with Raises(ca.E_INVALID_ARG, f"denominator {den}", "2, 4, 8"):
            dec.decode_scaled(img, dst.range, den)
        batch.upload([img])
        with Raises(ca.E_INVALID_ARG, f"denominator {den}", "2, 4, 8"):
            batch.decode_scaled(dst.range, den)
    assert dec.last_kernel() == "none" and (dst.read("refusals") == PREFILL).all()


WINDOW = "the stalled stream had drained before the consumer was issued: the case did not test the ordering"


def _u8_pack_want(rgba):
    return np.ascontiguousarray(rgba[..., :3].transpose(2, 0, 1))


def _batch_for_ordering(old, den, total):
    """A batch that has done everything once with the old frames: every buffer has its size."""
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(f.jpeg()) for f in old])
    batch.decode()
    batch.pack_tensor(torch.empty((2, 3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    batch.decode_scaled(Dest(total, 2).range, den, "rgb_planar")
    batch.wait()
    return batch


def ordering_batch_scaled_behind_a_stalled_decode(den):
    """stall(A); RGBA decode on A; scaled decode on B; pack of the RGBA outputs on C, with nothing but the library's events
    between them: the pack reads the new frames only if the scaled decode waited for the decode and the pack for the
    scaled decode (it orders itself behind the batch's last stream, B).  The scaled images are the new frames' too."""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    rgba = {id(f): orc.ImageData(f.jpeg()).decode() for f in old + new}
    want_new, want_old = np.stack([_u8_pack_want(rgba[id(f)]) for f in new]), np.stack([_u8_pack_want(rgba[id(f)]) for f in old])
    assert not np.array_equal(want_new, want_old), "the two outcomes this case must tell apart are the same"
    pitch, total = _geometry(48, 32, den, "rgb_planar", False)
    batch = _batch_for_ordering(old, den, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])   # (the outputs still hold the old frames)
    dst = Dest(total, 2)
    packed = torch.full((2, 3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode(A.cuda_stream)
    batch.decode_scaled(dst.range, den, "rgb_planar", hip_stream=B.cuda_stream)
    batch.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert batch.last_kernel() == "scaled"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(Expect(f).at(den), f, den, "rgb_planar", pitch, total), f"ordering, batch: scaled image {i}")
    assert np.array_equal(packed.cpu().numpy(), want_new), "the pack on the third stream did not read the decode on the first"


def ordering_batch_decode_behind_a_stalled_scaled(den):
    """stall(A); scaled decode on A; RGBA decode on B.  The decode on B orders itself behind the batch's last stream: while
    A's stall runs, B has not finished.  (B's state is read first, then A's: if A was still stalled at the second look, the
    first look was inside the stall.)  Then both results are the new frames'."""
    A, B = ss.independent_pair()
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    pitch, total = _geometry(48, 32, den, "rgba", False)
    batch = _batch_for_ordering(old, den, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])
    dst = Dest(total, 2)
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode_scaled(dst.range, den, "rgba", hip_stream=A.cuda_stream)
    batch.decode(B.cuda_stream)
    b_done = B.query()
    open_ = ss.window_open(A)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert not b_done, "the RGBA decode on the second stream finished while the scaled decode's stream was stalled"
    assert batch.last_kernel() != "scaled"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(Expect(f).at(den), f, den, "rgba", pitch, total), f"ordering, batch: scaled image {i}")
        assert np.array_equal(batch.read_output(i), orc.ImageData(f.jpeg()).decode()), f"ordering, batch: RGBA {i}"


def ordering_decoder_scaled_behind_a_stalled_decode(den):
    """stall(A); enqueue(new) on A; decode_scaled(other) on B -- it rewrites the decoder's one set of input buffers, so it
    must not run before the decode on A has read them; a pack of the texture on C.  The texture and the pack are the new
    frame's only if the scaled decode waited for the decode, the scaled image is the other frame's, and a decode on C
    afterwards leaves it alone.  (The window is looked at before the scaled decode is issued: an upload waits on the
    host for the previous one's staging.)"""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    rgba_new, rgba_old = orc.ImageData(new.jpeg()).decode(), orc.ImageData(old.jpeg()).decode()
    assert not np.array_equal(rgba_new, rgba_old)
    pitch, total = _geometry(48, 32, den, "rgba", False)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dec.pack_tensor(torch.empty((3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    dec.decode_scaled(ca.ImageData(other.jpeg()), Dest(total).range, den, blocking=True)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dst = Dest(total)
    packed = torch.full((3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    staged_new, staged_other, staged_old = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg()), ca.ImageData(old.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    open_ = ss.window_open(A)
    dec.decode_scaled(staged_other, dst.range, den, hip_stream=B.cuda_stream)
    assert dec.last_kernel() == "scaled"
    dec.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert np.array_equal(dec.read_texture(48, 32), rgba_new), "the decode on the first stream did not decode its own frame"
    assert np.array_equal(packed.cpu().numpy(), _u8_pack_want(rgba_new)), "the pack on the third stream did not read the decode on the first"
    want = _want(Expect(other).at(den), other, den, "rgba", pitch, total)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the scaled image")
    dec.enqueue(staged_old, Cs.cuda_stream)
    Cs.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dec.read_texture(48, 32), rgba_old)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the scaled image after the next decode")


def ordering_decoder_decode_behind_a_stalled_scaled(den):
    """stall(A); decode_scaled(other) on A; enqueue(new) on B -- the enqueue rewrites the input buffers the scaled decode
    on A has yet to read.  The scaled image is the other frame's only if the enqueue waited; the texture is the new
    frame's, and last_kernel names an RGBA kernel again."""
    A, B = ss.independent_pair()
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    pitch, total = _geometry(48, 32, den, "rgb_planar", False)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    rgba_kernel = dec.last_kernel()
    dec.decode_scaled(ca.ImageData(other.jpeg()), Dest(total).range, den, "rgb_planar", blocking=True)
    dst = Dest(total)
    staged_new, staged_other = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.decode_scaled(staged_other, dst.range, den, "rgb_planar", hip_stream=A.cuda_stream)
    assert dec.last_kernel() == "scaled"
    open_ = ss.window_open(A)
    dec.enqueue(staged_new, B.cuda_stream)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert dec.last_kernel() == rgba_kernel != "scaled"
    _compare(dst.read("ordering, decoder")[0], _want(Expect(other).at(den), other, den, "rgb_planar", pitch, total), "ordering, decoder: the scaled image")
    assert np.array_equal(dec.read_texture(48, 32), orc.ImageData(new.jpeg()).decode()), "the decode on the second stream did not decode its own frame"


def tables_beyond_the_lds_share():
    """Frames whose Huffman tables outgrow their share of LDS (cs.wide_cases, gs.wide_cases; cs.table_regime): every regime-B
    and regime-C frame of every sampling through the Decoder -- the direct tables staged in part, L2 lookups from global
    memory beyond entry 12288 --, and batches of images of one size whose regimes are A, B and C: planned with the largest
    image's tables while each image stages its own."""
    import wide_emul as we
    for layout in we.SAMPLINGS:
        dec = ca.Decoder(gpu)
        n = 0   # (counts the decodes: format, pitch, alignment, preprocessing and blocking vary with it)
        for f in (x for x in we.frames((layout,)) if we.regime(x) != "A"):
            x = Expect(f)
            for den in DENS:
                n += 1
                decoder_case(x, den, sc.FORMATS[n % 2], pitched=n % 3 == 0, odd=n % 4 == 1, dec=dec, device=n % 2 == 1, blocking=n % 5 != 0)
        for n, frames in enumerate(we.same_size_batches(layout)):
            xs = [Expect(f) for f in frames]
            for den in DENS:
                batch_case(xs, den, sc.FORMATS[(n + den // 4) % 2], pitched=n == 0, mode=(n + den // 2) % 3, chunk=2)


CASES = {f"cut_edges_and_intervals[{lay}]": (cut_edges_and_intervals, (lay,)) for lay in ("422", "444", "440", "420", "gray")}
CASES.update({fn.__name__: (fn, ()) for fn in (many_intervals, undecoded_tail, tiny_frames, interval_longer_than_the_window, coefficient_families,
                                               golden_files, dc_only_identity_with_the_cards_own_reduced, denominator_8_is_the_reduced_decode,
                                               batches, refusals_on_the_card, tables_beyond_the_lds_share)})
CASES.update({f"{fn.__name__}[1/{den}]": (fn, (den,)) for fn in (ordering_batch_scaled_behind_a_stalled_decode, ordering_batch_decode_behind_a_stalled_scaled,
                                                                  ordering_decoder_scaled_behind_a_stalled_decode,
                                                                  ordering_decoder_decode_behind_a_stalled_scaled) for den in DENS})


def main(out_path, only=""):
    global torch, ca, ps, rs, cs, gs, orc, ss, sc, gpu
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
    import scaled_stream as sc
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
