"""The GPU cases of tests/test_gpu_levels.py: Decoder.decode_levels / Batch.decode_levels into torch memory, every byte
against tests/levels_stream.py -- the destination between sentinels and over a pre-fill, so that what must not be written
shows.  Run in one process of their own that imports torch before the library (tests/gpu_luma_worker.py: why).

    python tests/gpu_levels_worker.py RESULTS.json [substring of the case names to run]

Every decode asserts last_kernel() == "levels".  RESULTS.json: case name -> null, or what went wrong; "wall_s"."""
import io
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ps = ls = rs = cs = gs = orc = ss = gpu = None   # set by main(): torch first
GUARD, SENTINEL, PREFILL = 256, 0x5C, 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("random_dense", "positions", "run_size0", "ac_sizes", "dc_cats", "dc_hostile", "dc_wrap", "q1_underflow")
LAYOUTS = ("422", "444", "440", "420", "gray")


class Dest:
    """n images' worth of destination inside one torch block: sentinels, `shift` bytes, the images over a pre-fill, sentinels.
    (torch's allocations begin on 256-byte boundaries and the guard is 256 bytes: shift 0 is an aligned destination.)"""

    def __init__(self, total, n=1, shift=0):
        self.total, self.n, self.shift = total, n, shift
        self.block = torch.full((GUARD + shift + total * n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.block[GUARD + shift:GUARD + shift + total * n] = PREFILL
        assert self.block.data_ptr() % 16 == 0
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


def _layout_of(f):
    return "gray" if isinstance(f, gs.GrayFrame) else f.layout


def _total(f):
    mw, mh, comps, hs, vs = ls.frame_geometry(f)
    mine = ls.shape(f.w, f.h, comps, hs, vs)
    for order in ls.ORDERS:
        assert ca.levels_shape(f.w, f.h, (hs, vs), comps, order) == mine
    return mine[1]


def _want(levels, f, order, total):
    return ls.destination(levels, *ls.frame_geometry(f), order=order, before=np.full(total, PREFILL, dtype=np.uint8))


def _compare(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def decoder_case(f, order="zigzag", device=False, levels=None, dec=None, blocking=True):
    levels = levels if levels is not None else ls.any_frame_levels(f, ca)
    total = _total(f)
    dec = dec or ca.Decoder(gpu)
    dec.set_device_preprocess(device)
    dst = Dest(total)
    img = ca.ImageData(f.jpeg(), **f.image_kw())
    if blocking:
        dec.decode_levels(img, dst.range, order, blocking=True)
    else:
        s = torch.cuda.Stream()
        dec.decode_levels(img, dst.range, order, hip_stream=s.cuda_stream)
        s.synchronize()
    what = f"{f.name}: Decoder, {order}, {'device' if device else 'host'} preprocessing"
    assert dec.last_kernel() == "levels", f"{what}: last_kernel() = {dec.last_kernel()}"
    _compare(dst.read(what)[0], _want(levels, f, order, total), what)
    return dec


def batch_case(frames, order="zigzag", mode=0, chunk=0, levels=None, batch=None):
    f = frames[0]
    total = _total(f)
    if batch is None:
        batch = ca.Batch(gpu)
        batch.set_device_preprocess(mode)
        batch.upload([ca.ImageData(x.jpeg(), **x.image_kw()) for x in frames])
        batch.set_chunk(chunk)
    dst = Dest(total, len(frames))   # (image i lies at i * total: a multiple of 128)
    batch.decode_levels(dst.range, order)
    batch.wait()
    what = f"{f.name} x{len(frames)}: Batch, {order}, mode {mode}, chunk {chunk}"
    assert batch.last_kernel() == "levels", f"{what}: last_kernel() = {batch.last_kernel()}"
    got = dst.read(what)
    for i, x in enumerate(frames):
        _compare(got[i], _want(levels[i] if levels else ls.any_frame_levels(x, ca), x, order, total), f"{what}, image {i}")
    return batch


# ---- the cases -------------------------------------------------------------------------------------------------------

def _family_frames(layout):
    """Every family's frames in the layout: all of cs.cases() there; grayscale: the first of each family and entropy mode."""
    if layout != "gray":
        return [f for f in cs.cases() if f.layout == layout and f.family in FAMILIES]
    seen, out = set(), []
    for f in gs.cases():
        if f.family in FAMILIES and (f.family, f.standard) not in seen:
            seen.add((f.family, f.standard))
            out.append(f)
    return out


def coefficient_families(layout):
    """random_dense, positions, run_size0, ac_sizes, dc_cats, dc_hostile, dc_wrap, q1_underflow in the layout, both orders,
    host and device preprocessing, through one decoder and now and then a batch; 4:2:2 has the families in both entropy modes,
    and every layout has levels the writer chose in positions 32..63."""
    frames = _family_frames(layout)
    assert {f.family for f in frames} == set(FAMILIES), sorted(set(FAMILIES) - {f.family for f in frames})
    if layout == "422":
        assert {f.standard for f in frames} == {False, True}
    dec, beyond = ca.Decoder(gpu), False
    for i, f in enumerate(frames):
        levels = ls.frame_levels(f)
        beyond = beyond or bool(levels[:, 32:].any())
        for k, order in enumerate(ls.ORDERS):
            decoder_case(f, order, device=(i + k) % 2 == 1, levels=levels, dec=dec, blocking=(i + k) % 3 != 0)
        if i % 4 == 0:
            batch_case([f, f], ls.ORDERS[i // 4 % 2], levels=[levels, levels], mode=i // 4 % 3, chunk=i // 4 % 2)
    assert beyond, f"{layout}: no frame with chosen levels in 32..63"


def standard_entropy_in_every_layout():
    """The `positions` family written for COMPEG_PARSE_STANDARD_ENTROPY (a ZRL advances 16) in every sampling, and grayscale."""
    for lay in ("444", "440", "420"):
        f = cs.positions("short", True, lay)
        assert f.standard
        for order in ls.ORDERS:
            decoder_case(f, order)
    g = ls.gray(cs.positions("short", True, "444"))
    for order in ls.ORDERS:
        decoder_case(g, order, device=True)


def tiny_and_one_lane():
    """A frame of one MCU, and 324 x 70 without DRI (one lane) in every sampling."""
    for layout in LAYOUTS:
        f = ps.sized(layout, 1, 1, 0, seed=4)
        assert f.mcus == 1
        for order in ls.ORDERS:
            decoder_case(f, order)
        batch_case([f, f], "natural")
        g = ps.sized(layout, 324, 70, 0, seed=9)
        assert g.intervals == 1
        decoder_case(g, "natural", device=True)
        decoder_case(g, "zigzag")


def interval_counts():
    """65 intervals: a second wave with one lane in use; 1030 intervals: seventeen waves, more than a workgroup holds, alone
    and as a batch of 256 images (workgroups of several waves, two and more an image)."""
    for layout, (w, h) in (("422", (1040, 8)), ("420", (1040, 16)), ("gray", (520, 8))):
        f = ps.sized(layout, w, h, 1, seed=6)
        assert f.intervals == 65
        for order in ls.ORDERS:
            decoder_case(f, order, blocking=False)
    f = ps.sized("422", 1648, 80, 1, seed=11)
    assert f.intervals == 1030
    levels = ls.frame_levels(f)
    decoder_case(f, "zigzag", levels=levels)
    decoder_case(f, "natural", levels=levels, device=True)
    batch_case([f, f, f], "natural", levels=[levels] * 3, chunk=2)
    g = [ps.sized("gray", 824, 80, 1, seed=s) for s in (1, 2, 3)]
    assert g[0].intervals == 1030
    lv = [ls.frame_levels(x) for x in g]
    batch_case([g[i % 3] for i in range(256)], "zigzag", levels=[lv[i % 3] for i in range(256)], mode=2)


def undecoded_tail():
    """Nine MCUs at DRI 4 in every sampling: the ninth lies behind the last complete interval and keeps the pre-fill."""
    for layout in LAYOUTS:
        hs, vs = ps.SAMPLINGS[layout]
        mw, mh = 8 * hs, 8 * (vs if layout != "gray" else 1)
        f = ps.sized(layout, 3 * mw, 3 * mh - 1, 4, seed=2, short=3)
        levels = ls.any_frame_levels(f, ca)
        want = _want(levels, f, "zigzag", _total(f))
        assert (want.reshape(-1, 128) == PREFILL).all(axis=1).sum() == f.dus_per_mcu, "one MCU's blocks keep the pre-fill"
        for order in ls.ORDERS:
            decoder_case(f, order, levels=levels)
        batch_case([f, f], "zigzag", levels=[levels, levels], mode=1)


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


def _file_case(name, j, kw, dec=None, batch=False):
    """A real encoder's file: wrap32(level x q) at positions 0..31 against the oracle's entropy pass, block by block; the
    blocks of undecoded MCUs keep the pre-fill."""
    coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), _ = rs.file_coefficients(ca, j, **kw)
    img = ca.ImageData(j, **kw)
    dec = dec or ca.Decoder(gpu)
    total = ca.levels_shape(w, h, (hs, vs), comps)[1]
    want = ls.rasters(coef, mcus_w, mcus_h, comps, hs, vs)
    for order in ls.ORDERS:
        dst = Dest(total)
        if batch:
            b = ca.Batch(gpu)
            b.upload([img])
            b.decode_levels(dst.range, order)
            b.wait()
            assert b.last_kernel() == "levels", name
            qs = [b.quant_table(0, c) for c in range(comps)]
        else:
            dec.decode_levels(img, dst.range, order, blocking=True)
            assert dec.last_kernel() == "levels", name
            qs = [img.quant_table(c) for c in range(comps)]
        got = ls.views(dst.read(name)[0], w, h, comps, hs, vs)
        for c in range(comps):
            grid, mask = want[c]
            deq = ls.dequantised_low(got[c], qs[c], order)
            assert np.array_equal(deq[mask], grid[mask][:, :32]), f"{name}: {order}, component {c}, {kw}"
            assert (got[c][~mask].view(np.uint8) == PREFILL).all(), f"{name}: {order}, component {c}: an undecoded MCU's block was written"
    return dec


def interval_longer_than_the_window():
    """One interval longer than the window cap (one lane, global reads beyond it): cs.random_strip, whose 64 positions the
    writer chose, and PIL's 256 x 256 noise without DRI, grayscale and 4:2:2, against the oracle; both entropy modes."""
    f = cs.random_strip()
    assert f.intervals == 1 and len(gs.file_scan(f.jpeg())) > 6144 * 4
    levels = ls.frame_levels(f)
    assert levels[:, 32:].any()
    for order in ls.ORDERS:
        decoder_case(f, order, levels=levels)
    for std in (False, True):
        _file_case("noise_256 L", _noise("L"), dict(allow_grayscale=True, standard_entropy=std))
        _file_case("noise_256 RGB 4:2:2", _noise("RGB"), dict(standard_entropy=std))


def golden_files():
    """Every golden file the decoder accepts (mjpeg.jpg among them), positions 0..31 through the quantiser against the oracle."""
    files = ps.golden_files(ca, GOLDEN)
    assert len(files) >= 6 and any(name.endswith("mjpeg.jpg") for name, _, _ in files)
    dec = ca.Decoder(gpu)
    for i, (name, j, kw) in enumerate(files):
        _file_case(name, j, kw, dec, batch=i % 3 == 2)


def batches():
    """Three images of one size and different content: chunks of two, the three preprocessing modes, image i at i x
    total_bytes, RGBA decodes and packs before and after with their results unchanged, both orders one after the other,
    last_kernel before, between and after, quant_table on the batch."""
    for layout, (w, h, ri) in (("422", (63, 33, 4)), ("420", (47, 31, 3)), ("gray", (23, 17, 1))):
        frames = [ps.sized(layout, w, h, ri, seed=s) for s in (1, 30, 77)]
        levels = [ls.frame_levels(f) for f in frames]
        rgba = [gs.expectation(f) if layout == "gray" else orc.ImageData(f.jpeg(), **f.image_kw()).decode() for f in frames]
        packed_want = np.stack([np.ascontiguousarray(x[..., :3].transpose(2, 0, 1)) for x in rgba])
        comps = ps.sampling_of(frames[0])[0]
        for mode in (0, 1, 2):
            batch = ca.Batch(gpu)
            batch.set_device_preprocess(mode)
            batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in frames])
            batch.set_chunk(2)
            batch.decode()
            batch.wait()
            first = batch.last_kernel()
            assert first != "levels"
            packed = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack before"
            batch_case(frames, "zigzag", levels=levels, batch=batch, mode=mode, chunk=2)
            batch_case(frames, "natural", levels=levels, batch=batch, mode=mode, chunk=2)
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} after the levels decodes"
            packed.zero_()
            batch.pack_tensor(packed, dtype="u8")
            batch.wait()
            assert np.array_equal(packed.cpu().numpy(), packed_want), f"{layout} mode {mode}: pack after the levels decodes"
            batch.decode()
            batch.wait()
            assert batch.last_kernel() == first
            for i in range(3):
                assert np.array_equal(batch.read_output(i), rgba[i]), f"{layout} mode {mode}: RGBA {i} decoded again"
            batch_case(frames, "zigzag", levels=levels, batch=batch, mode=mode, chunk=2)
            for i, f in enumerate(frames):
                for c in range(comps):
                    q = f.qtable(f.sel[c][2])
                    assert np.array_equal(batch.quant_table(i, c), q) and np.array_equal(batch.quant_table(i, c, "natural"), q[cs.ZIGZAG])
            with Raises(ca.E_INVALID_ARG, "image 3", "3 images"):
                batch.quant_table(3, 0)
            with Raises(ca.E_INVALID_ARG, f"component {comps}"):
                batch.quant_table(0, comps)


def decoder_state_is_untouched():
    """An RGBA decode and a pack before and after a levels decode of another frame: the texture, its extent and the pack's
    bytes are the RGBA decode's."""
    a, b = ps.sized("422", 48, 32, 4, seed=3), ps.sized("422", 64, 16, 2, seed=60)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(a.jpeg()))
    kernel = dec.last_kernel()
    want = orc.ImageData(a.jpeg()).decode()
    packed = torch.zeros((3, 32, 48), dtype=torch.uint8, device="cuda")
    dec.pack_tensor(packed, dtype="u8")
    torch.cuda.synchronize()
    before = packed.cpu().numpy().copy()
    assert np.array_equal(before, np.ascontiguousarray(want[..., :3].transpose(2, 0, 1)))
    decoder_case(b, "natural", dec=dec)
    assert np.array_equal(dec.read_texture(48, 32), want), "the levels decode touched the texture"
    packed.zero_()
    dec.pack_tensor(packed, dtype="u8")
    torch.cuda.synchronize()
    assert np.array_equal(packed.cpu().numpy(), before), "the pack behind a levels decode reads something else"
    dec.decode_blocking(ca.ImageData(a.jpeg()))
    assert dec.last_kernel() == kernel != "levels"


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
    total = ls.shape(33, 17)[1]
    assert total == (6 * 3 + 2 * 3 * 3) * 128
    dst = Dest(total * 3, 1)
    addr = dst.range[0]
    dec = ca.Decoder(gpu)
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(total - 1), str(total)):
        dec.decode_levels(img, (addr, total - 1))
    with Raises(ca.E_INVALID_ARG, "device_dst is NULL"):
        dec.decode_levels(img, (0, total))
    for off in (2, 8, 4, 1):
        with Raises(ca.E_INVALID_ARG, "address", "multiple of 16"):
            dec.decode_levels(img, (addr + off, total))
    with Raises(ca.E_INVALID_ARG, "order 5"):
        dec.decode_levels(img, (addr, total), 5)
    assert dec.last_kernel() == "none"
    batch = ca.Batch(gpu)
    with Raises(ca.E_INVALID_ARG, "nothing uploaded"):
        batch.decode_levels((addr, total * 3))
    batch.upload([img, img, img])
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(3 * total - 1), str(3 * total), "3 image"):
        batch.decode_levels((addr, 3 * total - 1))
    with Raises(ca.E_INVALID_ARG, "address", "multiple of 16"):
        batch.decode_levels((addr + 8, 3 * total - 8))
    batch.upload([img, ca.ImageData(ps.sized("422", 33, 9, 0).jpeg())])
    with Raises(ca.E_INVALID_ARG, "levels", "not all of one size", "image 1", "33x9", "33x17"):
        batch.decode_levels((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("440", 33, 17, 0).jpeg(), allow_sampling=True)])
    with Raises(ca.E_INVALID_ARG, "levels", "not all of one sampling", "image 1", "4:4:0", "4:2:2"):
        batch.decode_levels((addr, total * 3))
    batch.upload([img, ca.ImageData(ps.sized("gray", 33, 17, 0).jpeg(), allow_grayscale=True)])
    with Raises(ca.E_INVALID_ARG, "not all of one sampling", "grayscale"):
        batch.decode_levels((addr, total * 3))
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
    batch.decode_levels(Dest(total, 2).range, "natural")
    batch.wait()
    return batch


def ordering_batch_levels_behind_a_stalled_decode():
    """stall(A); RGBA decode on A; levels decode on B; pack of the RGBA outputs on C, with nothing but the library's events
    between them: the pack reads the new frames only if the levels decode waited for the decode and the pack for the levels
    decode (it orders itself behind the batch's last stream, B).  The levels are the new frames' too."""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    rgba = {id(f): orc.ImageData(f.jpeg()).decode() for f in old + new}
    want_new, want_old = np.stack([_u8_pack_want(rgba[id(f)]) for f in new]), np.stack([_u8_pack_want(rgba[id(f)]) for f in old])
    assert not np.array_equal(want_new, want_old), "the two outcomes this case must tell apart are the same"
    total = _total(new[0])
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])   # (the outputs still hold the old frames)
    dst = Dest(total, 2)
    packed = torch.full((2, 3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode(A.cuda_stream)
    batch.decode_levels(dst.range, "natural", hip_stream=B.cuda_stream)
    batch.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert batch.last_kernel() == "levels"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(ls.frame_levels(f), f, "natural", total), f"ordering, batch: levels of image {i}")
    assert np.array_equal(packed.cpu().numpy(), want_new), "the pack on the third stream did not read the decode on the first"


def ordering_batch_decode_behind_a_stalled_levels():
    """stall(A); levels decode on A; RGBA decode on B.  The decode on B orders itself behind the batch's last stream: while
    A's stall runs, B has not finished.  (B's state is read first, then A's: if A was still stalled at the second look, the
    first look was inside the stall.)  Then both results are the new frames'."""
    A, B = ss.independent_pair()
    old = [ps.sized("422", 48, 32, 4, seed=s) for s in (3, 40)]
    new = [ps.sized("422", 48, 32, 4, seed=s) for s in (60, 85)]
    total = _total(new[0])
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg()) for f in new])
    dst = Dest(total, 2)
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode_levels(dst.range, "zigzag", hip_stream=A.cuda_stream)
    batch.decode(B.cuda_stream)
    b_done = B.query()
    open_ = ss.window_open(A)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert not b_done, "the RGBA decode on the second stream finished while the levels decode's stream was stalled"
    assert batch.last_kernel() != "levels"
    got = dst.read("ordering, batch")
    for i, f in enumerate(new):
        _compare(got[i], _want(ls.frame_levels(f), f, "zigzag", total), f"ordering, batch: levels of image {i}")
        assert np.array_equal(batch.read_output(i), orc.ImageData(f.jpeg()).decode()), f"ordering, batch: RGBA {i}"


def ordering_decoder_levels_behind_a_stalled_decode():
    """stall(A); enqueue(new) on A; decode_levels(other) on B -- it rewrites the decoder's one set of input buffers, so it
    must not run before the decode on A has read them; a pack of the texture on C.  The texture and the pack are the new
    frame's only if the levels decode waited for the decode, the levels are the other frame's, and a decode on C
    afterwards leaves them alone.  (The window is looked at before the levels decode is issued: an upload waits on the
    host for the previous one's staging.)"""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    rgba_new, rgba_old = orc.ImageData(new.jpeg()).decode(), orc.ImageData(old.jpeg()).decode()
    assert not np.array_equal(rgba_new, rgba_old)
    total = _total(other)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dec.pack_tensor(torch.empty((3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    dec.decode_levels(ca.ImageData(other.jpeg()), Dest(total).range, blocking=True)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dst = Dest(total)
    packed = torch.full((3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    staged_new, staged_other, staged_old = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg()), ca.ImageData(old.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    open_ = ss.window_open(A)
    dec.decode_levels(staged_other, dst.range, hip_stream=B.cuda_stream)
    assert dec.last_kernel() == "levels"
    dec.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert np.array_equal(dec.read_texture(48, 32), rgba_new), "the decode on the first stream did not decode its own frame"
    assert np.array_equal(packed.cpu().numpy(), _u8_pack_want(rgba_new)), "the pack on the third stream did not read the decode on the first"
    want = _want(ls.frame_levels(other), other, "zigzag", total)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the levels")
    dec.enqueue(staged_old, Cs.cuda_stream)
    Cs.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(dec.read_texture(48, 32), rgba_old)
    _compare(dst.read("ordering, decoder")[0], want, "ordering, decoder: the levels after the next decode")


def ordering_decoder_decode_behind_a_stalled_levels():
    """stall(A); decode_levels(other) on A; enqueue(new) on B -- the enqueue rewrites the input buffers the levels decode
    on A has yet to read.  The levels are the other frame's only if the enqueue waited; the texture is the new frame's,
    and last_kernel names an RGBA kernel again."""
    A, B = ss.independent_pair()
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    total = _total(other)
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    rgba_kernel = dec.last_kernel()
    dec.decode_levels(ca.ImageData(other.jpeg()), Dest(total).range, "natural", blocking=True)
    dst = Dest(total)
    staged_new, staged_other = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.decode_levels(staged_other, dst.range, "natural", hip_stream=A.cuda_stream)
    assert dec.last_kernel() == "levels"
    open_ = ss.window_open(A)
    dec.enqueue(staged_new, B.cuda_stream)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert dec.last_kernel() == rgba_kernel != "levels"
    _compare(dst.read("ordering, decoder")[0], _want(ls.frame_levels(other), other, "natural", total), "ordering, decoder: the levels")
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
            levels = ls.frame_levels(f)
            for k, order in enumerate(ls.ORDERS):
                decoder_case(f, order, device=(i + k) % 2 == 1, levels=levels, dec=dec, blocking=(i + k) % 3 != 0)
        for n, frames in enumerate(we.same_size_batches(layout)):
            levels = [ls.frame_levels(f) for f in frames]
            for k, order in enumerate(ls.ORDERS):
                batch_case(frames, order, mode=(n + k) % 3, chunk=2 * k, levels=levels)


CASES = {f"coefficient_families[{lay}]": (coefficient_families, (lay,)) for lay in LAYOUTS}
CASES.update({fn.__name__: (fn, ()) for fn in (standard_entropy_in_every_layout, tiny_and_one_lane, interval_counts, undecoded_tail,
                                               interval_longer_than_the_window, golden_files, batches, decoder_state_is_untouched,
                                               refusals_on_the_card, tables_beyond_the_lds_share, ordering_batch_levels_behind_a_stalled_decode,
                                               ordering_batch_decode_behind_a_stalled_levels, ordering_decoder_levels_behind_a_stalled_decode,
                                               ordering_decoder_decode_behind_a_stalled_levels)})


def main(out_path, only=""):
    global torch, ca, ps, ls, rs, cs, gs, orc, ss, gpu
    t0 = time.time()
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import coef_stream as cs
    import gray_stream as gs
    import levels_stream as ls
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
