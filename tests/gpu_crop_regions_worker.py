"""The GPU cases of tests/test_gpu_crop_regions.py: Batch.decode_cropped_regions / Decoder.decode_cropped_regions into torch
memory, every byte against tests/crop_regions_stream.py -- the destination between sentinels and over a pre-fill, so that
what must not be written shows.  Run in one process of their own that imports torch before the library
(tests/gpu_luma_worker.py: why).

    python tests/gpu_crop_regions_worker.py RESULTS.json [substring of the case names to run]

Every decode asserts last_kernel() == "cropped".  RESULTS.json: case name -> null, or what went wrong; "wall_s"."""
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ps = crs = rgs = ss = orc = gpu = None   # set by main(): torch first
GUARD, SENTINEL, PREFILL = 256, 0x5C, 0xA5
_MIXED = {}   # the mixed batch, its expectation and its region list: made once, left unchanged


class Dest:
    """`total` bytes of destination inside one torch block: sentinels, `shift` bytes, the slots over a pre-fill, sentinels."""

    def __init__(self, total, shift=0):
        self.total, self.shift = total, shift
        self.block = torch.full((GUARD + shift + max(total, 1) + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.block[GUARD + shift:GUARD + shift + total] = PREFILL
        torch.cuda.synchronize()

    @property
    def range(self):
        return (self.block.data_ptr() + GUARD + self.shift, self.total)

    def read(self, what):
        torch.cuda.synchronize()
        host = self.block.cpu().numpy()
        assert (host[:GUARD + self.shift] == SENTINEL).all() and (host[GUARD + self.shift + self.total:] == SENTINEL).all(), f"{what}: a sentinel was written"
        return host[GUARD + self.shift:GUARD + self.shift + self.total]


def _compare(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{what}: {bad.size} of {want.size} bytes differ, first at {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def _shift(format, odd):
    """Bytes behind the 256-byte guard: the rgba destination needs a multiple of 4, the planar one takes any address."""
    return (4 if format == "rgba" else 1) if odd else 0


def _geometry(slot, format, pitched):
    pitch = (4 * slot[0] + 15) // 16 * 16 + 16 if pitched and format == "rgba" else None
    mine = rgs.shape(slot, format, pitch)
    assert ca.crop_regions_shape(slot, format, pitch) == mine
    return pitch, mine[1]


def _mixed():
    if not _MIXED:
        frames = rgs.mixed_batch()
        _MIXED.update(frames=frames, fulls=rgs.mixed_fulls(frames, ca), regions=rgs.mixed_regions())
    return _MIXED["frames"], _MIXED["fulls"], _MIXED["regions"]


def _upload(frames, mode=0):
    batch = ca.Batch(gpu)
    batch.set_device_preprocess(mode)
    batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in frames])
    return batch


def regions_case(batch, fulls, regions, slot, format="rgba", pitched=False, odd=False, chunk=0, what=""):
    """slot None: the library is left to take it from the list, the expectation takes rgs.slot_of."""
    given, slot = slot, slot or rgs.slot_of(regions)
    pitch, slot_bytes = _geometry(slot, format, pitched)
    total = slot_bytes * len(regions)
    batch.set_chunk(chunk)
    dst = Dest(total, _shift(format, odd))
    batch.decode_cropped_regions(dst.range, regions, given, format, pitch)
    batch.wait()
    what = f"{what}: {len(regions)} regions, {format}, {'pitched' if pitched else 'tight'}, {'odd' if odd else 'aligned'}, chunk {chunk}"
    if regions:
        assert batch.last_kernel() == "cropped", f"{what}: last_kernel() = {batch.last_kernel()}"
    _compare(dst.read(what), rgs.destination(fulls, regions, slot, format, pitch, before=np.full(total, PREFILL, dtype=np.uint8)), what)


# ---- the cases -------------------------------------------------------------------------------------------------------

def mixed_batch(mode):
    """The mixed batch with the full region list: both formats, tight / pitched, aligned / odd, chunks of 0, 1 and 3 regions."""
    frames, fulls, regions = _mixed()
    batch = _upload([f for f, _ in frames], mode)
    n = 0
    for format in rgs.FORMATS:
        for pitched, odd in ((False, False), (True, True)) if format == "rgba" else ((False, False), (False, True)):
            regions_case(batch, fulls, regions, rgs.SLOT, format, pitched, odd, chunk=(0, 1, 3, 0)[n % 4], what=f"mixed batch, mode {mode}")
            n += 1
    # (every chunk in every mode, on the format the loop above gave another chunk)
    regions_case(batch, fulls, regions, rgs.SLOT, "rgb_planar", chunk=1, what=f"mixed batch, mode {mode}")
    regions_case(batch, fulls, regions, rgs.SLOT, "rgba", chunk=3, what=f"mixed batch, mode {mode}")
    regions_case(batch, fulls, regions, None, "rgba", what=f"mixed batch, mode {mode}, slot from the list")


def identity_with_the_one_rectangle_decode():
    """A uniform batch of three 324 x 70 4:2:2 frames, one region per image with the same rectangle and slot = rectangle:
    byte for byte what Batch.decode_cropped writes for the same batch, for three rectangles, both formats."""
    w, h = crs.SIZE
    frames = [ps.sized("422", w, h, 9, standard=s % 2 == 0, seed=s) for s in (1, 50, 90)]
    batch = _upload(frames)
    for n, rect in enumerate(((37, 11, 150, 41), (0, 0, w, h), (300, 60, 24, 10))):
        for format in rgs.FORMATS:
            pitch = 4 * rect[2] + 16 if format == "rgba" and n == 0 else None
            total = crs.shape(w, h, rect, format, pitch)[1]
            assert rgs.shape(rect[2:], format, pitch)[1] == total
            one, many = Dest(3 * total), Dest(3 * total)
            batch.decode_cropped(one.range, rect, format, pitch)
            batch.decode_cropped_regions(many.range, [(i, rect) for i in range(3)], None, format, pitch)
            batch.wait()
            a, b = one.read("one rectangle"), many.read("region list")
            assert (a != PREFILL).any()
            _compare(b, a, f"region list against decode_cropped: {rect}, {format}")


def identity_with_the_cards_own_rgba():
    """Batch.decode of the mixed batch, then every region cut out of read_output: the card against itself, and the RGBA
    outputs are what they were after the region decode."""
    frames, fulls, regions = _mixed()
    batch = _upload([f for f, _ in frames])
    batch.decode()
    batch.wait()
    outs = [batch.read_output(i).copy() for i in range(len(frames))]
    own = [(outs[i], fulls[i][1]) for i in range(len(frames))]   # (the card's pixels, the expectation's mask of decoded MCUs)
    for format in rgs.FORMATS:
        _, slot_bytes = _geometry(rgs.SLOT, format, False)
        dst = Dest(slot_bytes * len(regions))
        batch.decode_cropped_regions(dst.range, regions, rgs.SLOT, format)
        batch.wait()
        assert batch.last_kernel() == "cropped"
        want = rgs.destination(own, regions, rgs.SLOT, format, before=np.full(dst.total, PREFILL, dtype=np.uint8))
        _compare(dst.read("own rgba"), want, f"against the card's own RGBA, {format}")
    for i in range(len(frames)):
        assert np.array_equal(batch.read_output(i), outs[i]), f"the region decode touched RGBA output {i}"


def decoder_form():
    """Six regions of one frame: blocking and on a stream, host and device preprocessing, both formats; the texture stays."""
    w, h = crs.SIZE
    f = ps.sized("420", w, h, 35, seed=6)
    full = crs.frame_rgba(f)
    regions = [(0, (37, 11, 150, 41), (1, 0)), (0, (0, 0, 1, 1)), (0, (300, 60, 24, 10), (126, 31)), (0, (100, 0, 3, 70), (0, 1)),
               (0, (0, 31, 150, 2), (0, 69)), (0, (160, 16, 16, 16), (134, 55))]
    slot = (151, 71)
    dec = ca.Decoder(gpu)
    other = ps.sized("422", 48, 32, 4, seed=3)
    dec.decode_blocking(ca.ImageData(other.jpeg()))
    texture = dec.read_texture(48, 32).copy()
    n = 0
    for device in (False, True):
        dec.set_device_preprocess(device)
        for blocking in (True, False):
            format = rgs.FORMATS[n % 2]
            pitch, slot_bytes = _geometry(slot, format, n == 2)
            dst = Dest(slot_bytes * 6, _shift(format, n % 2 == 1))
            img = ca.ImageData(f.jpeg(), **f.image_kw())
            if blocking:
                dec.decode_cropped_regions(img, dst.range, regions, slot, format, pitch, blocking=True)
            else:
                s = torch.cuda.Stream()
                dec.decode_cropped_regions(img, dst.range, regions, slot, format, pitch, hip_stream=s.cuda_stream)
                s.synchronize()
            what = f"Decoder: {format}, {'device' if device else 'host'} preprocessing, {'blocking' if blocking else 'stream'}"
            assert dec.last_kernel() == "cropped", what
            _compare(dst.read(what), rgs.destination([full], regions, slot, format, pitch, before=np.full(dst.total, PREFILL, dtype=np.uint8)), what)
            n += 1
    assert np.array_equal(dec.read_texture(48, 32), texture), "the region decode touched the texture"
    dst = Dest(64)
    dec.decode_cropped_regions(ca.ImageData(f.jpeg(), **f.image_kw()), dst.range, [], (4, 4), blocking=True)
    assert (dst.read("no regions") == PREFILL).all()


def one_region_and_none():
    frames, fulls, regions = _mixed()
    batch = _upload([f for f, _ in frames])
    regions_case(batch, fulls, regions[3:4], rgs.SLOT, "rgba", what="one region")
    regions_case(batch, fulls, [(6, (0, 0, 1, 1))], None, "rgb_planar", odd=True, what="one region, a 1 x 1 slot")
    before = batch.last_kernel()
    dst = Dest(64)
    batch.decode_cropped_regions(dst.range, [], (4, 4))
    batch.wait()
    assert (dst.read("no regions") == PREFILL).all() and batch.last_kernel() == before


def rgba_decodes_and_a_pack_around():
    """RGBA decodes and a pack before and after the region decode on the same batch, still right; last_kernel before,
    between and after."""
    w, h = 63, 33
    frames = [ps.sized("422", w, h, 4, seed=s) for s in (1, 30, 77)]
    fulls = [crs.frame_rgba(f) for f in frames]
    rgba = [orc.ImageData(f.jpeg(), **f.image_kw()).decode() for f in frames]
    packed_want = np.stack([np.ascontiguousarray(x[..., :3].transpose(2, 0, 1)) for x in rgba])
    regions = [(2, (5, 3, 40, 20), (1, 1)), (0, (0, 0, w, h)), (2, (62, 32, 1, 1), (62, 32)), (1, (7, 0, 9, 33), (3, 0))]
    for mode in (0, 2):
        batch = _upload(frames, mode)
        batch.decode()
        batch.wait()
        first = batch.last_kernel()
        assert first != "cropped"
        packed = torch.zeros((3, 3, h, w), dtype=torch.uint8, device="cuda")
        batch.pack_tensor(packed, dtype="u8")
        batch.wait()
        assert np.array_equal(packed.cpu().numpy(), packed_want), f"mode {mode}: pack before"
        regions_case(batch, fulls, regions, (w, h), "rgba", chunk=2, what=f"around, mode {mode}")
        regions_case(batch, fulls, regions, (w, h), "rgb_planar", odd=True, what=f"around, mode {mode}")
        for i in range(3):
            assert np.array_equal(batch.read_output(i), rgba[i]), f"mode {mode}: RGBA {i} after the region decodes"
        packed.zero_()
        batch.pack_tensor(packed, dtype="u8")
        batch.wait()
        assert np.array_equal(packed.cpu().numpy(), packed_want), f"mode {mode}: pack after the region decodes"
        batch.set_chunk(0)
        batch.decode()
        batch.wait()
        assert batch.last_kernel() == first
        for i in range(3):
            assert np.array_equal(batch.read_output(i), rgba[i]), f"mode {mode}: RGBA {i} decoded again"


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
    slot = (8, 4)
    slot_bytes = rgs.shape(slot)[1]
    assert slot_bytes == 128
    good = [(0, (4, 2, 5, 3)), (2, (0, 0, 8, 4)), (1, (30, 15, 3, 2), (5, 2))]
    dst = Dest(slot_bytes * 4)
    addr = dst.range[0]
    batch = ca.Batch(gpu)
    with Raises(ca.E_INVALID_ARG, "nothing uploaded"):
        batch.decode_cropped_regions(dst.range, good, slot)
    batch.upload([img, img, img])
    with Raises(ca.E_INVALID_ARG, "region 1", "image 3", "3 image"):
        batch.decode_cropped_regions(dst.range, [good[0], (3, (0, 0, 1, 1)), good[2]], slot)
    with Raises(ca.E_INVALID_ARG, "region 1", "5x3 at (29, 2)", "beyond", "33x17"):   # a bad region in the middle of a good list
        batch.decode_cropped_regions(dst.range, [good[0], (1, (29, 2, 5, 3)), good[2]], slot)
    with Raises(ca.E_INVALID_ARG, "region 2", "placed at (6, 2)", "8x4"):
        batch.decode_cropped_regions(dst.range, [good[0], good[1], (1, (30, 15, 3, 2), (6, 2))], slot)
    with Raises(ca.E_INVALID_ARG, "region 0", "empty"):
        batch.decode_cropped_regions(dst.range, [(0, (4, 2, 0, 3))] + good, slot)
    with Raises(ca.E_INVALID_ARG, "dst_bytes", str(3 * slot_bytes - 1), str(3 * slot_bytes), "3 slot"):
        batch.decode_cropped_regions((addr, 3 * slot_bytes - 1), good, slot)
    with Raises(ca.E_INVALID_ARG, "address", "multiple of 4"):
        batch.decode_cropped_regions((addr + 2, 3 * slot_bytes), good, slot)
    with Raises(ca.E_INVALID_ARG, "device_dst is NULL"):
        batch.decode_cropped_regions((0, 3 * slot_bytes), good, slot)
    with Raises(ca.E_INVALID_ARG, "pitch 30"):
        batch.decode_cropped_regions(dst.range, good, slot, pitch=30)
    with Raises(ca.E_INVALID_ARG, "format 5"):
        batch.decode_cropped_regions(dst.range, good, slot, 5)
    with Raises(ca.E_INVALID_ARG, "regions is NULL"):
        ca.check(ca.lib.compeg_batch_decode_cropped_regions(batch._h, ca.C.byref(ca._crop_regions_spec(slot, "rgba", None)), None, 2, ca.C.c_void_p(addr),
                                                            dst.total, None))
    assert batch.last_kernel() == "none"
    dec = ca.Decoder(gpu)
    with Raises(ca.E_INVALID_ARG, "region 1", "image 1", "1 image"):
        dec.decode_cropped_regions(img, dst.range, [good[0], (1, (0, 0, 1, 1))], slot, blocking=True)
    with Raises(ca.E_INVALID_ARG, "dst_bytes"):
        dec.decode_cropped_regions(img, (addr, slot_bytes), [good[0], good[0]], slot)
    assert dec.last_kernel() == "none"
    assert (dst.read("refusals") == PREFILL).all()


WINDOW = "the stalled stream had drained before the consumer was issued: the case did not test the ordering"
ORDER_REGIONS = [(1, (5, 3, 40, 27), (1, 0)), (0, (0, 0, 48, 32)), (1, (47, 31, 1, 1), (47, 31))]
ORDER_SLOT = (48, 32)


def _u8_pack_want(rgba):
    return np.ascontiguousarray(rgba[..., :3].transpose(2, 0, 1))


def _order_frames():
    """(old, new): two pairs of a 4:2:2 and a 4:2:0 frame (two samplings: two launches) of one size."""
    return [[ps.sized(lay, 48, 32, 4 if lay == "422" else 3, seed=s) for lay, s in zip(("422", "420"), seeds)] for seeds in ((3, 40), (60, 85))]


def _batch_for_ordering(old, total):
    """A batch that has done everything once with frames of the new ones' sizes and samplings: every buffer has its size."""
    batch = ca.Batch(gpu)
    batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in old])
    batch.decode()
    batch.pack_tensor(torch.empty((2, 3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    batch.decode_cropped_regions(Dest(total).range, ORDER_REGIONS, ORDER_SLOT, "rgb_planar")
    batch.wait()
    return batch


def ordering_batch_regions_behind_a_stalled_decode():
    """stall(A); RGBA decode on A; region decode on B; pack of the RGBA outputs on C, with nothing but the library's events
    between them: the pack reads the new frames only if the region decode waited for the decode and the pack for the
    region decode (it orders itself behind the batch's last stream, B)."""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new = _order_frames()
    rgba = {id(f): orc.ImageData(f.jpeg(), **f.image_kw()).decode() for f in old + new}
    want_new, want_old = np.stack([_u8_pack_want(rgba[id(f)]) for f in new]), np.stack([_u8_pack_want(rgba[id(f)]) for f in old])
    assert not np.array_equal(want_new, want_old), "the two outcomes this case must tell apart are the same"
    total = 3 * _geometry(ORDER_SLOT, "rgb_planar", False)[1]
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in new])   # (the outputs still hold the old frames)
    dst = Dest(total)
    packed = torch.full((2, 3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode(A.cuda_stream)
    batch.decode_cropped_regions(dst.range, ORDER_REGIONS, ORDER_SLOT, "rgb_planar", hip_stream=B.cuda_stream)
    batch.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    open_ = ss.window_open(A)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert batch.last_kernel() == "cropped"
    want = rgs.destination([crs.frame_rgba(f) for f in new], ORDER_REGIONS, ORDER_SLOT, "rgb_planar", before=np.full(total, PREFILL, dtype=np.uint8))
    _compare(dst.read("ordering, batch"), want, "ordering, batch: the regions")
    assert np.array_equal(packed.cpu().numpy(), want_new), "the pack on the third stream did not read the decode on the first"


def ordering_batch_decode_behind_stalled_regions():
    """stall(A); region decode on A; RGBA decode on B.  The decode on B orders itself behind the batch's last stream: while
    A's stall runs, B has not finished.  Then both results are the new frames'."""
    A, B = ss.independent_pair()
    old, new = _order_frames()
    total = 3 * _geometry(ORDER_SLOT, "rgba", False)[1]
    batch = _batch_for_ordering(old, total)
    batch.upload([ca.ImageData(f.jpeg(), **f.image_kw()) for f in new])
    dst = Dest(total)
    torch.cuda.synchronize()
    ss.stall(A)
    batch.decode_cropped_regions(dst.range, ORDER_REGIONS, ORDER_SLOT, "rgba", hip_stream=A.cuda_stream)
    batch.decode(B.cuda_stream)
    b_done = B.query()
    open_ = ss.window_open(A)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert not b_done, "the RGBA decode on the second stream finished while the region decode's stream was stalled"
    assert batch.last_kernel() != "cropped"
    want = rgs.destination([crs.frame_rgba(f) for f in new], ORDER_REGIONS, ORDER_SLOT, "rgba", before=np.full(total, PREFILL, dtype=np.uint8))
    _compare(dst.read("ordering, batch"), want, "ordering, batch: the regions")
    for i, f in enumerate(new):
        assert np.array_equal(batch.read_output(i), orc.ImageData(f.jpeg(), **f.image_kw()).decode()), f"ordering, batch: RGBA {i}"


DEC_REGIONS = [(0, (5, 3, 40, 27), (1, 0)), (0, (47, 31, 1, 1), (47, 31))]


def ordering_decoder_regions_behind_a_stalled_decode():
    """stall(A); enqueue(new) on A; decode_cropped_regions(other) on B -- it rewrites the decoder's one set of input buffers,
    so it must not run before the decode on A has read them; a pack of the texture on C.  (The window is looked at before
    the region decode is issued: an upload waits on the host for the previous one's staging.)"""
    A, B = ss.independent_pair()
    Cs = ss.independent_of((A, B))
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    rgba_new, rgba_old = orc.ImageData(new.jpeg()).decode(), orc.ImageData(old.jpeg()).decode()
    assert not np.array_equal(rgba_new, rgba_old)
    total = 2 * _geometry(ORDER_SLOT, "rgba", False)[1]
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dec.pack_tensor(torch.empty((3, 32, 48), dtype=torch.uint8, device="cuda"), dtype="u8")
    dec.decode_cropped_regions(ca.ImageData(other.jpeg()), Dest(total).range, DEC_REGIONS, ORDER_SLOT, blocking=True)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    dst = Dest(total)
    packed = torch.full((3, 32, 48), 7, dtype=torch.uint8, device="cuda")
    staged_new, staged_other = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.enqueue(staged_new, A.cuda_stream)
    open_ = ss.window_open(A)
    dec.decode_cropped_regions(staged_other, dst.range, DEC_REGIONS, ORDER_SLOT, hip_stream=B.cuda_stream)
    assert dec.last_kernel() == "cropped"
    dec.pack_tensor(packed, dtype="u8", hip_stream=Cs.cuda_stream)
    for s in (A, B, Cs):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert np.array_equal(dec.read_texture(48, 32), rgba_new), "the decode on the first stream did not decode its own frame"
    assert np.array_equal(packed.cpu().numpy(), _u8_pack_want(rgba_new)), "the pack on the third stream did not read the decode on the first"
    want = rgs.destination([crs.frame_rgba(other)], DEC_REGIONS, ORDER_SLOT, "rgba", before=np.full(total, PREFILL, dtype=np.uint8))
    _compare(dst.read("ordering, decoder"), want, "ordering, decoder: the regions")


def ordering_decoder_decode_behind_stalled_regions():
    """stall(A); decode_cropped_regions(other) on A; enqueue(new) on B -- the enqueue rewrites the input buffers the region
    decode on A has yet to read.  The regions are the other frame's only if the enqueue waited; the texture is the new
    frame's, and last_kernel names an RGBA kernel again."""
    A, B = ss.independent_pair()
    old, new, other = (ps.sized("422", 48, 32, 4, seed=s) for s in (3, 60, 85))
    total = 2 * _geometry(ORDER_SLOT, "rgb_planar", False)[1]
    dec = ca.Decoder(gpu)
    dec.decode_blocking(ca.ImageData(old.jpeg()))
    rgba_kernel = dec.last_kernel()
    dec.decode_cropped_regions(ca.ImageData(other.jpeg()), Dest(total).range, DEC_REGIONS, ORDER_SLOT, "rgb_planar", blocking=True)
    dst = Dest(total)
    staged_new, staged_other = ca.ImageData(new.jpeg()), ca.ImageData(other.jpeg())
    torch.cuda.synchronize()
    ss.stall(A)
    dec.decode_cropped_regions(staged_other, dst.range, DEC_REGIONS, ORDER_SLOT, "rgb_planar", hip_stream=A.cuda_stream)
    assert dec.last_kernel() == "cropped"
    open_ = ss.window_open(A)
    dec.enqueue(staged_new, B.cuda_stream)
    for s in (A, B):
        s.synchronize()
    torch.cuda.synchronize()
    assert open_, WINDOW
    assert dec.last_kernel() == rgba_kernel != "cropped"
    want = rgs.destination([crs.frame_rgba(other)], DEC_REGIONS, ORDER_SLOT, "rgb_planar", before=np.full(total, PREFILL, dtype=np.uint8))
    _compare(dst.read("ordering, decoder"), want, "ordering, decoder: the regions")
    assert np.array_equal(dec.read_texture(48, 32), orc.ImageData(new.jpeg()).decode()), "the decode on the second stream did not decode its own frame"


def tables_beyond_the_lds_share():
    """Frames whose Huffman tables outgrow their share of LDS (cs.wide_cases, gs.wide_cases; cs.table_regime) in one batch, all
    samplings and the three regimes side by side: a region of every image, so that every launch names regions of regime-A
    and regime-C images -- planned with the largest image's tables while each image stages its own; chunks of 0, 1 and 7
    regions, the three preprocessing modes.  And the Decoder's form on a regime-C frame of every sampling."""
    import wide_emul as we
    frames = [f for f in we.frames() if f.mcus <= 65]
    for lay in we.SAMPLINGS:
        assert {we.regime(f) for f in frames if we.layout_of(f) == lay} == set("ABC"), lay
    fulls = [crs.frame_rgba(f) for f in frames]
    slot = (max(f.w for f in frames) + 1, max(f.h for f in frames) + 1)
    regions = [(i, (0, 0, f.w, f.h) if i % 2 == 0 else (f.w // 3, f.h // 4, max(1, f.w // 2), max(1, f.h // 2)), (i % 2, i % 3 % 2)) for i, f in enumerate(frames)]
    for mode in (0, 1, 2):
        batch = _upload(frames, mode)
        regions_case(batch, fulls, regions, slot, rgs.FORMATS[mode % 2], pitched=mode == 0, odd=mode == 1, chunk=(0, 1, 7)[mode], what=f"wide tables, mode {mode}")
    dec = ca.Decoder(gpu)
    for n, lay in enumerate(we.SAMPLINGS):
        k, f = next((k, f) for k, f in enumerate(frames) if we.layout_of(f) == lay and we.regime(f) == "C" and f.intervals == 65)
        mine = [(0, (0, 0, f.w, f.h)), (0, (f.w // 3, f.h // 4, max(1, f.w // 2), max(1, f.h // 2)), (1, 1))]
        format = rgs.FORMATS[n % 2]
        pitch, slot_bytes = _geometry(slot, format, n == 0)
        dst = Dest(slot_bytes * 2, _shift(format, n % 2 == 1))
        dec.set_device_preprocess(n % 2 == 1)
        dec.decode_cropped_regions(ca.ImageData(f.jpeg(), **f.image_kw()), dst.range, mine, slot, format, pitch, blocking=True)
        assert dec.last_kernel() == "cropped", f.name
        _compare(dst.read(f.name), rgs.destination([fulls[k]], mine, slot, format, pitch, before=np.full(dst.total, PREFILL, dtype=np.uint8)), f"Decoder: {f.name}")


CASES = {f"mixed_batch[mode {m}]": (mixed_batch, (m,)) for m in (0, 1, 2)}
CASES.update({fn.__name__: (fn, ()) for fn in (identity_with_the_one_rectangle_decode, identity_with_the_cards_own_rgba, decoder_form,
                                               one_region_and_none, rgba_decodes_and_a_pack_around, refusals_on_the_card, tables_beyond_the_lds_share,
                                               ordering_batch_regions_behind_a_stalled_decode, ordering_batch_decode_behind_stalled_regions,
                                               ordering_decoder_regions_behind_a_stalled_decode, ordering_decoder_decode_behind_stalled_regions)})


def main(out_path, only=""):
    global torch, ca, ps, crs, rgs, ss, orc, gpu
    t0 = time.time()
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import crop_regions_stream as rgs
    import crop_stream as crs
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
