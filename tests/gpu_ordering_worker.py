"""The GPU cases of tests/test_gpu_ordering.py: the library's ordering across streams -- every pack behind the decode it
reads, every decode behind the packs that read what it overwrites, the record block and its pinned slots, the calls that
are specified to wait on the host -- with the PRODUCER STREAM HELD BUSY (tests/stream_stall.py), so that the library's
events and not the microseconds a small decode takes decide what a consumer reads.  Run in one process of their own that
imports torch before the library (tests/gpu_orient_worker.py has the same order).

    python tests/gpu_ordering_worker.py RESULTS.json [substring of the case names to run]

A case of kind "device-ordered" queues a stall, the producer behind it, the consumer on another stream, and asserts at once
that the stalled stream has not drained (window_open): the consumer was issued while the producer had not run.  A case in
which the stall was over by then proves nothing and fails.  A case of kind "host-waits" queues a pack behind a stall and
calls something that is specified to block the host; on return the stalled stream must have drained.  Every case first
asserts, from the references alone, that the outcome it wants differs from the stale or overtaken one (dry=True stops
there: tests/test_gpu_ordering.py runs that without a card).

An owner is primed before its case: it has decoded every frame and made every pack of the case once, so that no buffer of
the library grows inside a stall -- freeing a device block waits for the whole card, the stall included.

Frames are 48x32 (4:2:2, three by four MCUs) and 17x9, outputs (13, 5); destinations are NaN-filled and compared with the
references of the pack workers bit for bit.  RESULTS.json: case name -> null, or what went wrong; "stall_ms",
"stall_kind", "wall_s": the calibrated stall as measured on the card, what it is made of, the worker's wall time."""
import functools
import json
import os
import sys
import time
import traceback

import numpy as np

torch = ca = ss = gpu = None   # set by main(): torch first
A = B = C = G = spare = gpu_on_g = None   # the streams (A, B: independent_pair; C, G: independent of them) and the Gpu over G

ENTRIES = ("plain", "resized", "antialias", "regions", "filtered", "oriented", "nhwc")
RECORD_ENTRIES = ENTRIES[1:]   # everything but pack_tensor uploads records
OWNERS = ("decoder", "batch")
SIZE = (13, 5)
FRAMES = {"F1": (48, 32, 41), "F2": (48, 32, 42), "S": (17, 9, 21)}   # (w, h, seed)
PAD, FILL = (10.0, 114.0, 250.5), 0.5
# (src, dst, orientation) of two slots each, crops inside 48x32: any mixture of two lists' records reads inside the image.
# The families without an orientation drop it; the resized packs, which have no dst either, take the crops.
R1 = ((None, None, 6), ((1, 0, 40, 30), (2, 1, 9, 3), 3))
R2 = (((8, 4, 32, 24), None, 2), ((3, 2, 20, 17), (1, 0, 11, 5), 8))
R3 = (((16, 8, 30, 20), (4, 2, 6, 2), 5), ((0, 6, 48, 20), (0, 1, 13, 4), 1))
RS = ((None, None, 1), ((1, 0, 15, 8), (2, 1, 9, 3), 1))   # the same inside 17x9
WINDOW = "the stall had ended when the consumer was issued: this run proves nothing about their order"


def _refs():
    import nhwc_reference as nr   # (imports the others: orient, filter, region, resize, antialias, tensor)
    return nr


def _specs():
    fr = _refs().fr
    return {"f32": ("f32",) + tuple(fr.IDENTITY), "f16": ("f16", fr.IMAGENET_SCALE, fr.IMAGENET_BIAS)}


def _frame(name):
    w, h, seed = FRAMES[name]
    return _refs().fr.frame(w, h, seed=seed)


def _rgba(name):
    return _frame(name)[1]


def images(owner, which):
    """The frames an owner holds: a decoder one, a batch two -- and "new" is "old" with the two exchanged."""
    one, other = ("F1", "F2") if which == "old" else ("F2", "F1")
    return (one,) if owner == "decoder" else (one, other)


def _form(entry, variant):
    """(filter or kernel, antialias) of an entry point's two forms: two different kernels of its family."""
    if entry == "resized" or entry == "regions":
        return ("bilinear", "nearest")[variant], False
    if entry == "antialias":
        return "bilinear", variant == 0
    return ("bicubic", "triangle")[variant], False


class Pack:
    """One pack call: an entry point, a region list, an element spec and which of the family's two kernels."""

    def __init__(self, owner, entry, regions=R1, variant=0, spec=None):
        self.entry, self.regions, self.variant = entry, regions, variant
        self.spec = spec or ("f32", "f16")[(ENTRIES.index(entry) + OWNERS.index(owner)) % 2]

    def want(self, held):
        return _want(self.entry, tuple(held), self.regions, self.spec, self.variant)

    def fresh(self, held):
        """A destination of NaNs: an element that nobody writes shows."""
        dtype = _specs()[self.spec][0]
        return torch.full(self.want(held).shape, float("nan"), dtype={"f16": torch.float16, "f32": torch.float32}[dtype], device="cuda")

    def issue(self, own, dst, stream):
        dtype, scale, bias = _specs()[self.spec]
        common = dict(dtype=dtype, scale=scale, bias=bias, hip_stream=stream.cuda_stream)
        obj, n = own.obj, len(own.held)
        what, antialias = _form(self.entry, self.variant)
        slots = [(r % n, src, dst_, o) for r, (src, dst_, o) in enumerate(self.regions)]
        if self.entry == "plain":
            obj.pack_tensor(dst, **common)
        elif self.entry in ("resized", "antialias"):
            crops = [_crop(self.regions[i][0], own.held[i]) for i in range(n)]
            if own.kind == "decoder":
                obj.pack_tensor_resized(dst, SIZE, crops[0], filter=what, antialias=antialias, **common)
            else:
                obj.pack_tensor_resized(dst, SIZE, crops, filter=what, antialias=antialias, **common)
        elif self.entry == "regions":
            obj.pack_tensor_regions(dst, SIZE, [s[:3] for s in slots], pad=PAD, filter=what, **common)
        elif self.entry == "filtered":
            obj.pack_tensor_filtered(dst, SIZE, [s[:3] for s in slots], kernel=what, pad=PAD, **common)
        elif self.entry == "oriented":
            obj.pack_tensor_oriented(dst, SIZE, slots, kernel=what, pad=PAD, **common)
        else:
            obj.pack_tensor_nhwc(dst, SIZE, slots, channels=4, fill=FILL, kernel=what, pad=PAD, **common)


def _crop(src, name):
    return src if src is not None else (0, 0) + FRAMES[name][:2]


@functools.lru_cache(maxsize=None)
def _want(entry, held, regions, spec, variant):
    """What a pack stores when the owner holds the frames `held`: every slot from the reference of its pack worker."""
    nr = _refs()
    orf, fr = nr.orf, nr.fr
    gr, rr, ar, tr = fr.gr, fr.gr.rr, fr.gr.ar, fr.gr.rr.tr
    dtype, scale, bias = _specs()[spec]
    rgba, n = [_rgba(name) for name in held], len(held)
    what, antialias = _form(entry, variant)
    if entry == "plain":
        return np.stack([tr.expected(r, 1, dtype, scale, bias) for r in rgba])
    if entry in ("resized", "antialias"):
        crops = [_crop(regions[i][0], held[i]) for i in range(n)]
        if antialias:
            return np.stack([ar.expected(rgba[i], SIZE, 1, dtype, scale, bias, "rgb", crops[i]) for i in range(n)])
        return np.stack([rr.expected(rgba[i], SIZE, 1, dtype, scale, bias, "rgb", what, crops[i]) for i in range(n)])
    slots = []
    for r, (src, dst, o) in enumerate(regions):
        image = rgba[r % n]
        if entry == "regions":
            slots.append(gr.expected(image, SIZE, 1, dtype, scale, bias, "rgb", what, src, dst, PAD))
        elif entry == "filtered":
            slots.append(fr.expected(image, SIZE, 1, dtype, scale, bias, "rgb", what, src, dst, PAD))
        elif entry == "oriented":
            slots.append(orf.expected(image, SIZE, 1, dtype, scale, bias, "rgb", what, src, dst, PAD, o))
        else:
            slots.append(nr.expected(image, SIZE, 1, dtype, scale, bias, "rgb", what, src, dst, PAD, o, 4, FILL))
    return np.stack(slots)


def _tell_apart(a, b, what):
    """The precondition of every case: the wanted outcome is not the stale or overtaken one."""
    assert a.shape != b.shape or not np.array_equal(a, b), f"{what}: the two outcomes this case must tell apart are the same"


def _check(got, want, what):
    """torch.equal on the values: -0 and +0 are one (the library is built -fno-signed-zeros), everything else its bits."""
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert not torch.isnan(got.float()).any(), f"{what}: elements that no lane wrote"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} elements differ"


def _same_pixels(got, held, what):
    for i, name in enumerate(held):
        assert np.array_equal(got[i], _rgba(name)), f"{what}: image {i} read back is not {name}"


class Owner:
    """A Decoder or a Batch of two images that holds `held`, decoded and synchronised, after it has decoded `primed` (so
    that its buffers have the size of either) and made `packs` once (so that its record block and one pinned slot have
    theirs)."""

    def __init__(self, kind, held, primed=(), packs=(), on=None):
        self.kind, self.obj, self.held, self.staged = kind, (ca.Decoder if kind == "decoder" else ca.Batch)(on or gpu), (), None
        for frames in (primed, held):
            if frames:
                self.hold(frames)
        for pack in packs:
            pack.issue(self, pack.fresh(self.held), spare)
        spare.synchronize()
        torch.cuda.synchronize()

    def hold(self, frames):
        """Decodes `frames` and waits."""
        self.stage(frames)
        if self.kind == "decoder":
            self.obj.decode_blocking(self.staged)
            self.held = tuple(frames)
        else:
            self.decode(None)
            self.obj.wait()

    def stage(self, frames):
        """What the next decode decodes.  On a batch this is the upload, which waits on the host for the batch's stream."""
        if self.kind == "decoder":
            self.staged = ca.ImageData(_frame(frames[0])[0])
        else:
            self.obj.upload([ca.ImageData(_frame(name)[0]) for name in frames])
        self._next = tuple(frames)

    def decode(self, stream):
        """Records the decode of what was staged on `stream` and returns without waiting."""
        if self.kind == "decoder":
            changed = self.obj.enqueue(self.staged, stream.cuda_stream)
        else:
            changed = None
            self.obj.decode(stream.cuda_stream if stream is not None else 0)
        self.held = self._next
        return changed

    def read(self):
        if self.kind == "decoder":
            w, h, _ = FRAMES[self.held[0]]
            return [self.obj.read_texture(w, h)]
        return [self.obj.read_output(i) for i in range(len(self.held))]


def _drain(*streams):
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()


def read_after_write(owner, entry, dry=False):
    """device-ordered.  The owner holds the old frames; stall(A), the decode of the new ones on A, the pack on B.  The
    destination holds the new frames' values; a pack that overtook the decode would have stored the old ones'."""
    pack, old, new = Pack(owner, entry), images(owner, "old"), images(owner, "new")
    _tell_apart(pack.want(new), pack.want(old), "new frames, old frames")
    if dry:
        return
    own = Owner(owner, old, primed=new, packs=[pack])
    own.stage(new)
    dst = pack.fresh(new)
    _drain()
    ss.stall(A)
    own.decode(A)
    pack.issue(own, dst, B)
    open_ = ss.window_open(A)
    _drain(A, B)
    assert open_, WINDOW
    _check(dst, pack.want(new), f"{entry} behind the stalled decode")


def write_after_read(owner, entry, dry=False):
    """device-ordered.  The owner holds the old frames; stall(B), the pack on B, then on A what must stand behind it.  A
    decoder decodes the new frame on A: the destination holds the old frame's values and the texture then reads back as the
    new one.  A batch can decode nothing else without an upload, which waits on the host (host_waits has that), so its
    second decode would store the same pixels again and no value could tell; instead a pack_tensor into a second destination
    goes on A, and wait() -- which follows the batch's last stream, A -- must return only when B has drained as well."""
    pack, old, new = Pack(owner, entry), images(owner, "old"), images(owner, "new")
    second = Pack(owner, "plain", spec="f16" if pack.spec == "f32" else "f32")
    _tell_apart(pack.want(old), pack.want(new), "old frames, new frames")
    if dry:
        return
    own = Owner(owner, old, primed=new, packs=[pack, second])
    if owner == "decoder":
        own.stage(new)
    dst, dst2 = pack.fresh(old), second.fresh(old)
    _drain()
    ss.stall(B)
    pack.issue(own, dst, B)
    if owner == "decoder":
        own.decode(A)
        open_ = ss.window_open(B)
    else:
        second.issue(own, dst2, A)
        open_ = ss.window_open(B)
        own.obj.wait()
        waited = B.query()
    _drain(A, B)
    assert open_, WINDOW
    _check(dst, pack.want(old), f"{entry} in front of what followed on the other stream")
    if owner == "decoder":
        _same_pixels(own.read(), new, "the decode behind the stalled pack")
    else:
        _check(dst2, second.want(old), "pack_tensor behind the stalled pack")
        assert waited, "wait() returned while the pack on the other stream had not run"


def batch_decode_behind_a_stalled_pack(dry=False):
    """device-ordered.  write_after_read's batch form with the batch's own decode between the two packs: stall(B), a pack
    on B, decode(A) -- the wait at the top of compeg_batch::decode --, pack_tensor on A, wait()."""
    pack, second, old = Pack("batch", "filtered"), Pack("batch", "plain", spec="f16"), images("batch", "old")
    if dry:
        return
    own = Owner("batch", old, packs=[pack, second])
    dst, dst2 = pack.fresh(old), second.fresh(old)
    _drain()
    ss.stall(B)
    pack.issue(own, dst, B)
    own.decode(A)
    second.issue(own, dst2, A)
    open_ = ss.window_open(B)
    own.obj.wait()
    waited = B.query()
    _drain(A, B)
    assert open_, WINDOW
    assert waited, "wait() returned while the pack in front of the decode had not run"
    _check(dst, pack.want(old), "the pack in front of the decode")
    _check(dst2, second.want(old), "pack_tensor behind the decode")


def chain_of_three_streams(owner, first, then, dry=False):
    """device-ordered.  stall(A), the decode of the new frames on A, a pack on B, a pack through another entry point on C,
    no host waits: both destinations hold the new frames' values."""
    packs, old, new = (Pack(owner, first), Pack(owner, then, R2)), images(owner, "old"), images(owner, "new")
    for p in packs:
        _tell_apart(p.want(new), p.want(old), f"{p.entry}: new frames, old frames")
    if dry:
        return
    own = Owner(owner, old, primed=new, packs=packs)
    own.stage(new)
    dsts = [p.fresh(new) for p in packs]
    _drain()
    ss.stall(A)
    own.decode(A)
    packs[0].issue(own, dsts[0], B)
    packs[1].issue(own, dsts[1], C)
    open_ = ss.window_open(A)
    _drain(A, B, C)
    assert open_, WINDOW
    for p, d, s in zip(packs, dsts, "BC"):
        _check(d, p.want(new), f"{p.entry} on {s}")


def record_block_two_streams(owner, entry, dry=False):
    """device-ordered.  stall(A), a pack of R1 on A, a pack of R2 on B into another destination: the one device record block
    is rewritten for the second only behind the kernel of the first.  Each destination shows its own regions."""
    packs, old = (Pack(owner, entry, R1), Pack(owner, entry, R2)), images(owner, "old")
    _tell_apart(packs[0].want(old), packs[1].want(old), "R1, R2")
    if dry:
        return
    own = Owner(owner, old, packs=packs)
    dsts = [p.fresh(old) for p in packs]
    _drain()
    ss.stall(A)
    packs[0].issue(own, dsts[0], A)
    packs[1].issue(own, dsts[1], B)
    open_ = ss.window_open(A)
    _drain(A, B)
    assert open_, WINDOW
    _check(dsts[0], packs[0].want(old), f"{entry} of R1 on the stalled stream")
    _check(dsts[1], packs[1].want(old), f"{entry} of R2 on the other stream")


def pinned_slots_one_stream(owner, entry, dry=False):
    """device-ordered.  stall(A), three packs on A with three region lists and two kernels of the family: none of their
    copies out of pinned memory has run when the next pack stages its records, so each needs a slot of its own.  Each
    destination shows its own regions.  (tests/gpu_filter_worker.py: record_staging, with the stream held.)"""
    packs, old = (Pack(owner, entry, R1, 0), Pack(owner, entry, R2, 1), Pack(owner, entry, R3, 0)), images(owner, "old")
    for i, j in ((0, 1), (1, 2), (0, 2)):
        _tell_apart(packs[i].want(old), packs[j].want(old), f"packs {i} and {j}")
    if dry:
        return
    own = Owner(owner, old, packs=packs)
    dsts = [p.fresh(old) for p in packs]
    _drain()
    ss.stall(A)
    for p, d in zip(packs, dsts):
        p.issue(own, d, A)
    open_ = ss.window_open(A)
    _drain(A)
    assert open_, WINDOW
    for i, (p, d) in enumerate(zip(packs, dsts)):
        _check(d, p.want(old), f"{entry}, pack {i} of three")


def growth(dry=False):
    """host-waits.  A new decoder holds the 17x9 frame; stall(B) and a pack of it on B; stall(A), enqueue(F2, A) -- the
    texture grows to 48x32, which the call reports --, pack_tensor_filtered on B: the small frame's values in the first
    destination, F2's in the second.  Growing the texture frees its block, and the pack on B has still to read that block:
    the free must wait for it, on the host, so B has drained when enqueue returns.  That is why this case is none of the
    device-ordered kind: the wait takes the stall on A with it, and no window is left to assert.  (With the allocation
    there already nothing grows: a decoder's texture keeps the largest extent it has had.)"""
    small, pack = Pack("decoder", "filtered", RS), Pack("decoder", "filtered")
    _tell_apart(pack.want(("F2",)), pack.want(("F1",)), "F2, F1")
    _tell_apart(_rgba("F2")[:9, :17], _rgba("S"), "F2's corner, the small frame")
    if dry:
        return
    own = Owner("decoder", ("S",))
    own.stage(("F2",))
    first, dst = small.fresh(("S",)), pack.fresh(("F2",))
    _drain()
    ss.stall(B)
    small.issue(own, first, B)
    ss.stall(A)
    open_ = ss.window_open(B)
    changed = own.decode(A)
    waited = B.query()
    pack.issue(own, dst, B)
    _drain(A, B)
    assert open_, "the stall had ended before the call was made: " + WINDOW
    assert changed, "enqueue did not report that the texture changed"
    assert waited, "enqueue freed the texture's old block while the pack that reads it had not run"
    _check(first, small.want(("S",)), "the pack of the small frame, in front of the growth")
    _check(dst, pack.want(("F2",)), "filtered pack behind the decode that grew the texture")
    _same_pixels(own.read(), ("F2",), "the grown texture")


def gpu_stream_decodes_behind_a_pack(dry=False):
    """device-ordered.  A decoder of a Gpu opened over the torch stream G; stall(B), a pack on B, start_decode(F2), which
    runs on G: the destination holds F1's values and the texture reads back as F2."""
    pack = Pack("decoder", "oriented")
    _tell_apart(pack.want(("F1",)), pack.want(("F2",)), "F1, F2")
    if dry:
        return
    own = Owner("decoder", ("F1",), primed=("F2",), packs=[pack], on=gpu_on_g)
    own.stage(("F2",))
    dst = pack.fresh(("F1",))
    _drain(G)
    ss.stall(B)
    pack.issue(own, dst, B)
    op = own.obj.start_decode(own.staged)
    own.held = ("F2",)
    open_ = ss.window_open(B)
    op.wait()
    waited = B.query()
    _drain(B, G)
    assert open_, WINDOW
    assert waited, "the decode's event completed while the pack in front of it had not run"
    _check(dst, pack.want(("F1",)), "the pack in front of start_decode")
    _same_pixels(own.read(), ("F2",), "start_decode behind the stalled pack")


def gpu_stream_decode_stalled(dry=False):
    """device-ordered.  stall(G), start_decode(F2) on the Gpu's own stream G, a pack on B: F2's values."""
    pack = Pack("decoder", "nhwc")
    _tell_apart(pack.want(("F2",)), pack.want(("F1",)), "F2, F1")
    if dry:
        return
    own = Owner("decoder", ("F1",), primed=("F2",), packs=[pack], on=gpu_on_g)
    own.stage(("F2",))
    dst = pack.fresh(("F2",))
    _drain(G)
    ss.stall(G)
    op = own.obj.start_decode(own.staged)
    own.held = ("F2",)
    pack.issue(own, dst, B)
    open_ = ss.window_open(G)
    _drain(B, G)
    assert open_, WINDOW
    op.wait()
    _check(dst, pack.want(("F2",)), "the pack behind start_decode on the stalled stream")


def host_waits(owner, call, entry, dry=False):
    """host-waits.  The owner holds the old frames; stall(B), a pack on B, then a call that is specified to block the host
    until the owner's last stream -- B -- has drained.  On return B.query() is true; the destination holds the old frames'
    values; and what the call hands back is right."""
    pack, old, new = Pack(owner, entry), images(owner, "old"), images(owner, "new")
    _tell_apart(pack.want(old), pack.want(new), "old frames, new frames")
    _tell_apart(_rgba("F1"), _rgba("F2"), "F1, F2")
    if dry:
        return
    own = Owner(owner, old, primed=new, packs=[pack])
    fresh_images = [ca.ImageData(_frame(name)[0]) for name in new]   # (parsed in front of the stall)
    dst = pack.fresh(old)
    _drain()
    ss.stall(B)
    pack.issue(own, dst, B)
    open_ = ss.window_open(B)
    after = None
    if call == "read_texture" or call == "read_output":
        after = (own.read(), old)
    elif call == "decode_blocking":
        own.obj.decode_blocking(fresh_images[0])
    elif call == "into_texture":
        texture = own.obj.into_texture()
    elif call == "drop":
        own.obj = None   # (the only reference: the decoder is freed here)
    elif call == "upload":
        own.obj.upload(fresh_images)
    else:
        assert call == "wait"
        own.obj.wait()
    waited = B.query()
    _drain(B)
    assert open_, "the stall had ended before the call was made: " + WINDOW
    assert waited, f"{call} returned while the pack on the owner's last stream had not run"
    _check(dst, pack.want(old), f"the pack in front of {call}")
    if call == "decode_blocking":
        own.held = new
        after = (own.read(), new)
    elif call == "into_texture":
        after = ([torch.as_tensor(texture, device="cuda").cpu().numpy()[:32, :48]], old)
    elif call == "upload":
        own._next = new
        own.decode(None)
        after = (own.read(), new)
    if after:
        _same_pixels(after[0], after[1], f"after {call}")


def control(when, dry=False):
    """The control of tests/stream_stall.py for the pair of streams the cases use, both ways: work on one really runs while
    the other is stalled.  Without it an open window would say nothing."""
    if dry:
        return
    assert ss.overtakes(A, B), f"{when}: work on B did not run while A was stalled"
    assert ss.overtakes(B, A), f"{when}: work on A did not run while B was stalled"
    assert ss.overtakes(A, C) and ss.overtakes(G, B) and ss.overtakes(B, G), f"{when}: C or G shares a queue with A or B"


def _cases():
    cases = {"control_at_the_start": (control, ("at the start",))}
    for owner in OWNERS:
        for entry in ENTRIES:
            cases[f"read_after_write[{owner}-{entry}]"] = (read_after_write, (owner, entry))
        for entry in ENTRIES:
            cases[f"write_after_read[{owner}-{entry}]"] = (write_after_read, (owner, entry))
        for entry in RECORD_ENTRIES:
            cases[f"record_block_two_streams[{owner}-{entry}]"] = (record_block_two_streams, (owner, entry))
        for entry in RECORD_ENTRIES:
            cases[f"pinned_slots_one_stream[{owner}-{entry}]"] = (pinned_slots_one_stream, (owner, entry))
    cases["batch_decode_behind_a_stalled_pack"] = (batch_decode_behind_a_stalled_pack, ())
    cases["chain_of_three_streams[decoder-filtered-nhwc]"] = (chain_of_three_streams, ("decoder", "filtered", "nhwc"))
    cases["chain_of_three_streams[batch-resized-oriented]"] = (chain_of_three_streams, ("batch", "resized", "oriented"))
    cases["growth"] = (growth, ())
    cases["gpu_stream_decodes_behind_a_pack"] = (gpu_stream_decodes_behind_a_pack, ())
    cases["gpu_stream_decode_stalled"] = (gpu_stream_decode_stalled, ())
    for owner, call, entry in (("decoder", "read_texture", "plain"), ("decoder", "decode_blocking", "regions"), ("decoder", "into_texture", "antialias"),
                               ("decoder", "drop", "filtered"), ("batch", "read_output", "oriented"), ("batch", "upload", "nhwc"), ("batch", "wait", "resized")):
        cases[f"host_waits[{owner}-{call}]"] = (host_waits, (owner, call, entry))
    cases["control_at_the_end"] = (control, ("at the end",))
    return cases


CASES = _cases()


def precondition(name):
    """What a case asserts before it touches the card: from the references alone."""
    fn, args = CASES[name]
    fn(*args, dry=True)


def main(out_path, only=""):
    global torch, ca, ss, gpu, A, B, C, G, spare, gpu_on_g
    t0 = time.time()
    import torch   # first: see the module's docstring
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import compeg_amd as ca
    import stream_stall as ss
    gpu = ca.Gpu.open(0)
    results, device_said_no, no_streams = {}, False, None
    try:
        spare = torch.cuda.Stream()
        A, B = ss.independent_pair()
        C = ss.independent_of([A])
        G = ss.independent_of([B], [B])
        gpu_on_g = ca.Gpu.from_stream(0, G.cuda_stream)
    except AssertionError as e:
        no_streams = f"no streams to run the cases on: {e}"
    except Exception:
        no_streams, device_said_no = traceback.format_exc(), True
    results["stall_ms"], results["stall_kind"] = ss.stall_ms(), ss.stall_kind()
    for name, (fn, args) in CASES.items():
        if only not in name and not name.startswith("control"):
            continue
        if no_streams:   # (neither skipped nor passed)
            results[name] = no_streams
            continue
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
        results["wall_s"] = round(time.time() - t0, 3)
        with open(out_path, "w") as f:   # (kept current: what ran is on record whatever happens next)
            json.dump(results, f)
        if device_said_no:   # nothing more is started on it
            break
    with open(out_path, "w") as f:
        json.dump(results, f)
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
