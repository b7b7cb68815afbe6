"""The edge matrix of the device-side scan preprocessor (compeg_amd/csrc/scan_kernels.hip), shared by the CPU tests
(tests/test_scan_edges.py) and the GPU tests (tests/test_gpu_scan_edges.py): the segments, the references, the case
file that tests/gpu_scan/scan_harness reads and the check of what it hands back.  All comparisons are exact.

Groups (one launch each, one test each):
  ladder[...]   runs of 1-20, 31-33, 47-49, 255-257 and 509-530 FF bytes that end at chunk offsets -2 .. +2, straddle the
                4096-byte tile seam, start the segment or end it, followed by 00, D0, D7, a plain byte, C0, D8, CF or nothing
  length[N]     the lengths at which tile and chunk counts change, each with the true interval count expected, one less,
                one more, 0, 1, a slot count below the count (wrapped start positions) and a power-of-two count
  dense         xx FF D0 up to the documented capacity, FF D0 / FF 00 / FF FF throughout, zeros, plain bytes at every
                output shift of emit_kernel's 16-byte path
  seam          a lead FF at byte 4094, 4095, 4096 behind kept bytes of every residue mod 4
  mixed         images of 0, 1, 2 and 257 tiles in one launch, span_kernel, a descriptor offset, some patch targets
  reuse[...]    two launches in a row on one arena, the second on what the first left there
  pull[...], pull3[...]   the compute-queue copies around their 16-byte rounding and their 48-block grid stride

References: words, start positions, count and error text from the oracle's ScanBuffer; kept bytes from a plain loop;
result[4] from a restatement of max_wave_span (group 64); the two flag bits from their definitions (flags())."""
import functools
import struct

import numpy as np

from oracle import oracle as orc

MAGIC = 0x484E4353
PREFILL = 0xA5
GUARD = 256
TILE = 4096
LOOK_BACK = 512          # kMaxLookBack
TILE_STATE_BYTES = 20    # kScanTileStateBytes
RESULT_BYTES = 32        # kScanResultBytes
PULL_STRIDE = 48 * 256 * 16   # bytes one sweep of the pull kernels' grid moves


# ---- references -----------------------------------------------------------------------------------------------------

def slots_for(expected):
    s = 1
    while s < expected:
        s <<= 1
    return s


@functools.lru_cache(maxsize=None)
def oracle_scan(seg, expected):
    """(count, words, start positions as uint32, error text or None) of the oracle's ScanBuffer."""
    sb, err = orc.ScanBuffer(), None
    try:
        sb.process(seg, expected)
        count = expected
    except orc.OracleError as e:
        err = str(e)
        count = int(err.split("counted ")[1].split(",")[0])
    return count, sb.processed_scan_data(), np.frombuffer(sb.start_positions(), dtype=np.uint32).copy(), err


@functools.lru_cache(maxsize=None)
def kept_bytes(seg):
    """Output bytes in front of padding: every byte that is not FF, and one per FF 00 pair (a plain loop)."""
    kept, i, n = 0, 0, len(seg)
    while i < n:
        j = seg.find(b"\xff", i)
        if j < 0:
            kept += n - i
            break
        kept += j - i
        if j + 1 >= n:
            break                      # a lone FF at the end is dropped
        if seg[j + 1] == 0:
            kept += 1
        i = j + 2
    return kept


@functools.lru_cache(maxsize=None)
def flags(seg):
    """result[3].  Bit 1: some byte behind an FF is neither 00, D0..D7 nor FF.  Bit 0: some chunk start g (a multiple
    of 16, 512 < g < len) has the 512 bytes in front of it all FF."""
    a = np.frombuffer(seg, dtype=np.uint8)
    if a.size < 2:
        return 0
    ff = a == 0xFF
    ordinary = ff | (a == 0) | ((a & 0xF8) == 0xD0)
    out = 2 if bool(np.any(ff[:-1] & ~ordinary[1:])) else 0
    g = np.arange(LOOK_BACK + 16, a.size, 16)
    if g.size:
        c = np.concatenate(([0], np.cumsum(ff)))
        if bool(np.any(c[g] - c[g - LOOK_BACK] == LOOK_BACK)):
            out |= 1
    return out


def flags_brute(seg):
    out = 0
    for i in range(1, len(seg)):
        if seg[i - 1] == 0xFF and not (seg[i] in (0x00, 0xFF) or 0xD0 <= seg[i] <= 0xD7):
            out |= 2
    for g in range(0, len(seg), 16):
        if g > LOOK_BACK and all(b == 0xFF for b in seg[g - LOOK_BACK:g]):
            out |= 1
    return out


def parser_end(seg):
    """Where the reference's parser ends the entropy-coded segment (src/file.rs:163-201), None if it runs off the end."""
    pos, n = 0, len(seg)
    while True:
        while pos < n and seg[pos] != 0xFF:
            pos += 1
        offset = 1
        while pos + offset < n and seg[pos + offset] == 0xFF:
            offset += 1
        if pos + offset >= n:
            return None
        byte = seg[pos + offset]
        if byte == 0 or 0xD0 <= byte <= 0xD7:
            pos += offset + 1
        else:
            return pos + offset - 1


def wave_span(starts, nstarts, nwords, intervals, group=64):
    """max_wave_span (compeg_amd/csrc/desc.cpp): the widest stretch of words that `group` consecutive intervals cover."""
    best = 0
    for first in range(0, intervals, group):
        lo = int(starts[first]) if first < nstarts else 0
        after = first + group
        hi = int(starts[after]) if (after < intervals and after < nstarts) else nwords
        if hi > lo:
            best = max(best, hi - lo)
    return best


def wave_span_brute(starts, nstarts, nwords, intervals, group=64):
    """The same from its meaning: per wave, from where its first interval starts to where the next wave's does."""
    def start(i):
        return int(starts[i]) if i < nstarts else None
    best = 0
    for wave in range((intervals + group - 1) // group):
        lo = start(wave * group)
        lo = 0 if lo is None else lo
        nxt = (wave + 1) * group
        hi = start(nxt) if nxt < intervals else None
        hi = nwords if hi is None else hi
        best = max(best, hi - lo)
    return best


# ---- the matrix -----------------------------------------------------------------------------------------------------

class Image:
    def __init__(self, name, seg, expected=None, mis=0, fill=0, patch=False):
        self.name, self.seg, self.mis, self.fill, self.patch = name, bytes(seg), mis, fill, patch
        self.expected = oracle_scan(self.seg, 0)[0] if expected is None else expected   # None: the true count

    @property
    def slots(self):
        return slots_for(self.expected)


class Group:
    def __init__(self, name, images, skip=0, with_span=False, keep=False):
        self.name, self.images, self.skip, self.with_span, self.keep = name, images, skip, with_span, keep


class PullGroup:
    def __init__(self, name, sizes):
        self.name, self.sizes = name, sizes
        rng = np.random.default_rng(sum(sizes) + len(sizes))
        # (the source up to the next multiple of 16: what the pinned buffer holds there)
        self.data = [rng.integers(0, 256, (n + 15) // 16 * 16, dtype=np.uint8).tobytes() for n in sizes]


def plain(n, seed=0):
    """n bytes that are neither FF nor 00, all different from their neighbours."""
    return bytes(1 + (i * 7 + seed * 13) % 253 for i in range(n))


def _spread(images, every):
    """Misalignment and neighbours: image i lies at mis = i % 4 with FF or 00 around it, some have patch targets, and
    every `every`-th image runs at all eight combinations -- against the one reference, so neither may show."""
    out = []
    for i, im in enumerate(images):
        im.mis, im.fill, im.patch = i % 4, (0xFF, 0x00)[(i // 4) % 2], i % 3 == 0
        out.append(im)
        if i % every == 0:
            for mis in range(4):
                for fill in (0xFF, 0x00):
                    if (mis, fill) != (im.mis, im.fill):
                        out.append(Image(f"{im.name}@{mis}/{fill:02x}", im.seg, im.expected, mis, fill, not im.patch))
    return out


RUNS = list(range(1, 21)) + [31, 32, 33, 47, 48, 49, 255, 256, 257] + list(range(509, 531))
FOLLOW = {"00": b"\x00", "d0": b"\xd0", "d7": b"\xd7", "plain": b"\x41", "c0": b"\xc0", "d8": b"\xd8", "cf": b"\xcf", "none": b""}
ENDS = ("chunk-2", "chunk-1", "chunk+0", "chunk+1", "chunk+2", "seam", "start", "end")
TAIL = plain(5, 3) + b"\xff\xd1" + plain(3, 4)


def _prefix(n):
    p = bytearray(plain(n, 1))
    if n >= 6:
        p[1:3] = b"\xff\xd2"      # (the run's interval does not start at word 0)
    return bytes(p)


def _ladder_segment(run, end, follow):
    ff = b"\xff" * run
    if end == "start":
        return ff + follow + (TAIL if follow else b"")
    if end == "end":
        return _prefix(21) + ff + follow
    if end == "seam":
        at = TILE - (run + 1) // 2                 # run 1: the FF is the tile's last byte
    else:
        off = int(end[5:])
        at = (run + 3 + 15 - off) // 16 * 16 + off - run      # ends at 16 k + off, at least 3 bytes in front of it
    return _prefix(at) + ff + follow + (TAIL if follow else b"")   # (followed by nothing: the run ends the segment)


def _ladder(end):
    images = [Image(f"run{run}-{name}", _ladder_segment(run, end, follow)) for run in RUNS for name, follow in FOLLOW.items()]
    return Group(f"ladder[{end}]", _spread(images, 16), with_span=ENDS.index(end) % 2 == 0)


LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8191, 8192, 8193, 256 * 4096 - 1, 256 * 4096,
           256 * 4096 + 1, 257 * 4096 + 5)


def _length_segment(n, power_of_two):
    """Random bytes, an FF pair every 33 bytes or so (stuffing or RSTn in turn), and, unless the count is to be a power
    of two, a few FFs with whatever follows them."""
    rng = np.random.default_rng(1000 + n)
    a = rng.integers(0, 255, n, dtype=np.uint8)
    pos = np.arange(7, max(n - 8, 0), 33)
    pos = pos + rng.integers(0, 8, pos.size)
    marker = rng.random(pos.size) < 0.4
    if power_of_two:
        want = 1
        while want * 2 <= int(marker.sum()) + 1:
            want *= 2
        marker[np.flatnonzero(marker)[want - 1:]] = False     # want - 1 markers: want intervals
    else:
        a[rng.random(n) < 0.003] = 0xFF
    a[pos] = 0xFF
    a[pos + 1] = np.where(marker, 0xD0 + (np.cumsum(marker) - 1) % 8, 0)
    return a.tobytes()


def _length(n):
    seg = _length_segment(n, False)
    count = oracle_scan(seg, 0)[0]
    expected = [count, count - 1, count + 1, 0, 1]
    wrapped = max(1, count // 3)
    if slots_for(wrapped) < count:
        expected.append(wrapped)
    images = []
    for e in dict.fromkeys(e for e in expected if e >= 0):
        images.append(Image(f"expected{e}", seg, e))
    seg2 = _length_segment(n, True)
    count2 = oracle_scan(seg2, 0)[0]
    assert count2 & (count2 - 1) == 0 and oracle_scan(seg2, count2)[3] is None
    images.append(Image(f"power-of-two{count2}", seg2, count2))
    images = images[n % 4:] + images[:n % 4]       # (which of them runs at every misalignment varies with n)
    return Group(f"length[{n}]", _spread(images, len(images)), with_span=n % 2 == 1)


def _dense():
    images = []
    triple = b"".join(bytes([1 + i % 200, 0xFF, 0xD0]) for i in range(2731))
    for n in (4096, 4097, 8192):
        for tail in (0, 1, 2):
            images.append(Image(f"xx-ff-d0[{n}-tail{tail}]", triple[:n - tail] + b"\x41" * tail))
    images.append(Image("ff-d0", b"\xff\xd0" * 2048))
    images.append(Image("ff-00", b"\xff\x00" * 2048))
    images.append(Image("ff-00-shifted", b"\x41" + b"\xff\x00" * 2047 + b"\xff"))
    images.append(Image("ff-00-shifted-two-tiles", b"\x41" + b"\xff\x00" * 4095 + b"\xff"))
    images.append(Image("ff-ff", b"\xff" * 4096))                      # (a run beyond the look-back bound: bit 0)
    images.append(Image("ff-ff-short", b"\xff" * 512 + b"\x41" * 9))   # (the whole look-back and not a byte more)
    images.append(Image("ff-ff-pairs", b"\xff\xff\x41\x42" * 1030))
    images.append(Image("zeros", b"\x00" * 4101))
    images.append(Image("plain", plain(8197)))
    for first in (0, 1, 2, 3, 4):      # the 16-byte path of emit_kernel at every output shift, across a seam
        images.append(Image(f"plain-behind{first}", plain(first, 2) + b"\xff\xd0" + plain(8300, first)))
    return Group("dense", _spread(images, 1), with_span=True)


def _seam():
    images = []
    for at in (4094, 4095, 4096):
        for stuffed in range(4):      # `stuffed` FF 00 pairs in front: at - stuffed kept bytes
            front = bytearray(plain(at, at))
            for k in range(stuffed):
                front[40 * k + 5:40 * k + 7] = b"\xff\x00"
            for name, second in (("d3", b"\xd3"), ("00", b"\x00")):
                images.append(Image(f"ff@{at}-kept{(at - stuffed) % 4}-{name}", bytes(front) + b"\xff" + second + plain(9, 5)))
    return Group("seam", _spread(images, 1))


def _mixed():
    big = _length_segment(257 * 4096 + 5, False)
    two = _length_segment(8192, False)
    images = [
        Image("decoy-a", plain(5) + b"\xff\xd0" + plain(4), patch=True),      # descs[0], descs[1]: not launched
        Image("decoy-b", _length_segment(4097, False), mis=1, fill=0xFF),
        Image("empty", b"", 1, mis=2, fill=0xFF, patch=True),
        Image("one-byte", b"\x41", 1, mis=3),
        Image("one-tile", _length_segment(4096, False), mis=1, fill=0xFF, patch=True),
        Image("257-tiles", big, mis=3, fill=0xFF, patch=True),
        Image("two-tiles", two, oracle_scan(two, 0)[0] + 5, mis=2),
        Image("empty-expecting-3", b"", 3, fill=0xFF),
        Image("short", b"\x41\xff\xd0", mis=1, patch=True),
        Image("5000", _length_segment(5000, False), 17, mis=0, fill=0xFF),
    ]
    return Group("mixed", images, skip=2, with_span=True)


_REUSE_LENGTHS = (0, 17, 4097, 8192, 12000)


def _reuse(second):
    """Same lengths, slots and places both times; the second launch's output is shorter, so what the first one wrote
    lies behind it."""
    images = []
    for i, n in enumerate(_REUSE_LENGTHS):
        if second:
            seg = (b"\xff\x00" * n)[:n]
            if n > 100:
                seg = seg[:50] + b"\xff\xd4" + seg[52:]
        else:
            seg = b"".join(bytes([1 + k % 200, 0xFF, 0xD0 + k % 8]) for k in range(n // 3 + 1))[:n]
        images.append(Image(f"len{n}", seg, 4001, mis=i % 4, fill=(0xFF, 0)[i % 2], patch=i % 2 == 0))
    return Group(f"reuse[{'second' if second else 'first'}]", images, with_span=True, keep=second)


PULL_SIZES = (0, 1, 15, 16, 17, PULL_STRIDE - 16, PULL_STRIDE, PULL_STRIDE + 16)
PULL3_SIZES = {"one": (0, 17, 0), "two": (PULL_STRIDE + 16, 0, 15), "three": (1, PULL_STRIDE, PULL_STRIDE - 16),
               "three-small": (16, 33, 4096)}

BUILDERS = {}
for _end in ENDS:
    BUILDERS[f"ladder[{_end}]"] = functools.partial(_ladder, _end)
for _n in LENGTHS:
    BUILDERS[f"length[{_n}]"] = functools.partial(_length, _n)
BUILDERS["dense"] = _dense
BUILDERS["seam"] = _seam
BUILDERS["mixed"] = _mixed
BUILDERS["reuse[first]"] = functools.partial(_reuse, False)   # (these two stay next to each other, in this order)
BUILDERS["reuse[second]"] = functools.partial(_reuse, True)
for _n in PULL_SIZES:
    BUILDERS[f"pull[{_n}]"] = functools.partial(PullGroup, f"pull[{_n}]", (_n,))
for _name, _sizes in PULL3_SIZES.items():
    BUILDERS[f"pull3[{_name}]"] = functools.partial(PullGroup, f"pull3[{_name}]", _sizes)
GROUP_NAMES = tuple(BUILDERS)
SCAN_GROUP_NAMES = tuple(n for n in GROUP_NAMES if not n.startswith("pull"))
SMALL_GROUP_NAMES = tuple(n for n in SCAN_GROUP_NAMES if not (n.startswith("length[10") or n == "mixed"))


@functools.lru_cache(maxsize=None)
def group(name):
    g = BUILDERS[name]()
    assert g.name == name
    return g


# ---- the harness's files --------------------------------------------------------------------------------------------

def write_cases(path, names):
    with open(path, "wb") as f:
        f.write(struct.pack("<II", MAGIC, len(names)))
        for name in names:
            g = group(name)
            if isinstance(g, PullGroup):
                f.write(struct.pack("<II", 1 if len(g.sizes) == 1 else 2, len(g.sizes)))
                for n, data in zip(g.sizes, g.data):
                    f.write(struct.pack("<I", n) + data)
                continue
            f.write(struct.pack("<IIIII", 0, len(g.images), g.skip, int(g.with_span), int(g.keep)))
            for im in g.images:
                f.write(struct.pack("<IIIIII", len(im.seg), im.expected, im.slots, im.mis, im.fill, int(im.patch)))
                f.write(im.seg + b"\x00" * (-len(im.seg) % 4))


def read_result(path):
    """(rows of 10 words, the arena) of one launch."""
    raw = np.fromfile(path, dtype=np.uint8)
    magic, _kind, arena_bytes, rows = (int(v) for v in raw[:16].view(np.uint32))
    assert magic == MAGIC and raw.size == 16 + 40 * rows + arena_bytes, "result file damaged"
    return raw[16:16 + 40 * rows].view(np.uint32).reshape(rows, 10).astype(np.int64), raw[16 + 40 * rows:]


def _check_layout(regions, arena_bytes):
    """Every output at its documented size and the runtime's alignment, at least GUARD bytes clear of the next."""
    end = 0
    for off, size, align, what in sorted(regions):
        assert off % align == 0, f"{what}: offset {off} not aligned to {align}"
        assert off - end >= GUARD, f"{what}: less than {GUARD} guard bytes in front of it"
        end = off + size
    assert arena_bytes - end >= GUARD, "less than a guard behind the last output"


def _put_u32(buf, at, values):
    v = np.asarray(values, dtype="<u4")
    buf[at:at + 4 * v.size] = v.view(np.uint8)


def check_scan(g, rows, arena, before=None):
    """What one launch of group g left in its arena against the references; `before`: the arena as the launch found
    it (keep).  Everything the references do not name must be as it was: padding, unused slots, result[5..7], the
    outputs of images that were not launched, every guard."""
    assert len(rows) == len(g.images)
    if g.keep:
        want = before.copy()
    else:
        want = np.full(arena.size, PREFILL, dtype=np.uint8)
    compare = np.ones(arena.size, dtype=bool)
    regions = []
    for im, row in zip(g.images, rows):
        o_tile, n_tile, o_starts, n_starts, o_words, n_words, o_res, n_res, o_patch, n_patch = (int(v) for v in row)
        n = len(im.seg)
        assert n_tile == (n + TILE - 1) // TILE * TILE_STATE_BYTES and n_starts == 4 * im.slots, im.name
        assert n_words == n + n // 3 + 4 and n_res == RESULT_BYTES and n_patch == (8 if im.patch else 0), im.name
        regions += [(o_tile, n_tile, 256, f"{im.name}: tile_state"), (o_starts, n_starts, 256, f"{im.name}: starts_out"),
                    (o_words, n_words, 256, f"{im.name}: words_out"), (o_res, n_res, 32, f"{im.name}: result")]
        if im.patch:
            regions.append((o_patch, 8, 256, f"{im.name}: patch targets"))
        _put_u32(want, o_res + 12, [0])      # (flags are OR-ed in: the caller clears them before every launch)
    _check_layout(regions, arena.size)
    for im, row in list(zip(g.images, rows))[g.skip:]:
        o_tile, n_tile, o_starts, n_starts, o_words, n_words, o_res, n_res, o_patch, n_patch = (int(v) for v in row)
        compare[o_tile:o_tile + n_tile] = False          # scratch
        flag = flags(im.seg)
        _put_u32(want, o_res + 12, [flag])
        if flag & 1:
            # an FF run beyond the look-back bound: the host takes the image over, only flags and guards are specified
            for off, size in ((o_starts, n_starts), (o_words, n_words), (o_res, 12), (o_res + 16, 4), (o_patch, n_patch)):
                compare[off:off + size] = False
            continue
        count, words, starts, _ = oracle_scan(im.seg, im.expected)
        nwords, nstarts = len(words) // 4, min(count, im.slots)
        assert len(words) % 4 == 0 and len(words) <= n_words and starts.size == nstarts
        _put_u32(want, o_res, [count, kept_bytes(im.seg), nwords])
        if g.with_span:
            _put_u32(want, o_res + 16, [wave_span(starts, nstarts, nwords, im.expected)])
        want[o_words:o_words + len(words)] = np.frombuffer(words, dtype=np.uint8)
        _put_u32(want, o_starts, starts)
        if im.patch:
            _put_u32(want, o_patch, [nwords, nstarts])
    bad = np.flatnonzero((arena != want) & compare)
    if bad.size:
        lines = []
        for at in bad[:12]:
            at = int(at)
            where = next((f"{what} + {at - off}" for off, size, _, what in regions if off <= at < off + size), None)
            if where is None:
                off, size, _, what = min(regions, key=lambda r: min(abs(at - r[0]), abs(at - r[0] - r[1])))
                where = f"guard of {what} ({at - off - size} behind its end)" if at >= off + size else f"guard of {what} ({off - at} in front of it)"
            lines.append(f"{where}: {int(arena[at]):02x}, want {int(want[at]):02x}")
        raise AssertionError(f"{g.name}: {bad.size} bytes differ\n" + "\n".join(lines))


def check_pull(g, rows, arena):
    """Exact copies; up to the next multiple of 16 the destination holds what the source held there or is untouched;
    nothing else is written."""
    want = np.full(arena.size, PREFILL, dtype=np.uint8)
    compare = np.ones(arena.size, dtype=bool)
    regions = []
    assert len(rows) == len(g.sizes)
    for k, (n, data, row) in enumerate(zip(g.sizes, g.data, rows)):
        off, size = int(row[0]), int(row[1])
        assert size == (n + 15) // 16 * 16
        regions.append((off, size, 16, f"segment {k}"))
        src = np.frombuffer(data, dtype=np.uint8)
        want[off:off + n] = src[:n]
        tail = arena[off + n:off + size]
        compare[off + n:off + size] = ~((tail == src[n:size]) | (tail == PREFILL))   # (either is within the contract)
    _check_layout(regions, arena.size)
    bad = np.flatnonzero((arena != want) & compare)
    assert bad.size == 0, f"{g.name}: {bad.size} bytes differ, the first at arena offset {int(bad[0])} (segments at {[r[0] for r in regions]})"
