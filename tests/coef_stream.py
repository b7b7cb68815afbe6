"""Baseline JPEGs written from coefficients, and what the reference must make of them.  A plain module (Python and
numpy, no fixtures), shared by tests/test_coef_stream.py (the oracle and the host front end), tests/test_coef_emulation.py
(the emulated kernel bodies) and tests/test_gpu_coef.py (the card).

tools/synth.py's frames are pictures put through a forward DCT, a quantiser and the two standard Huffman tables: they
never hold an AC magnitude above 10 bits, a code of 16 bits in front of 15 magnitude bits, a run symbol without
magnitude bits, a chroma sample outside RGB's gamut.  A Frame here is the entropy-coded stream itself: per data unit, in
scan order, a DC difference and a list of AC symbols (run, size, magnitude bits), with explicit ZRL and EOB entries, under
Huffman tables given as symbol -> code length.  write() packs it (canonical codes, ones behind a segment's last bit,
FF 00 stuffing, RST markers, EOI); predict() says which dequantised coefficients the reference keeps of it: ZRL
advances 17 positions (quirk Q2; 16 with standard_entropy), positions >= 32 are dropped (Q3), the DC predictor and both
dequantising products wrap at 32 bits, and in front of a DC code the reader is not topped up (Q1): where it holds fewer
bits than the code and its magnitude need, it runs dry and the rest of the restart interval decodes from the bits it
still had and zeros behind them.  rgba() is a numpy float32 restatement of the reference's IDCT and colour step
(oracle/compeg_oracle.c: orc_dct_pass, orc_finalize_pass) with the mutants the cases have to tell from it.

cases() names the frames; every name says family, tables, layout and entropy mode."""
from dataclasses import dataclass, field

import numpy as np

LAYOUTS = {"422": (2, 1), "444": (1, 1), "440": (1, 2), "420": (2, 2)}   # (as tests/route_matrix.py has them)
RETAINED = 32
EOB = (0, 0, 0)
ZRL = (15, 0, 0)
ZIGZAG = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31,
                   40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61,
                   35, 36, 48, 49, 57, 58, 62, 63])   # [row * 8 + col] -> zig-zag position


def mag(v):
    """(size, magnitude bits) of a signed value: T.81 F.1.2.1."""
    size = abs(int(v)).bit_length()
    return size, (v if v > 0 else v + (1 << size) - 1)


def ac(run, v):
    """The AC symbol of `run` zeros and then the level v."""
    size, bits = mag(v)
    assert 0 <= run <= 15 and 1 <= size <= 15
    return (run, size, bits)


def extend(bits, size):
    return bits if size == 0 or bits >= 1 << (size - 1) else bits - (1 << size) + 1


def wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


@dataclass
class Frame:
    name: str
    layout: str
    mcus_w: int
    mcus_h: int
    dus: list                      # (DC difference, [AC symbols]) per data unit, scan order, every MCU of the frame
    huff: dict                     # table slot (0: DC 0, 1: AC 0, 2: DC 1, 3: AC 1) -> {symbol: code length}
    ri: int = 0
    quant: tuple = (1, 1)          # a value for all 64 positions, or 64 values in zig-zag order, per table
    sel: tuple = ((0, 0, 0), (1, 1, 1), (1, 1, 1))   # (Td, Ta, Tq) of Y, Cb, Cr
    standard: bool = False
    family: str = ""
    tables: str = ""
    _jpeg: bytes = field(default=None, repr=False)

    @property
    def sampling(self):
        return LAYOUTS[self.layout]

    @property
    def dus_per_mcu(self):
        return self.sampling[0] * self.sampling[1] + 2

    @property
    def comp_of_du(self):
        return [0] * (self.sampling[0] * self.sampling[1]) + [1, 2]

    @property
    def mcus(self):
        return self.mcus_w * self.mcus_h

    @property
    def w(self):
        return self.mcus_w * 8 * self.sampling[0]

    @property
    def h(self):
        return self.mcus_h * 8 * self.sampling[1]

    @property
    def interval(self):
        return self.ri or self.mcus

    @property
    def intervals(self):
        return self.mcus // self.interval

    def qtable(self, t):
        q = self.quant[t]
        return np.full(64, q, dtype=np.int64) if np.isscalar(q) else np.asarray(q, dtype=np.int64)

    def image_kw(self):
        return dict(allow_sampling=self.layout != "422", standard_entropy=self.standard)

    def jpeg(self):
        if self._jpeg is None:
            self._jpeg = write(self)
        return self._jpeg


# ---- Huffman tables ---------------------------------------------------------------------------------------------------

def canonical(lengths):
    """{symbol: length} -> (BITS, HUFFVAL, {symbol: (code, length)}): symbols of one length in the dict's order."""
    order = sorted(lengths, key=lambda s: lengths[s])   # (stable)
    bits = [sum(1 for s in order if lengths[s] == n) for n in range(1, 17)]
    codes, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            codes[order[k]] = (code, n)
            code += 1
            k += 1
        code <<= 1
    kraft = sum(2.0 ** -n for n in lengths.values())
    assert kraft < 1.0, "a full table would hold the all-ones code"
    assert all(1 <= n <= 16 for n in lengths.values())
    return bits, order, codes


def table(kind, symbols):
    """One of the three table sets over `symbols`: `short` at codes of at most 8 bits (L1 only), `edge` at 9, 10, 11 and
    12 bits in turn (the two sides of kDcFastBits = 9 and kFastBits = 11), `long` at 16 bits (every one escapes to the
    two-level tables)."""
    symbols = list(dict.fromkeys(symbols))
    if kind == "short":
        n = max(2, len(symbols).bit_length())   # 2^n > len
        assert n <= 8
        return {s: n for s in symbols}
    if kind == "edge":
        return {s: 9 + i % 4 for i, s in enumerate(symbols)}
    assert kind == "long"
    return {s: 16 for s in symbols}


def table_set(kind, dc_symbols, ac_symbols):
    if kind in WIDE_KINDS:
        return wide_table_set(kind, dc_symbols, ac_symbols)
    dc, act = table(kind, dc_symbols), table(kind, ac_symbols)
    return {0: dc, 1: act, 2: dict(dc), 3: dict(act)}


# ---- tables that outgrow their share of LDS ------------------------------------------------------------------------------

# The host (compeg_amd/csrc/front.cpp: HuffmanLut::build) gives every 8-bit prefix that begins a code of more than 8 bits
# one L2 block of 256 entries and concatenates the blocks of Th0 DC, Th0 AC, Th1 DC, Th1 AC; the kernels stage them in LDS
# behind L1, and behind them the two direct AC tables of kFastEntries entries each (front.h).  The planners stage at most
# LDS_SHARE entries (kernels.hip: plan_huffman, plan_stream, plan_walk: `12288u`).  Hence the three regimes of a file:
L2_BLOCK = 256
FAST_ENTRIES = 2048                          # front.h: kFastEntries = 1 << kFastBits
LDS_SHARE = 12288                            # kernels.hip: plan_huffman's l2_entries_in_lds cap
ALL_STAGED = LDS_SHARE - 2 * FAST_ENTRIES    # 8192: L2 and both direct tables fit -- the fast entropy mode (fast_tables_usable)
INDEX_SPACE = 1 << 15                        # the delegate index has 15 bits: 128 blocks in all (front.cpp: ImageData::parse)


def l2_blocks(lengths):
    """The L2 blocks HuffmanLut::build makes of {symbol: length}: the distinct 8-bit prefixes of the longer codes."""
    return len({code >> (n - 8) for (code, n) in canonical(lengths)[2].values() if n > 8})


def regime_of(entries):
    """A: everything staged, the fast mode on.  B: all of L2 staged, the direct tables in part, the fast mode off.  C: L2
    lookups at and beyond LDS_SHARE come from global memory."""
    return "A" if entries <= ALL_STAGED else "B" if entries <= LDS_SHARE else "C"


def table_regime(f):
    """-> dict(blocks=[Th0 DC, Th0 AC, Th1 DC, Th1 AC], first=[each table's first L2 entry], entries, regime)."""
    blocks = [l2_blocks(f.huff[t]) for t in range(4)]
    first = [L2_BLOCK * sum(blocks[:t]) for t in range(4)]
    entries = L2_BLOCK * sum(blocks)
    return dict(blocks=blocks, first=first, entries=entries, regime=regime_of(entries))


def entry_of(f, t, symbol):
    """The L2 entry index of the symbol's code in table slot t (its first, where the code is shorter than 16 bits); None
    for a code of at most 8 bits."""
    codes = canonical(f.huff[t])[2]
    code, n = codes[symbol]
    if n <= 8:
        return None
    prefixes = sorted({c >> (m - 8) for (c, m) in codes.values() if m > 8})
    return table_regime(f)["first"][t] + L2_BLOCK * prefixes.index(code >> (n - 8)) + ((code << (16 - n)) & 0xFF)


# kind -> (blocks up to the end of Th0 AC, blocks in all).  The DC tables hold categories 0..15 only (a higher one closes
# the cooperative kernel and the walk: desc.cpp, fill_coop / mcu_ok), so they come to 4 blocks each or fewer and the AC
# tables make up the rest.
WIDE_KINDS = {
    "wide_a": (16, 32),      # 8192 entries: the last file of regime A
    "wide_b": (18, 36),      # 9216: the direct tables staged in part
    "wide_b48": (24, 48),    # 12288: the last file of regime B -- L2 fills the share, nothing of the direct tables
    "wide_c": (48, 92),      # Th0 AC ends at entry 12288: wholly staged; Th1 DC and Th1 AC wholly beyond
    "wide_c2": (64, 88),     # entry 12288 lies inside Th0 AC: one table read from both places
    "full": (64, 128),       # 32768 entries: the last file the parser accepts
    "over": (64, 129),       # one block more: refused
}
_DC_BLOCKS = 4
_TAIL = (10, 11, 12, 13, 14, 15, 16)


def _wide_lengths(used, universe, n9):
    """used symbols dealt in turn to four groups -- codes of at most 8 bits, the first of the 9-bit codes, the last of them,
    a tail of one code each of 10 .. 16 bits -- and symbols the stream never uses filling the 9-bit codes up to n9 and the
    tail up to seven.  canonical() keeps this order within a length: the used 9-bit codes stand at both ends of the
    table's blocks, the tail in its last one.  None: the universe has too few symbols."""
    used = list(dict.fromkeys(used))
    spare = [s for s in universe if s not in used]
    lo_cap = (n9 + 1) // 2
    groups = {"short": [], "lo": [], "hi": [], "tail": []}
    cap = {"short": len(used), "lo": lo_cap, "hi": n9 - lo_cap, "tail": len(_TAIL)}
    turn = ["short", "lo", "hi", "tail"]
    k = 0
    for s in used:
        while len(groups[turn[k % 4]]) >= cap[turn[k % 4]]:
            k += 1
        groups[turn[k % 4]].append(s)
        k += 1
    fill = n9 - len(groups["lo"]) - len(groups["hi"]) + len(_TAIL) - len(groups["tail"])
    if fill > len(spare):
        return None
    pad9 = [spare.pop(0) for _ in range(n9 - len(groups["lo"]) - len(groups["hi"]))]
    groups["tail"] += [spare.pop(0) for _ in range(len(_TAIL) - len(groups["tail"]))]
    long_mass = n9 / 512 + sum(2.0 ** -n for n in _TAIL)
    ns = next((n for n in range(1, 9) if len(groups["short"]) * 2.0 ** -n + long_mass < 1.0), None)
    if ns is None:
        return None
    out = {s: ns for s in groups["short"]}
    out.update({s: 9 for s in groups["lo"] + pad9 + groups["hi"]})
    out.update(dict(zip(groups["tail"], _TAIL)))
    return out


def wide_table(used, universe, blocks):
    """{symbol: length} over the used symbols and padding from `universe` with exactly `blocks` L2 blocks; with too few
    symbols for that (a DC table of sixteen categories), as many as they make."""
    best = None
    for n9 in range(0, 2 * blocks + 1):
        t = _wide_lengths(used, universe, n9)
        if t is None:
            break
        best = t
        if l2_blocks(t) == blocks:
            return t
    assert best is not None and universe is not _AC_UNIVERSE, (blocks, len(list(used)))
    return best


_AC_UNIVERSE = tuple(range(256))
_DC_UNIVERSE = tuple(range(16))


def wide_table_set(kind, dc_symbols, ac_symbols):
    th0_end, total = WIDE_KINDS[kind]
    dc0 = wide_table(dc_symbols, _DC_UNIVERSE, _DC_BLOCKS)
    ac0 = wide_table(ac_symbols, _AC_UNIVERSE, th0_end - l2_blocks(dc0))
    dc1 = dict(dc0)
    ac1 = wide_table(ac_symbols, _AC_UNIVERSE, total - th0_end - l2_blocks(dc1))
    return {0: dc0, 1: ac0, 2: dc1, 3: ac1}


def symbols_of(dus):
    dcs = sorted({abs(int(d)).bit_length() for d, _ in dus})
    acs = sorted({r << 4 | s for _, syms in dus for (r, s, _) in syms})
    return dcs, acs


# ---- the writer -------------------------------------------------------------------------------------------------------

class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, n):
        self.acc = self.acc << n | (value & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            self.n -= 8
            self.out.append(self.acc >> self.n & 0xFF)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)   # ones behind the segment's last bit
        out, self.out = bytes(self.out), bytearray()
        return out


def _segments(f):
    """The unstuffed bytes of every restart interval's entropy-coded segment (the trailing MCUs no complete interval
    covers are coded too, as one more segment)."""
    codes = {t: canonical(l)[2] for t, l in f.huff.items()}
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    assert len(f.dus) == f.mcus * dpm, (f.name, len(f.dus), f.mcus * dpm)
    segs = []
    for first in range(0, f.mcus, f.interval):
        b, nbits = _Bits(), 0
        for du in range(first * dpm, min(first + f.interval, f.mcus) * dpm):
            td, ta, _ = f.sel[comps[du % dpm]]
            diff, syms = f.dus[du]
            size, bits = mag(diff)
            b.put(*codes[2 * td][size])
            b.put(bits, size)
            for (r, s, mbits) in syms:
                assert 0 <= mbits < 1 << s if s else mbits == 0
                b.put(*codes[2 * ta + 1][r << 4 | s])
                b.put(mbits, s)
        segs.append(b.flush())
    return segs


def symbol_bits(f):
    """(symbol, first bit within its restart interval's segment, code bits, magnitude bits) of everything write() codes:
    symbol "dc" for a DC code, else the AC symbol's byte."""
    codes = {t: canonical(l)[2] for t, l in f.huff.items()}
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    out = []
    for first in range(0, f.mcus, f.interval):
        at = 0
        for du in range(first * dpm, min(first + f.interval, f.mcus) * dpm):
            td, ta, _ = f.sel[comps[du % dpm]]
            size = mag(f.dus[du][0])[0]
            out.append(("dc", at, codes[2 * td][size][1], size))
            at += codes[2 * td][size][1] + size
            for (r, s, _) in f.dus[du][1]:
                out.append((r << 4 | s, at, codes[2 * ta + 1][r << 4 | s][1], s))
                at += codes[2 * ta + 1][r << 4 | s][1] + s
    return out


def write(f):
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    out = bytearray(b"\xff\xd8")
    for t in range(len(f.quant)):
        q = f.qtable(t)
        assert q.min() >= 1 and q.max() <= 255
        out += seg(0xDB, bytes([t]) + bytes(int(x) for x in q))
    hs, vs = f.sampling
    out += seg(0xC0, bytes([8]) + f.h.to_bytes(2, "big") + f.w.to_bytes(2, "big") + bytes([3])
               + bytes([1, hs << 4 | vs, f.sel[0][2], 2, 0x11, f.sel[1][2], 3, 0x11, f.sel[2][2]]))
    for t in sorted(f.huff):
        bits, vals, _ = canonical(f.huff[t])
        out += seg(0xC4, bytes([(t & 1) << 4 | t >> 1]) + bytes(bits) + bytes(vals))
    if f.ri:
        out += seg(0xDD, f.ri.to_bytes(2, "big"))
    out += seg(0xDA, bytes([3, 1, f.sel[0][0] << 4 | f.sel[0][1], 2, f.sel[1][0] << 4 | f.sel[1][1],
                            3, f.sel[2][0] << 4 | f.sel[2][1], 0, 63, 0]))
    segs = _segments(f)
    for i, s in enumerate(segs):
        out += s.replace(b"\xff", b"\xff\x00")
        if i + 1 < len(segs):
            out += bytes([0xFF, 0xD0 + i % 8])
    return bytes(out + b"\xff\xd9")


# ---- what the reference makes of a frame ------------------------------------------------------------------------------

def _lookup(by_code, window16):
    for (code, n), sym in by_code.items():
        if window16 >> (16 - n) == code:
            return n, sym
    return 0, 0   # (no such code: the tables' entry is zero -- nothing consumed, symbol 0)


class _Reader:
    """The reference's bit reader, state for state (src/huffman.wgsl: u32 arithmetic wraps, shift counts modulo 32,
    words beyond the buffer read as zero): what it does once it has run dry is part of the stream's meaning."""
    M = 0xFFFFFFFF

    def __init__(self, words, start):
        self.words, self.next_word, self.cur, self.nxt, self.left = words, start, 0, 0, 0
        self.refill()

    def refill(self):
        if self.left < 32:
            w = self.words[self.next_word] if self.next_word < len(self.words) else 0
            self.next_word += 1
            self.cur |= w >> (self.left & 31)
            self.nxt = (((w << 1) & self.M) << ((31 - self.left) & 31)) & self.M
            self.left += 32

    def take(self, n):
        """peek(n), then consume(n)."""
        v = (self.cur >> 1) >> ((31 - n) & 31)
        self.cur = ((self.cur << (n & 31)) & self.M) | ((self.nxt >> 1) >> ((31 - n) & 31))
        self.nxt = (self.nxt << (n & 31)) & self.M
        self.left = (self.left - n) & self.M
        return v

    def symbol(self, by_code):
        n, sym = _lookup(by_code, self.cur >> 16)
        self.take(n)
        return sym


def _words(segs):
    """The preprocessed scan: every segment from a word boundary, zeros behind it; and each segment's first word."""
    words, starts = [], []
    for s in segs:
        starts.append(len(words))
        s = s + bytes(-len(s) % 4)
        words += [int.from_bytes(s[i:i + 4], "big") for i in range(0, len(s), 4)]
    return words, starts


def predict(f, standard=None, retained=RETAINED, zrl=None, saturate=False, facts=None):
    """The dequantised coefficients the reference keeps: int32 [data units of the complete intervals, 64], positions
    >= `retained` zero.  standard / zrl / retained / saturate: the mutants' knobs (a ZRL advance, a Q3 cut, AC products
    saturated to 16 bits in place of wrapping).

    Every interval is followed symbol by symbol, counting the bits the reference's reader holds (`left`: 32 more whenever
    it is topped up below 32 -- in front of every AC symbol, in front of a DC code with standard_entropy only).  An
    interval in which a DC code and its magnitude need more than it holds there (quirk Q1) is decoded again by _Reader,
    the reader's own arithmetic: from that code on it sees what it still held and zeros.

    facts: a dict that receives what the cases' edges are made of -- `left_at_dc` (the set of counts in front of DC
    codes), `underflow_left` (the counts at which the reader ran dry), `dry` (data units decoded from a dry reader),
    `max_symbol_bits` (code + magnitude), `max_pred_q` (the largest |predictor x quantiser| before the wrap)."""
    standard = f.standard if standard is None else standard
    mutated = zrl is not None   # (a data unit then may not end where its symbols do: what is there is taken, no more)
    zrl = (16 if standard else 17) if zrl is None else zrl
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    codes = {t: canonical(l)[2] for t, l in f.huff.items()}
    by_code = {t: {v: k for k, v in c.items()} for t, c in codes.items()}
    q = [f.qtable(f.sel[c][2]) for c in range(3)]
    out = np.zeros((f.intervals * f.interval * dpm, 64), dtype=np.int64)
    facts = {} if facts is None else facts
    facts.update(left_at_dc=set(), underflow_left=set(), dry=0, max_symbol_bits=0, max_pred_q=0)
    words, starts = _words(_segments(f))

    def store(du, comp, pos, level):
        if pos < retained:
            v = level * int(q[comp][pos])
            out[du, pos] = max(-32768, min(32767, v)) if saturate else wrap32(v)

    def dc(du, comp, pred, diff):
        pred[comp] = wrap32(pred[comp] + diff)
        facts["max_pred_q"] = max(facts["max_pred_q"], abs(pred[comp]) * int(q[comp][0]))
        out[du, 0] = wrap32(pred[comp] * int(q[comp][0]))

    def by_symbols(iv):
        """-> the data unit at whose DC code the reader runs dry, or None."""
        pred, left = [0, 0, 0], 32
        for du in range(iv * f.interval * dpm, (iv + 1) * f.interval * dpm):
            comp = comps[du % dpm]
            td, ta, _ = f.sel[comp]
            diff, syms = f.dus[du]
            size, _ = mag(diff)
            n = codes[2 * td][size][1]
            if standard and left < 32:
                left += 32
            facts["left_at_dc"].add(left)
            if left < n + size:
                facts["underflow_left"].add(left)
                return du
            left -= n + size
            facts["max_symbol_bits"] = max(facts["max_symbol_bits"], n + size)
            dc(du, comp, pred, diff)
            pos, k = 1, 0
            while pos < 64:
                if mutated and k == len(syms):
                    break
                assert k < len(syms), f"{f.name}: data unit {du} ends at position {pos} without EOB"
                r, s, bits = syms[k]
                k += 1
                n = codes[2 * ta + 1][r << 4 | s][1]
                left += 32 if left < 32 else 0
                left -= n + s
                facts["max_symbol_bits"] = max(facts["max_symbol_bits"], n + s)
                if (r, s) == (0, 0):
                    break
                if (r, s) == (15, 0):
                    pos += zrl
                    continue
                pos += r
                store(du, comp, pos, extend(bits, s))
                pos += 1
            assert mutated or k == len(syms), f"{f.name}: data unit {du} has symbols behind its end"
        return None

    def by_reader(iv):
        pred, b = [0, 0, 0], _Reader(words, starts[iv])
        for du in range(iv * f.interval * dpm, (iv + 1) * f.interval * dpm):
            comp = comps[du % dpm]
            td, ta, _ = f.sel[comp]
            out[du] = 0
            if standard:
                b.refill()
            size = b.symbol(by_code[2 * td])
            dc(du, comp, pred, extend(b.take(size), size))
            pos = 1
            while pos < 64:
                b.refill()
                rs = b.symbol(by_code[2 * ta + 1])
                if rs == 0:
                    break
                if rs == 0xF0:
                    pos += zrl
                    continue
                pos += rs >> 4
                store(du, comp, pos, extend(b.take(rs & 15), rs & 15))
                pos += 1

    for iv in range(f.intervals):
        dry_at = by_symbols(iv)
        if dry_at is not None:
            facts["dry"] += (iv + 1) * f.interval * dpm - dry_at
            by_reader(iv)
    return out.astype(np.int32)


# ---- the reference's IDCT and colour step, restated in numpy float32 ------------------------------------------------

_SCALE = np.array([1.0, 1.387039845, 1.306562965, 1.175875602, 1.0, 0.785694958, 0.541196100, 0.275899379], dtype=np.float32)
_C1414, _C1847, _C1082, _C2613 = (np.float32(c) for c in (1.414213562, 1.847759065, 1.082392200, 2.613125930))
MUTANTS = ("fma_rows", "round_nearest", "saturate16", "logical_shift", "cut31", "cut33", "zrl16")


def _msub(a, b, c, fused):
    """a * b - c, every step rounded to f32; fused: contracted to one rounding."""
    if fused:
        return (a.astype(np.float64) * np.float64(b) - c.astype(np.float64)).astype(np.float32)
    return a * b - c


def _nmsub(c, a, b, fused):
    """c - a * b."""
    if fused:
        return (c.astype(np.float64) - a.astype(np.float64) * np.float64(b)).astype(np.float32)
    return c - a * b


def _aan(i, bias, fused):
    """One pass of the reference's transform on i[0..7] (arrays): orc_dct_pass, statement by statement."""
    z5 = i[0] + bias if bias is not None else i[0]
    tmp10, tmp11 = z5 + i[4], z5 - i[4]
    tmp13 = i[2] + i[6]
    tmp12 = _msub(i[2] - i[6], _C1414, tmp13, fused)
    t0, t3, t1, t2 = tmp10 + tmp13, tmp10 - tmp13, tmp11 + tmp12, tmp11 - tmp12
    z13, z10, z11, z12 = i[5] + i[3], i[5] - i[3], i[1] + i[7], i[1] - i[7]
    t7 = z11 + z13
    t11 = (z11 - z13) * _C1414
    z5o = (z10 + z12) * _C1847
    t10 = _nmsub(z5o, z12, _C1082, fused)
    t12 = _nmsub(z5o, z10, _C2613, fused)
    t6 = t12 - t7
    t5 = t11 - t6
    t4 = t10 - t5
    return [t0 + t7, t1 + t6, t2 + t5, t3 + t4, t3 - t4, t2 - t5, t1 - t6, t0 - t7]


def samples(coef, mutant=None):
    """int32 [n, 64] dequantised coefficients (zig-zag order) -> uint8 [n, 8, 8] samples."""
    grid = coef[:, ZIGZAG].reshape(-1, 8, 8).astype(np.float32)          # (float)cv: to nearest
    grid = grid * (_SCALE[:, None] * _SCALE[None, :])                      # mul = SCALE[row] * SCALE[col], one f32 product
    cols = _aan([grid[:, r, :] * np.float32(0.125) for r in range(8)], None, False)       # lane = column; [row] -> [n, col]
    ws = np.stack(cols, axis=1)                                            # [n, row, col]
    rows = _aan([ws[:, :, c] for c in range(8)], np.float32(128.5), mutant == "fma_rows")
    px = np.stack(rows, axis=2)
    px = np.minimum(np.maximum(px, np.float32(0)), np.float32(255))
    return (np.rint(px) if mutant == "round_nearest" else np.trunc(px)).astype(np.uint8)


def rgba(f, coef, mutant=None):
    """The frame's output from predicted coefficients [data units, 64]: orc_finalize_pass."""
    hs, vs = f.sampling
    dpm = f.dus_per_mcu
    smp = samples(coef, mutant)
    mcus = smp.shape[0] // dpm
    smp = smp.reshape(mcus, dpm, 8, 8)
    H, W = f.mcus_h * 8 * vs, f.mcus_w * 8 * hs
    planes = np.zeros((3, H, W), dtype=np.int32)
    alpha = np.zeros((H, W), dtype=np.uint8)
    for m in range(mcus):
        my, mx = divmod(m, f.mcus_w)
        y = np.block([[smp[m, v * hs + h] for h in range(hs)] for v in range(vs)])
        sl = (slice(my * 8 * vs, (my + 1) * 8 * vs), slice(mx * 8 * hs, (mx + 1) * 8 * hs))
        planes[0][sl] = y
        for c in (1, 2):
            planes[c][sl] = np.repeat(np.repeat(smp[m, hs * vs + c - 1], vs, axis=0), hs, axis=1)
        alpha[sl] = 255
    yy, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    def sh(v, n):
        if mutant == "logical_shift":
            return ((v.astype(np.int64) & 0xFFFFFFFF) >> n).astype(np.int32)
        return v >> n   # arithmetic (quirk Q5)
    r = yy + sh(45 * cr, 5)
    g = yy - sh(11 * cb + 23 * cr, 5)
    b = yy + sh(113 * cb, 6)
    out = np.stack([np.clip(r, 0, 255), np.clip(g, 0, 255), np.clip(b, 0, 255), alpha], axis=2).astype(np.uint8)
    out[alpha == 0] = 0
    return out[:f.h, :f.w]


def expectation(f, mutant=None):
    """The frame's RGBA by the restatement; with a mutant, by the restatement gone wrong in that one way."""
    kw = {"cut31": dict(retained=31), "cut33": dict(retained=33), "zrl16": dict(zrl=16), "saturate16": dict(saturate=True)}
    return rgba(f, predict(f, **kw.get(mutant, {})), mutant)


# ---- the frames -------------------------------------------------------------------------------------------------------

FLAT = (0, [EOB])
ENTROPY_FAMILIES = ("ac_sizes", "dc_cats", "dc_hostile", "q1_underflow", "positions", "run_size0", "pairs")
ARITHMETIC_FAMILIES = ("basis", "dc_sweep", "gamut", "saturated", "dc_wrap", "random_dense", "texture", "cancel")


def _place(dus, huff, sel, layout, ri, standard, fit, absolute):
    """The data units in their order, DC values turned into differences (absolute: the first entry of a unit is the
    dequantised-by-1 DC value it must come out with), and with fit -- which needs a DRI -- flat units put between them
    wherever the reference's reader would run dry at the next one's DC code (quirk Q1: it is not topped up there, and long
    codes leave it few bits) or the difference would need a category above 15: every unit of a case is decoded from its
    own bits.  A reader that cannot take even a flat unit's DC code is left dry to its interval's end."""
    hs, vs = LAYOUTS[layout]
    comps = [0] * (hs * vs) + [1, 2]
    dpm = len(comps)
    todo, out = list(dus), []
    while todo:
        left, pred = 32, [0, 0, 0]
        for slot in range((ri * dpm) if ri else len(todo)):
            comp = comps[slot % dpm]
            td, ta, _ = sel[comp]
            if standard and left < 32:
                left += 32

            def diff_of(du):
                return du[0] - pred[comp] if absolute else du[0]

            def need(du):
                size = abs(int(diff_of(du))).bit_length()
                return huff[2 * td].get(size, 99) + size
            flat = (pred[comp] if absolute else 0, [EOB])
            du = todo.pop(0) if todo and (not fit or not ri or left >= need(todo[0])) else flat
            out.append((diff_of(du), du[1]))
            pred[comp] += diff_of(du)
            if left < need(du):
                left = 0   # (dry from here on)
                continue
            left -= need(du)
            for (r, s, _) in du[1]:
                left += 32 if left < 32 else 0
                left -= huff[2 * ta + 1][r << 4 | s] + s
    return out


def _frame(family, tables, layout, dus, standard=False, ri=0, across=8, huff=None, tag="", fit=True, absolute=False, **kw):
    """Data units laid over whole MCUs (flat ones behind the last), `across` MCUs a row at the most."""
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2
    if huff is None:
        dcs = range(16) if absolute else symbols_of(list(dus) + [FLAT])[0]
        huff = table_set(tables, dcs, symbols_of(list(dus) + [FLAT])[1])
    dus = _place(dus, huff, kw.get("sel", Frame.sel), layout, ri, standard, fit, absolute)
    mcus = max(1, -(-len(dus) // dpm))
    mw = min(across, mcus)
    mh = -(-mcus // mw)
    if ri:
        while (mw * mh) % ri:   # (whole intervals only: every MCU is decoded)
            mh += 1
    dus = list(dus) + [FLAT] * (mw * mh * dpm - len(dus))
    name = f"{family}{tag}/{tables}/{layout}/{'standard' if standard else 'reference'}" + (f"/dri{ri}" if ri else "")
    return Frame(name, layout, mw, mh, dus, huff, ri=ri, standard=standard, family=family, tables=tables, **kw)


def _ends(size):
    lo, hi = 1 << (size - 1), (1 << size) - 1
    return (lo, -lo, hi, -hi)


def ac_sizes(tables, layout="422", dc=False):
    """Every size 1..15 at both ends of both signs, behind runs of 0 and of 15 (positions 1, 17 and 18; the all-ones
    magnitudes fill the stream with stuffed FF bytes).  In `long` the symbol 0xFF is 16 + 15 = 31 bits.  dc: DC
    differences of up to +-90 in place of zeros (a decode that loses its place in the stream then shows in the DC terms
    too, which is all a 1/8-scale decode keeps)."""
    dus = []
    for size in range(1, 16):
        a, b, c, d = _ends(size)
        dus.append((0, [ac(0, a), ac(15, b), ac(0, c), EOB]))
        dus.append((0, [ac(15, d), ac(0, c), ac(15, a), EOB]))     # (the third lands on 33: dropped)
        dus.append((0, [ac(0, b), ac(0, d), ac(15, c), EOB]))
        dus.append((0, [ac(15, c), ac(15, d), EOB]))
    if dc:
        dus = [((37 * k) % 181 - 90, syms) for k, (_, syms) in enumerate(dus)]
    return _frame("ac_sizes", tables, layout, dus, tag="_dc" if dc else "")


def dc_cats(tables, layout="422", ri=1):
    """Every DC category 0..15 at both ends of both signs (DRI 1: the difference is the value); in `long` category 15
    stands behind a 16-bit code, 31 bits, the last stream the direct DC table accepts."""
    vals = [0] + [v for size in range(1, 16) for v in _ends(size)]
    dus = [(v, [EOB]) for v in vals]
    return _frame("dc_cats", tables, layout, dus, ri=ri)


def dc_hostile(layout="422"):
    """Category 16 behind a 2-bit code and category 17 behind a 16-bit code (what no baseline stream holds: the
    cooperative and walk forms must refuse the tables or stop and hand over)."""
    vals = [0, 40000, -40000, 3, 65535, -32768, 100000, -131071, 65536, -7, 1 << 15, 70000]
    dus = [(v, [ac(0, 5), EOB] if i % 2 else [EOB]) for i, v in enumerate(vals)]
    dc = {16: 2, 0: 3, 2: 4, 3: 4, 15: 5, 17: 16}
    act = {0x00: 2, 0x03: 3}
    return _frame("dc_hostile", "own", layout, dus, ri=2, fit=False, huff={0: dc, 1: act, 2: dict(dc), 3: dict(act)})


def q1_underflow(standard, layout="422", ri=2):
    """A 16-bit EOB code and then a 16-bit DC code of category 15, over and over in one interval: the reference's
    reader, not topped up in front of the DC code, holds 16..47 bits there and needs 31.  A first coefficient of 1..15
    bits in every interval moves the pattern through the bit phases of a 32-bit word."""
    dus = []
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2
    for phase in range(16):
        first = [ac(0, 1 << (phase - 1))] if phase else []
        body = [(0, first + [EOB])] + [((-1) ** k * (20000 + 37 * k + phase), [EOB]) for k in range(1, ri * dpm)]
        dus += body
    return _frame("q1_underflow", "long", layout, dus, standard=standard, ri=ri, fit=False, across=8)


def positions(tables, standard, layout="422"):
    """Coefficients landing exactly on zig-zag 31, 32, 46, 47, 62 and 63 by a run; one, two and three ZRLs and then a
    coefficient; a ZRL from 46, 47 and 48; a run that overshoots 63; 63 coefficients and no EOB; EOB first."""
    def reach(target, v):
        """Coefficients on 1.. then one on `target` by the longest runs."""
        syms, pos = [], 1
        while target - pos > 15:
            syms.append(ac(15, 3))
            pos += 16
        syms.append(ac(target - pos, v))
        return syms, target + 1
    zrl = 16 if standard else 17
    dus = []
    for target in (31, 32, 46, 47, 62, 63):
        syms, pos = reach(target, -9 - target)
        dus.append((5, syms + ([EOB] if pos < 64 else [])))
    for n in (1, 2, 3):
        pos = 1 + n * zrl
        dus.append((-5, [ZRL] * n + [ac(2, 11 * n), EOB]))
    for start in (46, 47, 48):
        syms, pos = reach(start - 1, 21)
        pos += zrl
        tail = []
        if pos < 64:                       # (standard mode: the data unit goes on behind the ZRL)
            tail = [ac(0, -2)]
            tail += [EOB] if pos + 1 < 64 else []
        dus.append((1, syms + [ZRL] + tail))
    syms, pos = reach(55, 6)
    dus.append((2, syms + [ac(12, 77)]))                           # 56 + 12 = 68: overshoots, ends the data unit
    dus.append((3, [ac(0, (-1) ** k * (k + 1)) for k in range(63)]))   # 63 coefficients, no EOB
    dus.append((-4, [EOB]))
    dus.append((0, [ac(14, -3), ZRL, ac(0, 5), EOB] if standard else [ac(14, -3), ZRL, EOB]))   # ZRL from 16: to 32 / 33
    return _frame("positions", tables, layout, dus, standard=standard, ri=4 if layout == "422" else 2)


def run_size0(tables, layout="422"):
    """The symbols 0x10 .. 0xE0 (a run and no magnitude bits): they advance and write a zero; real coefficients between
    them."""
    dus = []
    for r in range(1, 15):
        dus.append((r, [ac(0, 7), (r, 0, 0), ac(0, -r), (r, 0, 0), ac(1, 100 + r), EOB]))
        dus.append((-r, [(r, 0, 0), (15 - r, 0, 0), ac(0, 9), (r, 0, 0), EOB]))
    dus.append((0, [(14, 0, 0)] * 4 + [(6, 0, 0)]))   # 1 + 4 * 15 + 6 = 67: ends the data unit without EOB
    return _frame("run_size0", tables, layout, dus, ri=3 if layout == "422" else 0)


def pairs(tables, layout="422"):
    """Codes of 1 and 2 bits with 1-bit magnitudes: two symbols fit in the walk tables' prefix.  Pairs whose first symbol
    ends the data unit (EOB, then the next unit's DC code), every alignment against the 32-bit words (the lengths of the
    units run through 0..11 coefficients), and with `long` every symbol escaping."""
    rng = np.random.default_rng(12)
    dus = []
    for n in range(96):
        k = n % 12
        syms = [ac(int(rng.integers(0, 2)), int(rng.choice((-1, 1)))) for _ in range(k)]
        dus.append((int(rng.choice((0, 0, 1, -1))), syms + [EOB]))
    huff = None
    if tables == "short":
        dc, act = {0: 1, 1: 2}, {0x00: 1, 0x01: 2, 0x11: 3}
        huff = {0: dc, 1: act, 2: dict(dc), 3: dict(act)}
    return _frame("pairs", tables, layout, dus, ri=6 if layout == "422" else 3, huff=huff)


_MAX15 = (1 << 15) - 1


def basis(q, layout="422", ri=1):
    """One coefficient alone at each of the 32 retained positions, amplitudes +-1 and +-32767; one data unit with only
    positions 32..63 set (nothing may appear).  DRI 1: the DC position's difference is its value."""
    dus = []
    for pos in range(32):
        for v in (1, -1, _MAX15, -_MAX15):
            if pos == 0:
                dus.append((v, [EOB]))
            else:
                syms, p = [], 1
                while pos - p > 15:   # (a ZRL advances 17; 16 short of the place, a run symbol without magnitude 2)
                    syms.append(ZRL if pos - p >= 17 else (1, 0, 0))
                    p += 17 if pos - p >= 17 else 2
                dus.append((0, syms + [ac(pos - p, v), EOB]))
    dus.append((0, [ZRL, ac(14, 500)] + [ac(0, 500 + k) for k in range(31)]))   # 18 + 14 = 32, then 33..63
    qt = tuple(np.full(64, q) for _ in range(2))
    return _frame("basis", "short", layout, dus, ri=ri, absolute=True, tag=f"_q{q}", quant=qt)


def dc_sweep(layout="422", ri=1):
    """A flat data unit for every dequantised DC from -1100 to 1100, in Y and in each chroma (DRI 1, q = 1): every 8-bit
    level, both clamps, every truncation boundary behind the 128.5 bias.  2201 MCUs: a chroma has one data unit in each."""
    hs, vs = LAYOUTS[layout]
    vals = list(range(-1100, 1101))
    dus = []
    for i, v in enumerate(vals):
        ys = [vals[(i * hs * vs + k) % len(vals)] for k in range(hs * vs)]
        dus += [(y, [EOB]) for y in ys] + [(v, [EOB]), (-v, [EOB])]
    return _frame("dc_sweep", "short", layout, dus, ri=ri, absolute=True, across=31)


def gamut(layout="422", ri=1):
    """Flat MCUs with dequantised DC 8 * (v - 128), which the IDCT turns into level v exactly: Cb and Cr each over all 256
    values while the other is 0, 128 and 255, Y over 0, 1, 127, 128, 254, 255 (DRI 1)."""
    hs, vs = LAYOUTS[layout]
    n = hs * vs
    ys = (0, 1, 127, 128, 254, 255)
    dus = []
    for sweep_cb in (True, False):
        for other in (0, 128, 255):
            for v in range(256):
                for y0 in range(0, len(ys), 2):   # (three MCUs a value; with one Y an MCU the odd values take the odd levels)
                    yv = [ys[(y0 + (v % 2 if n == 1 else 0) + k) % len(ys)] for k in range(n)]
                    cb, cr = (v, other) if sweep_cb else (other, v)
                    dus += [(8 * (y - 128), [EOB]) for y in yv] + [(8 * (cb - 128), [EOB]), (8 * (cr - 128), [EOB])]
    return _frame("gamut", "short", layout, dus, ri=ri, absolute=True, across=72)


def saturated(layout="422", ri=1):
    """All 32 positions at +-32767 and q = 255: all plus, alternating, seeded random signs (f32 rounding far above 2^24,
    then the clamp)."""
    rng = np.random.default_rng(31)
    signs = [np.ones(32, int), (-1) ** np.arange(32), -((-1) ** np.arange(32))] + [rng.choice((-1, 1), 32) for _ in range(13)]
    dus = [(int(s[0]) * _MAX15, [ac(0, int(s[p]) * _MAX15) for p in range(1, 32)] + [EOB]) for s in signs]   # (DC: the value)
    qt = tuple(np.full(64, 255) for _ in range(2))
    return _frame("saturated", "short", layout, dus, ri=ri, absolute=True, quant=qt)


def dc_wrap(layout="422"):
    """A strip one MCU wide, one interval of 320 MCUs: every luma data unit adds 32767 to the predictor at q0 = 255, so
    the 32-bit product wraps inside the frame and the samples flip between the clamps."""
    hs, vs = LAYOUTS[layout]
    mcu = [(_MAX15, [EOB])] * (hs * vs) + [(3, [EOB]), (-2, [EOB])]
    qt = (np.full(64, 255), np.full(64, 7))
    return _frame("dc_wrap", "short", layout, mcu * 320, across=1, quant=qt)


_ALL_AC = [r << 4 | s for r in range(16) for s in range(1, 16)] + [0x00, 0xF0]


def random_dense(ri, layout="422", mcus=None, across=None, tag="", tables="long"):
    """Seeded random symbol lists over the full symbol set of `long` (sizes 1..15, every run, ZRL, EOB).  With a DRI the
    reference's reader runs dry at some DC code of most intervals (quirk Q1: 16-bit codes all round); without one (a
    single interval) every DC category is kept to the bits the reader holds there, so that the whole frame decodes."""
    mcus = mcus or (63 if ri in (3, 7) else 64)   # (whole intervals)
    across = across or (7 if ri in (3, 7) else 8)
    rng = np.random.default_rng(1000 + ri + mcus)
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2
    huff = table_set(tables, range(16), _ALL_AC)
    dus = []
    left = 32
    for i in range(mcus * dpm):
        dcl, acl = (huff[0], huff[1]) if i % dpm < dpm - 2 else (huff[2], huff[3])   # (Frame.sel: luma on Th0, chroma on Th1)
        size = int(rng.integers(0, 16))
        while not ri and size and dcl[size] + size > left:
            size -= 1
        left -= dcl[size] + size
        diff = extend(int(rng.integers(0, 1 << size)), size) if size else 0
        syms, pos = [], 1
        for _ in range(int(rng.integers(0, 24))):
            if rng.random() < 0.06 and (ri or pos + 17 < 64):
                syms.append(ZRL)
                pos += 17
            else:
                r, s = int(rng.integers(0, 16)) if rng.random() < 0.3 else int(rng.integers(0, 3)), int(rng.integers(1, 16))
                if not ri and pos + r + 1 >= 64:
                    break   # (every data unit ends on an EOB there: 16 bits at the least in front of the DC code)
                syms.append((r, s, int(rng.integers(0, 1 << s))))
                pos += r + 1
            if pos >= 64:
                break
        if pos < 64:
            syms.append(EOB)
        for (r, s, _) in syms:
            left += 32 if left < 32 else 0
            left -= acl[r << 4 | s] + s
        dus.append((diff, syms))
    qt = (np.arange(64) % 13 + 1, np.arange(64) % 7 + 2)
    return _frame("random_dense", tables, layout, dus, ri=ri, fit=False, across=across, huff=huff, tag=tag, quant=qt)


def texture(layout="422"):
    """Seeded random levels of 1..5 bits at most positions, quantisers 1..13, DC around mid-grey: most samples stay
    between the clamps, where the last bit of every f32 operation of the transform shows (what tells a contracted
    multiply-add and a rounding conversion from the reference's separate operations and truncation)."""
    rng = np.random.default_rng(77)
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2
    dus = []
    for _ in range(64 * dpm):
        syms, pos = [], 1
        while True:
            r = int(rng.integers(0, 4))
            if pos + r >= 40:
                break
            s = int(rng.integers(1, 6))
            syms.append((r, s, int(rng.integers(0, 1 << s))))
            pos += r + 1
        dus.append((int(rng.integers(-60, 61)), syms + [EOB]))
    qt = (np.arange(64) % 13 + 1, np.arange(64) % 7 + 2)
    return _frame("texture", "edge", layout, dus, ri=4, quant=qt)


def cancel(layout="422", ri=1):
    """Two horizontal frequencies of some millions (levels x 255 at zig-zag 1 and 6) that cancel at one column of the
    data unit, a third (zig-zag 15, q = 1) that tunes the rest away, and a DC of 4: that column's samples stand at 129.0
    give or take the rounding of products of about 10^6.  Which side of the truncation they fall on depends on every
    single f32 rounding of the row pass (a contracted multiply-add rounds once where the reference rounds twice)."""
    rng = np.random.default_rng(5)
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2

    def b(c, x):
        return np.sqrt(2.0) / 8.0 * np.cos((2 * x + 1) * c * np.pi / 16.0)
    dus = []
    for i in range((64 - 64 % ri) * dpm):   # (whole intervals in 64 MCUs)
        x = i % 8
        a1 = int(rng.integers(4000, 7000)) * int(rng.choice((-1, 1)))
        a3 = int(round(-a1 * b(1, x) / b(3, x)))
        rest = 255.0 * (a1 * b(1, x) + a3 * b(3, x))
        a5 = int(round(-rest / b(5, x)))
        dus.append((4, [ac(0, a1), ac(4, a3)] + ([ac(8, a5)] if a5 else []) + [EOB]))
    q = np.full(64, 255)
    q[[0, 15]] = 1
    return _frame("cancel", "short", layout, dus, ri=ri, absolute=True, across=ri if 64 % ri else 8, quant=(q, q.copy()))


def random_strip():
    """The `random_dense` strip of 520 MCUs without DRI (tests/route_matrix.py: STRIP_MCUS)."""
    return random_dense(0, mcus=520, across=1, tag="_strip")


def one_mcu(tables, layout="422"):
    """A frame of one MCU: a dozen different AC symbols in every data unit, so that each table's used codes are of every
    length the table set has."""
    dpm = LAYOUTS[layout][0] * LAYOUTS[layout][1] + 2
    dus = [(97 * k - 150, [ac((k + j) % 3, (-1) ** j * ((1 << (j % 9)) + k)) for j in range(12)] + [EOB]) for k in range(dpm)]
    return _frame("one_mcu", tables, layout, dus, fit=False)


_WIDE = None


def wide_cases():
    """Frames whose Huffman tables outgrow their share of LDS (WIDE_KINDS; table_regime), in every layout: `ac_sizes`
    without DRI, with DC differences -- its data units are those of its `short` twin, one frame per regime --, `dc_cats` at DRI 1 (64 intervals;
    DC codes of 10 to 16 bits, which escape the cooperative kernel's direct DC table), `positions` under standard entropy,
    `random_dense` at DRI 1 over 65 MCUs (two waves, every AC symbol in use: lookups all over the tables), a frame of one
    MCU, and in 4:2:2 the dense strip of 520 MCUs.  Not part of cases(): tests/test_gpu_coef.py pins a kernel to each of
    those."""
    global _WIDE
    if _WIDE is None:
        out = []
        for lay in LAYOUTS:
            out += [ac_sizes(k, lay, dc=True) for k in ("wide_a", "wide_b", "wide_b48", "wide_c", "full")]
            out += [dc_cats(k, lay) for k in ("wide_b", "wide_c", "wide_c2")]
            out += [positions(k, True, lay) for k in ("wide_b", "wide_c")]
            out += [random_dense(1, lay, mcus=65, across=5, tables=k) for k in ("wide_b", "wide_b48", "wide_c", "wide_c2", "full")]
            out += [one_mcu(k, lay) for k in ("wide_c", "wide_c2")]
        out.append(random_dense(0, mcus=520, across=1, tag="_strip", tables="wide_c"))
        assert len({f.name for f in out}) == len(out)
        _WIDE = out
    return _WIDE


def wide_case(name):
    return next(f for f in wide_cases() if f.name == name)


def one_block_too_many(layout="422"):
    """`ac_sizes` under tables of 129 blocks: one more than `full`, the first file both parsers refuse."""
    return ac_sizes("over", layout, dc=True)


_CASES = None


def cases():
    """Every named frame: each family in 4:2:2 under every table set it is defined for, and one representative of each
    family in 4:4:4, 4:4:0 and 4:2:0."""
    global _CASES
    if _CASES is None:
        out = []
        for t in ("short", "edge", "long"):
            out += [ac_sizes(t), dc_cats(t), run_size0(t)]
        out += [dc_hostile(), q1_underflow(False), q1_underflow(True), pairs("short"), pairs("long")]
        out += [dc_cats("short", ri=4), q1_underflow(False, ri=4)]   # (intervals the walk + lane-per-MCU route takes)
        out += [basis(255, ri=8), dc_sweep(ri=8), gamut(ri=8), saturated(ri=8), cancel(ri=9)]   # (the same: mixed, 8 and more)
        out += [positions(t, std) for t in ("short", "long") for std in (False, True)]
        out += [basis(1), basis(255), dc_sweep(), gamut(), saturated(), dc_wrap(), texture(), cancel()]
        out += [random_dense(ri) for ri in (0, 1, 3, 7)] + [random_strip()]
        for lay in ("444", "440", "420"):
            out += [ac_sizes("long", lay), dc_cats("long", lay), dc_hostile(lay), q1_underflow(False, lay),
                    positions("short", False, lay), run_size0("edge", lay), pairs("short", lay), basis(255, lay),
                    dc_sweep(lay), gamut(lay), saturated(lay), dc_wrap(lay), random_dense(3, lay), texture(lay), cancel(lay)]
            if lay != "420":   # (intervals of two MCUs: the paired 4:4:4 / 4:4:0 kernels and their streamed form)
                out += [dc_cats("edge", lay, ri=2), basis(255, lay, ri=2), dc_sweep(lay, ri=2), gamut(lay, ri=2),
                        saturated(lay, ri=2), cancel(lay, ri=2)]
        assert len({f.name for f in out}) == len(out)
        _CASES = out
    return _CASES


def case(name):
    return next(f for f in cases() if f.name == name)
