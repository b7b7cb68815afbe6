"""Grayscale (one-component) baseline JPEGs at the level of tests/coef_stream.py, and what the decoder must make of them.
A plain module (Python and numpy, no fixtures), shared by tests/test_gray_stream.py (the oracle's twin and the host front
end), tests/test_gray_emulation.py (the emulated lane body) and tests/test_gpu_gray.py (the card).

A grayscale image decodes to what its 4:4:4 twin decodes to: the same file with two more components whose data units are
all "DC difference 0, EOB" -- Cb = Cr = 128, every pixel R = G = B = the luma sample, A = 255.  The twin's chroma data
units move the stream's bit positions, so where the reference's reader runs dry (quirk Q1) the two streams part: there
the restatement alone -- cs.predict on the one-component stream -- is the expectation."""
from dataclasses import dataclass

import numpy as np

import coef_stream as cs


@dataclass
class GrayFrame(cs.Frame):
    """A cs.Frame with one data unit per MCU.  px_w / px_h: the frame header's extent where it is not whole MCUs; hv: the
    lone component's sampling factors as the header states them (ignored by a decoder: T.81 A.2.2)."""
    px_w: int = 0
    px_h: int = 0
    hv: int = 0x11

    @property
    def sampling(self):
        return (1, 1)

    @property
    def dus_per_mcu(self):
        return 1

    @property
    def comp_of_du(self):
        return [0]

    @property
    def w(self):
        return self.px_w or self.mcus_w * 8

    @property
    def h(self):
        return self.px_h or self.mcus_h * 8

    def image_kw(self):
        return dict(allow_grayscale=True, standard_entropy=self.standard)

    def jpeg(self):
        if self._jpeg is None:
            self._jpeg = write(self)
        return self._jpeg


def scan_bytes(f):
    """The entropy-coded segment as write() emits it: stuffed, RSTn between the intervals."""
    segs = cs._segments(f)
    out = bytearray()
    for i, s in enumerate(segs):
        out += s.replace(b"\xff", b"\xff\x00")
        if i + 1 < len(segs):
            out += bytes([0xFF, 0xD0 + i % 8])
    return bytes(out)


def write(f, ncomp_in_scan=1, scan_id=1):
    """cs.write with a one-component SOF0 and SOS (component id 1)."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    out = bytearray(b"\xff\xd8")
    for t in range(len(f.quant)):
        q = f.qtable(t)
        assert q.min() >= 1 and q.max() <= 255
        out += seg(0xDB, bytes([t]) + bytes(int(x) for x in q))
    out += seg(0xC0, bytes([8]) + f.h.to_bytes(2, "big") + f.w.to_bytes(2, "big") + bytes([1, 1, f.hv, f.sel[0][2]]))
    for t in sorted(f.huff):
        bits, vals, _ = cs.canonical(f.huff[t])
        out += seg(0xC4, bytes([(t & 1) << 4 | t >> 1]) + bytes(bits) + bytes(vals))
    if f.ri:
        out += seg(0xDD, f.ri.to_bytes(2, "big"))
    comps = bytes([scan_id, f.sel[0][0] << 4 | f.sel[0][1]]) + bytes([2, 0x11]) * (ncomp_in_scan - 1)
    out += seg(0xDA, bytes([ncomp_in_scan]) + comps + bytes([0, 63, 0]))
    return bytes(out + scan_bytes(f) + b"\xff\xd9")


def twin(f):
    """The 4:4:4 cs.Frame with flat chroma: the same tables for luma and chroma, chroma under quantiser table 1."""
    td, ta, tq = f.sel[0]
    assert 0 in f.huff[2 * td] and 0x00 in f.huff[2 * ta + 1], "cs.FLAT's symbols are in the luma tables"
    quant = tuple(f.quant) if len(f.quant) > 1 else (f.quant[0], 1)
    dus = [u for du in f.dus for u in (du, cs.FLAT, cs.FLAT)]
    assert not (f.px_w or f.px_h), "twins are made of whole MCUs"
    return cs.Frame(f.name + "/twin", "444", f.mcus_w, f.mcus_h, dus, f.huff, ri=f.ri, quant=quant,
                    sel=((td, ta, tq), (td, ta, 1), (td, ta, 1)), standard=f.standard, family=f.family, tables=f.tables)


def gray_of(f444, mcus_w=None, ri=None):
    """The luma data units of a 4:4:4 cs.Frame (their DC differences stay valid: the predictor is the component's own).
    mcus_w / ri: laid out anew, that many MCUs a row (whole rows, whole intervals: flat units behind the last)."""
    assert f444.layout == "444"
    dus = list(f444.dus[0::3])
    mw = f444.mcus_w if mcus_w is None else mcus_w
    r = f444.ri if ri is None else ri
    mh = -(-len(dus) // mw)
    while r and (mw * mh) % r:
        mh += 1
    dus += [cs.FLAT] * (mw * mh - len(dus))
    name = f444.name.split("/dri")[0].replace("/444/", "/gray/") + (f"/dri{r}" if r else "") + f"/w{mw}"
    return GrayFrame(name, "gray", mw, mh, dus, f444.huff, ri=r, quant=f444.quant, sel=(f444.sel[0],) * 3,
                     standard=f444.standard, family=f444.family, tables=f444.tables)


def expectation(f, whole_mcus=False):
    """RGBA [h, w, 4]: cs.predict -> cs.samples -> the luma replicated, A = 255; MCUs behind the last complete restart
    interval stay zero.  whole_mcus: not cut to the frame's extent."""
    smp = cs.samples(cs.predict(f))
    out = np.zeros((f.mcus_h * 8, f.mcus_w * 8, 4), dtype=np.uint8)
    for m in range(smp.shape[0]):
        my, mx = divmod(m, f.mcus_w)
        out[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8, :3] = smp[m][:, :, None]
        out[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8, 3] = 255
    return out if whole_mcus else out[:f.h, :f.w]


# ---- a T.81 symbol reader for real encoders' files --------------------------------------------------------------------

class _Src:
    def __init__(self, data):
        self.data, self.at = data, 0

    def bit(self):
        assert self.at < 8 * len(self.data), "the segment ends inside a symbol"
        b = self.data[self.at >> 3] >> (7 - (self.at & 7)) & 1
        self.at += 1
        return b

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | self.bit()
        return v

    def symbol(self, by_code):
        code, n = 0, 0
        while True:
            code, n = code << 1 | self.bit(), n + 1
            assert n <= 16, "no such code"
            if (code, n) in by_code:
                return by_code[(code, n)]


def from_jpeg(jpeg, name="file"):
    """A one-component baseline JPEG -> the GrayFrame whose writer reproduces its entropy-coded segment: tables, DRI and
    every data unit's symbols as the file has them (decoded as T.81 has it: ZRL = 16 positions)."""
    at, quant, huff, ri, sof, sos = 2, {}, {}, 0, None, None
    assert jpeg[:2] == b"\xff\xd8"
    while sos is None:
        assert jpeg[at] == 0xFF
        m, n = jpeg[at + 1], int.from_bytes(jpeg[at + 2:at + 4], "big")
        body = jpeg[at + 4:at + 2 + n]
        if m == 0xDB:
            for k in range(0, len(body), 65):
                assert body[k] >> 4 == 0
                quant[body[k] & 15] = np.array(list(body[k + 1:k + 65]), dtype=np.int64)
        elif m == 0xC4:
            k = 0
            while k < len(body):
                tc, th = body[k] >> 4, body[k] & 15
                counts = list(body[k + 1:k + 17])
                vals = list(body[k + 17:k + 17 + sum(counts)])
                lengths = [n_ for n_, c in enumerate(counts, 1) for _ in range(c)]
                huff[2 * th + tc] = dict(zip(vals, lengths))   # (HUFFVAL order: canonical() keeps it within a length)
                k += 17 + sum(counts)
        elif m == 0xC0:
            sof = body
        elif m == 0xDD:
            ri = int.from_bytes(body[:2], "big")
        elif m == 0xDA:
            sos = body
        at += 2 + n
    assert sof[0] == 8 and sof[5] == 1 and sos[0] == 1 and sos[1] == sof[6]
    h, w = int.from_bytes(sof[1:3], "big"), int.from_bytes(sof[3:5], "big")
    td, ta, tq = sos[2] >> 4, sos[2] & 15, sof[8]
    end = jpeg.rindex(b"\xff\xd9")
    raw = jpeg[at:end]
    segs, cur, i = [], bytearray(), 0
    while i < len(raw):
        if raw[i] == 0xFF and raw[i + 1] == 0x00:
            cur.append(0xFF)
            i += 2
        elif raw[i] == 0xFF:
            assert 0xD0 <= raw[i + 1] <= 0xD7
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            cur.append(raw[i])
            i += 1
    segs.append(bytes(cur))
    mw, mh = -(-w // 8), -(-h // 8)
    interval = ri or mw * mh
    by_code = {t: {v: k for k, v in cs.canonical(l)[2].items()} for t, l in huff.items()}
    dus = []
    for n, s in enumerate(segs):
        src = _Src(s)
        for _ in range(min(interval, mw * mh - n * interval)):
            size = src.symbol(by_code[2 * td])
            diff = cs.extend(src.bits(size), size)
            syms, pos = [], 1
            while pos < 64:
                rs = src.symbol(by_code[2 * ta + 1])
                r, sz = rs >> 4, rs & 15
                syms.append((r, sz, src.bits(sz)))
                if rs == 0:
                    break
                pos += 16 if rs == 0xF0 else r + 1
            dus.append((diff, syms))
    assert len(dus) == mw * mh
    qt = tuple(quant.get(t, np.ones(64, dtype=np.int64)) for t in range(max(quant) + 1))
    return GrayFrame(name, "gray", mw, mh, dus, huff, ri=ri, quant=qt, sel=((td, ta, tq),) * 3, standard=True,
                     px_w=w if w != mw * 8 else 0, px_h=h if h != mh * 8 else 0, hv=sof[7], _jpeg=None)


def file_scan(jpeg):
    """The entropy-coded segment of a file with one scan: from behind its SOS header to its EOI."""
    at = jpeg.index(b"\xff\xda")
    return jpeg[at + 2 + int.from_bytes(jpeg[at + 2:at + 4], "big"):jpeg.rindex(b"\xff\xd9")]


# ---- the frames -------------------------------------------------------------------------------------------------------

def _families_444():
    """One frame of every family of cs.cases() at layout 444 (the first of each)."""
    seen = {}
    for f in cs.cases():
        if f.layout == "444":
            seen.setdefault(f.family, f)
    return list(seen.values())


def random_gray(ri, mcus_w, standard, mcus=20):
    """Seeded random dense data units over every AC symbol under codes of 8 bits (DC: 5 bits, categories up to 4), valid in
    the given entropy mode (a ZRL advances 16 or 17 there).  With such codes neither this stream nor its twin runs the
    reference's reader dry: in front of a DC code it holds 9 bits at the least and needs 9 at the most."""
    rng = np.random.default_rng(500 + 10 * ri + mcus_w + (100 if standard else 0))
    zrl = 16 if standard else 17
    mh = -(-mcus // mcus_w)
    while ri and (mcus_w * mh) % ri:
        mh += 1
    dus = []
    for _ in range(mcus_w * mh):
        size = int(rng.integers(0, 5))
        diff = cs.extend(int(rng.integers(0, 1 << size)), size) if size else 0
        syms, pos = [], 1
        for _ in range(int(rng.integers(0, 30))):
            if rng.random() < 0.08:
                syms.append(cs.ZRL)
                pos += zrl
            else:
                r = int(rng.integers(0, 16)) if rng.random() < 0.3 else int(rng.integers(0, 3))
                sz = int(rng.integers(1, 16)) if rng.random() < 0.3 else int(rng.integers(1, 7))
                syms.append((r, sz, int(rng.integers(0, 1 << sz))))
                pos += r + 1
            if pos >= 64:
                break
        if pos < 64:
            syms.append(cs.EOB)
        dus.append((diff, syms))
    huff = cs.table_set("short", range(16), cs._ALL_AC)
    name = f"random_gray/short/gray/{'standard' if standard else 'reference'}" + (f"/dri{ri}" if ri else "") + f"/w{mcus_w}"
    return GrayFrame(name, "gray", mcus_w, mh, dus, huff, ri=ri, quant=(np.arange(64) % 13 + 1, np.arange(64) % 7 + 2),
                     sel=((0, 0, 0),) * 3, standard=standard, family="random_gray", tables="short")


_CASES = None
GEOMETRIES = ((0, 5), (1, 6), (2, 5), (3, 6), (7, 2), (2, 1), (3, 1), (0, 1))   # (DRI, MCUs a row)


def cases():
    """Every family of cs.cases() at layout 444 through gray_of, as it stands (its own DRI and width) and -- the families
    whose frames are small -- under DRI none, 1, 2, 3, 7 at 1, 2, 5 and 6 MCUs a row; both entropy modes where the family
    has them."""
    global _CASES
    if _CASES is None:
        out = {}   # (by name: a family's own geometry may be one of GEOMETRIES)
        for f in _families_444():
            g = gray_of(f)
            out.setdefault(g.name, g)
            if len(f.dus) // 3 <= 200:
                for ri, mw in GEOMETRIES:
                    g = gray_of(f, mcus_w=mw, ri=ri)
                    out.setdefault(g.name, g)
        for std in (False, True):
            for ri, mw in GEOMETRIES:
                g = random_gray(ri, mw, std)
                out.setdefault(g.name, g)
        out = list(out.values())
        assert len({f.name for f in out}) == len(out)
        _CASES = out
    return _CASES


def case(name):
    return next(f for f in cases() if f.name == name)


_WIDE = None


def on_th1(g):
    """The frame with its one component on Th1's tables: in cs.WIDE_KINDS' `wide_c` those lie wholly beyond the LDS share.
    (The tables of one set give a used symbol the same group of lengths in Th0 and Th1; what the reference's reader makes of
    the other lengths is cs.predict's to say.)"""
    td, ta, tq = g.sel[0]
    return GrayFrame(g.name + "/th1", "gray", g.mcus_w, g.mcus_h, g.dus, g.huff, ri=g.ri, quant=g.quant, sel=((1, 1, tq),) * 3,
                     standard=g.standard, family=g.family, tables=g.tables)


def wide_cases():
    """cs.wide_cases() at layout 444 through gray_of: the file keeps all four tables, so its regime is the 4:4:4 frame's.
    In regimes A and B the component decodes with Th0's tables; in regime C with Th1's, which lie wholly beyond the LDS
    share in every kind -- its DC lookups too, so that a decode which keeps the DC terms alone (1/8 scale) meets them."""
    global _WIDE
    if _WIDE is None:
        out = [gray_of(f) for f in cs.wide_cases() if f.layout == "444"]
        out = [on_th1(g) if cs.table_regime(g)["regime"] == "C" else g for g in out]
        assert len({f.name for f in out}) == len(out)
        _WIDE = out
    return _WIDE
