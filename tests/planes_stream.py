"""What a planes decode (include/compeg_hip.h, "Planar YCbCr output") must write, made on the host.  A plain module (Python
and numpy, no fixtures), shared by tests/test_planes_stream.py (the expectation pinned to the oracle's RGBA),
tests/test_planes_emulation.py (the emulated lane body) and tests/test_gpu_planes.py (the card).

The chain: the dequantised coefficients the reference keeps (cs.predict for frames written from coefficients; the oracle's
own orc_huffman_pass / orc_huffman_pass_ext for real encoders' files) -> cs.samples -> the data units laid into whole-MCU
planes, with a mask of what was decoded at all -> format and chroma option applied -> cut to the planes' extents and laid
into the destination over whatever was there before.  The layout (offsets, pitches, extents) is restated here and
compared with compeg_planes_shape in the tests."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import coef_stream as cs
import gray_stream as gs
from oracle import oracle as orc

FORMATS = ("planar", "semiplanar", "yuyv", "uyvy")
SAMPLINGS = {"422": (2, 1), "444": (1, 1), "440": (1, 2), "420": (2, 2), "gray": (1, 1)}


@dataclass
class PlanesFrame(cs.Frame):
    """A cs.Frame whose frame header states px_w x px_h where that is not whole MCUs."""
    px_w: int = 0
    px_h: int = 0

    @property
    def w(self):
        return self.px_w or self.mcus_w * 8 * self.sampling[0]

    @property
    def h(self):
        return self.px_h or self.mcus_h * 8 * self.sampling[1]


def sized(layout, w, h, ri, standard=False, seed=0, source=None, short=0):
    """A frame of w x h pixels in `layout` ("422" .. "420", "gray"): the data units of cs.texture (or of `source`, a frame of
    the same layout) taken round and round from unit `seed` on, laid over the MCUs the extent needs, DRI ri (0: none).
    short: that many MCUs are missing from the last restart interval's count -- the frame has MCUs no complete interval
    covers."""
    gray = layout == "gray"
    hs, vs = SAMPLINGS[layout]
    src = source or cs.texture("444" if gray else layout)
    dpm = 1 if gray else hs * vs + 2
    units = src.dus[0::3] if gray and source is None else src.dus
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    n = mw * mh * dpm
    dus = [units[(seed + i) % len(units)] for i in range(n)]
    name = f"sized/{layout}/{w}x{h}/{'standard' if standard else 'reference'}/dri{ri}/s{seed}" + (f"/short{short}" if short else "")
    if not short:
        assert not ri or (mw * mh) % ri == 0, "whole intervals (or say how many MCUs are short)"
    else:
        assert ri and (mw * mh) % ri == ri - short
    kw = dict(ri=ri, quant=src.quant, standard=standard, family="sized", tables=src.tables, px_w=w, px_h=h)
    if gray:
        return SizedGray(name, "gray", mw, mh, dus, src.huff, sel=(src.sel[0],) * 3, **kw)
    return PlanesFrame(name, layout, mw, mh, dus, src.huff, sel=src.sel, **kw)


@dataclass
class SizedGray(gs.GrayFrame):
    pass


def sampling_of(f):
    """(components, hs, vs) as compeg_planes_shape takes them."""
    return (1, 1, 1) if isinstance(f, gs.GrayFrame) else (3,) + tuple(f.sampling)


# ---- the layout, restated --------------------------------------------------------------------------------------------

def layout(w, h, components, hs, vs, format="planar", chroma="coded", pitch=None):
    """-> ([(offset, pitch, row_bytes, width, height)] per plane, total bytes): plane p + 1 begins where plane p's rows end,
    every row at its full pitch; no alignment."""
    cw, ch = -(-w // hs), (-(-h // 2) if chroma == "420" else -(-h // vs))
    if format in ("yuyv", "uyvy"):
        planes = [(4 * -(-w // 2), w, h)]
    elif components == 1:
        planes = [(w, w, h)]
    elif format == "semiplanar":
        planes = [(w, w, h), (2 * cw, cw, ch)]
    else:
        planes = [(w, w, h), (cw, cw, ch), (cw, cw, ch)]
    pitch = (0, 0) if pitch is None else (pitch if isinstance(pitch, (tuple, list)) else (pitch, 0))
    out, at = [], 0
    for p, (row, pw, ph) in enumerate(planes):
        pt = (pitch[0] if p == 0 else pitch[1]) or row
        out.append((at, pt, row, pw, ph))
        at += pt * ph
    return out, at


# ---- samples into planes ---------------------------------------------------------------------------------------------

def whole_planes(smp, dpm, hs, vs, mcus_w, mcus_h):
    """uint8 samples [data units, 8, 8] of the decoded MCUs -> (Y, Cb, Cr, masks): whole-MCU planes at each component's own
    resolution and bool masks of the samples a decoded MCU covers.  dpm = 1: luma only (Cb = Cr = None)."""
    mcus = smp.shape[0] // dpm
    smp = smp.reshape(mcus, dpm, 8, 8)
    y = np.zeros((mcus_h * 8 * vs, mcus_w * 8 * hs), dtype=np.uint8)
    my_ = np.zeros(y.shape, dtype=bool)
    cb = cr = mc = None
    if dpm > 1:
        cb, cr = np.zeros((mcus_h * 8, mcus_w * 8), dtype=np.uint8), np.zeros((mcus_h * 8, mcus_w * 8), dtype=np.uint8)
        mc = np.zeros(cb.shape, dtype=bool)
    for m in range(mcus):
        r, c = divmod(m, mcus_w)
        if r >= mcus_h:
            break
        sl = (slice(r * 8 * vs, (r + 1) * 8 * vs), slice(c * 8 * hs, (c + 1) * 8 * hs))
        y[sl] = np.block([[smp[m, v * hs + h] for h in range(hs)] for v in range(vs)])
        my_[sl] = True
        if dpm > 1:
            sc = (slice(r * 8, r * 8 + 8), slice(c * 8, c * 8 + 8))
            cb[sc], cr[sc], mc[sc] = smp[m, dpm - 2], smp[m, dpm - 1], True
    return y, cb, cr, (my_, mc)


def frame_planes(f):
    """A coefficient frame's whole-MCU planes: cs.predict -> cs.samples -> whole_planes."""
    comps, hs, vs = sampling_of(f)
    return whole_planes(cs.samples(cs.predict(f)), f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)


def file_planes(ca, jpeg, **kw):
    """A real encoder's file: the oracle's own entropy pass (orc_huffman_pass; _ext with the standard-entropy flag) over the
    image's metadata block, LUTs and preprocessed scan, then cs.samples -> whole_planes.  -> (planes, (w, h, comps, hs, vs)).
    kw: compeg_amd.ImageData's (allow_sampling, allow_grayscale, standard_entropy)."""
    standard = bool(kw.get("standard_entropy"))
    img = ca.ImageData(jpeg, **kw)
    off, n = img.scan_range()
    sb = orc.ScanBuffer()
    try:
        sb.process(jpeg[off:off + n], img.parallelism())
    except orc.OracleError:
        pass   # (a count mismatch leaves the truncated result in place, as in the reference)
    words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32).copy()
    starts = np.frombuffer(sb.start_positions(), dtype=np.uint32).copy()
    md = np.frombuffer(img.metadata(), dtype=np.uint32)
    ri, intervals, mcus_w, dpm = int(md[256]), int(md[272]), int(md[273]), int(md[276])
    dus = ri * intervals * dpm
    l2 = img.huffman_l2()
    bufs = [np.frombuffer(b, dtype=np.uint8).copy() for b in (img.metadata(), img.huffman_l1(), l2 or b"\0\0")]
    coef = np.zeros(max(1, dus * 32), dtype=np.int32)
    args = (bufs[0].ctypes.data, bufs[1].ctypes.data, bufs[2].ctypes.data, len(l2), words.ctypes.data, words.size, starts.ctypes.data,
            starts.size, coef.ctypes.data, coef.size)
    if standard:
        ext = orc.lib().orc_huffman_pass_ext
        vp, sz = C.c_void_p, C.c_size_t
        ext.restype, ext.argtypes = None, [vp, vp, vp, sz, vp, sz, vp, sz, vp, sz, C.c_uint]
        ext(*args, 2)   # (COMPEG_PARSE_STANDARD_ENTROPY)
    else:
        orc.lib().orc_huffman_pass(*args)
    full = np.zeros((dus, 64), dtype=np.int32)
    full[:, :32] = coef[:dus * 32].reshape(dus, 32)
    comps = img.components()
    hs, vs = img.sampling()
    w, h = img.width(), img.height()
    mcus_h = -(-h // (8 * vs))
    return whole_planes(cs.samples(full), dpm, hs, vs, mcus_w, mcus_h), (w, h, comps, hs, vs)


# ---- formats ---------------------------------------------------------------------------------------------------------

def _interleave(a, b):
    out = np.zeros((a.shape[0], a.shape[1] * 2), dtype=a.dtype)
    out[:, 0::2], out[:, 1::2] = a, b
    return out


def formatted(planes, format="planar", chroma="coded"):
    """Whole-MCU planes -> [(bytes [rows, row bytes], mask)] per destination plane, still whole MCUs."""
    y, cb, cr, (my_, mc) = planes
    if cb is None:
        assert format in ("planar", "semiplanar") and chroma == "coded"
        return [(y, my_)]
    if chroma == "420":
        cb = ((cb[0::2].astype(np.uint16) + cb[1::2] + 1) >> 1).astype(np.uint8)
        cr = ((cr[0::2].astype(np.uint16) + cr[1::2] + 1) >> 1).astype(np.uint8)
        mc = mc[0::2]
    if format == "planar":
        return [(y, my_), (cb, mc), (cr, mc)]
    if format == "semiplanar":
        return [(y, my_), (_interleave(cb, cr), _interleave(mc, mc))]
    uv, muv = _interleave(cb, cr), _interleave(mc, mc)
    return [(_interleave(y, uv), _interleave(my_, muv)) if format == "yuyv" else (_interleave(uv, y), _interleave(muv, my_))]


def destination(planes, w, h, components, hs, vs, format="planar", chroma="coded", pitch=None, before=None):
    """The destination's bytes after the decode: uint8 [total] -- `before` (that many bytes; default zeros) with every byte a
    decoded MCU covers inside the planes' extents replaced."""
    lay, total = layout(w, h, components, hs, vs, format, chroma, pitch)
    out = np.zeros(total, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8, copy=True)
    assert out.size == total
    for (off, pt, row, _, rows), (val, mask) in zip(lay, formatted(planes, format, chroma)):
        val, mask = val[:rows, :row], mask[:rows, :row]
        for r in range(val.shape[0]):
            seg = out[off + r * pt: off + r * pt + val.shape[1]]
            seg[mask[r]] = val[r][mask[r]]
    return out


def views(buf, w, h, components, hs, vs, format="planar", chroma="coded", pitch=None):
    """The planes of a destination: [rows, row bytes] arrays cut out of `buf` (uint8 [total])."""
    lay, total = layout(w, h, components, hs, vs, format, chroma, pitch)
    return [np.stack([buf[off + r * pt: off + r * pt + row] for r in range(rows)]) for off, pt, row, _, rows in lay]


# ---- the host colour step --------------------------------------------------------------------------------------------

def colour(y, cb, cr, hs, vs, w, h, mask=None):
    """Planar planes (cut to their extents or whole MCUs) -> RGBA [h, w, 4]: chroma nearest neighbour, cs.rgba's integer
    colour step; pixels outside `mask` (bool, luma resolution) are zero, alpha included."""
    yy = y[:h, :w].astype(np.int32)
    if cb is None:
        r = g = b = yy
    else:
        cbu = np.repeat(np.repeat(cb, vs, axis=0), hs, axis=1)[:h, :w].astype(np.int32) - 128
        cru = np.repeat(np.repeat(cr, vs, axis=0), hs, axis=1)[:h, :w].astype(np.int32) - 128
        r = yy + ((45 * cru) >> 5)
        g = yy - ((11 * cbu + 23 * cru) >> 5)
        b = yy + ((113 * cbu) >> 6)
    out = np.stack([np.clip(r, 0, 255), np.clip(g, 0, 255), np.clip(b, 0, 255), np.full(yy.shape, 255)], axis=2).astype(np.uint8)
    if mask is not None:
        out[~mask[:h, :w]] = 0
    return out


# ---- the real encoders' files ----------------------------------------------------------------------------------------

def golden_files(ca, golden):
    """[(name, bytes, ImageData keywords)] of every JPEG under tests/golden the front end accepts with both extensions on."""
    import os
    out = []
    for sub in sorted(os.listdir(golden)):
        folder = os.path.join(golden, sub)
        for name in sorted(os.listdir(folder)) if os.path.isdir(folder) else []:
            if not name.endswith(".jpg"):
                continue
            with open(os.path.join(folder, name), "rb") as fh:
                j = fh.read()
            kw = dict(allow_sampling=True, allow_grayscale=True)
            try:
                ca.ImageData(j, **kw)
            except ca.Error:
                continue
            out.append((f"{sub}/{name}", j, kw))
    return out
