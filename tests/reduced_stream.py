"""What a reduced decode (include/compeg_hip.h, "Reduced-size decode") must write, made on the host.  A plain module (Python
and numpy, no fixtures), shared by tests/test_reduced_stream.py (the expectation pinned to the oracle's own transform and
colour step), tests/test_reduced_emulation.py (the emulated lane body) and tests/test_gpu_reduced.py (the card).

The chain: the dequantised coefficients the reference keeps (cs.predict for frames written from coefficients; the oracle's
own orc_huffman_pass / orc_huffman_pass_ext for real encoders' files, as ps.file_planes takes them) -> columns 1..63 set to
zero -> cs.samples -> ps.whole_planes, masks included -> [::8, ::8] of every plane: one sample per data unit -> ps.colour at
the reduced extent -> the two formats laid into the destination over whatever was there before.  compeg_reduced_shape is
restated here and compared with the library in the tests."""
import ctypes as C

import numpy as np

import coef_stream as cs
import planes_stream as ps
from oracle import oracle as orc

FORMATS = ("rgba", "rgb_planar")


# ---- the shape, restated ---------------------------------------------------------------------------------------------

def shape(w, h, format="rgba", pitch=None):
    """-> (ow, oh, pitch, total bytes of one image): ow x oh = ceil(w / 8) x ceil(h / 8); rgba rows at `pitch` (None or 0:
    tight, 4 ow), the last row at its full pitch; rgb_planar a tight [3, oh, ow] block whose pitch is ow."""
    ow, oh = -(-w // 8), -(-h // 8)
    if format == "rgb_planar":
        assert not pitch
        return ow, oh, ow, 3 * ow * oh
    pt = pitch or 4 * ow
    assert pt >= 4 * ow and pt % 4 == 0
    return ow, oh, pt, pt * oh


# ---- one sample per data unit ----------------------------------------------------------------------------------------

def dc_sample(dc, mutant=None):
    """The header's formula on int32 DC terms: trunc(clamp(f32(dc) * 0.125f + 128.5f, 0, 255)), every step one f32
    operation.  mutant: "rint" (to nearest in place of the truncation) or "bias128" (128 in place of 128.5)."""
    f = np.asarray(dc).astype(np.int32).astype(np.float32) * np.float32(0.125)
    f = f + np.float32(128.0 if mutant == "bias128" else 128.5)
    f = np.minimum(np.maximum(f, np.float32(0)), np.float32(255))
    return (np.rint(f) if mutant == "rint" else np.trunc(f)).astype(np.uint8)


def zero_ac(coef):
    z = np.array(coef, copy=True)
    z[:, 1:] = 0
    return z


def reduced_planes(coef, dpm, hs, vs, mcus_w, mcus_h, mutant=None):
    """Coefficients [data units of the decoded MCUs, 64] -> (Y, Cb, Cr, mask) at one sample per data unit: Y and the mask
    [mcus_h vs, mcus_w hs], Cb and Cr [mcus_h, mcus_w] (None for one component).  The chain of the module's docstring; with
    a mutant, dc_sample gone wrong in that way stands in for cs.samples."""
    z = zero_ac(coef)
    if mutant is None:
        smp = cs.samples(z)
    else:
        smp = np.repeat(dc_sample(z[:, 0], mutant)[:, None], 64, axis=1).reshape(-1, 8, 8)
    y, cb, cr, (my, _) = ps.whole_planes(smp, dpm, hs, vs, mcus_w, mcus_h)
    cut = (lambda a: None if a is None else a[::8, ::8])
    return cut(y), cut(cb), cut(cr), cut(my)


def file_coefficients(ca, jpeg, **kw):
    """A real encoder's file (or any frame's bytes): the oracle's own entropy pass over the image's metadata block, LUTs
    and preprocessed scan, as ps.file_planes runs it.  -> (int32 [data units, 64], (w, h, comps, hs, vs, dpm, mcus_w, mcus_h),
    the metadata block)."""
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
    hs, vs = img.sampling()
    w, h = img.width(), img.height()
    return full, (w, h, img.components(), hs, vs, dpm, mcus_w, -(-h // (8 * vs))), bufs[0]


def frame_reduced(f, mutant=None, ca=None):
    """A coefficient frame's reduced planes.  A frame with MCUs behind its last complete interval ("/short" in its name)
    has a segment more in its scan than its header counts: what the reference makes of that is the oracle's to say, so
    its coefficients come from file_coefficients (ca: the package)."""
    comps, hs, vs = ps.sampling_of(f)
    if f.family == "sized" and "/short" in f.name:
        coef = file_coefficients(ca, f.jpeg(), **f.image_kw())[0]
    else:
        coef = cs.predict(f)
    return reduced_planes(coef, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h, mutant)


def file_reduced(ca, jpeg, **kw):
    """-> (reduced planes, (w, h, comps, hs, vs))."""
    coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), _ = file_coefficients(ca, jpeg, **kw)
    return reduced_planes(coef, dpm, hs, vs, mcus_w, mcus_h), (w, h, comps, hs, vs)


def rgba(red, w, h, hs, vs):
    """Reduced planes -> (RGBA [oh, ow, 4] with undecoded pixels zero, mask [oh, ow]): chroma nearest neighbour, the
    integer colour step, A = 255."""
    y, cb, cr, mask = red
    ow, oh = -(-w // 8), -(-h // 8)
    return ps.colour(y, cb, cr, hs, vs, ow, oh, mask), mask[:oh, :ow]


# ---- the destination -------------------------------------------------------------------------------------------------

def destination(red, w, h, hs, vs, format="rgba", pitch=None, before=None):
    """The destination's bytes after the decode: uint8 [total] -- `before` (that many bytes; default zeros) with the bytes
    of every pixel a decoded MCU covers inside ow x oh replaced."""
    ow, oh, pt, total = shape(w, h, format, pitch)
    px, mask = rgba(red, w, h, hs, vs)
    out = np.zeros(total, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8, copy=True)
    assert out.size == total
    for r in range(oh):
        if format == "rgba":
            row = out[r * pt: r * pt + 4 * ow].reshape(ow, 4)
            row[mask[r]] = px[r][mask[r]]
        else:
            for c in range(3):
                row = out[c * ow * oh + r * ow: c * ow * oh + (r + 1) * ow]
                row[mask[r]] = px[r, :, c][mask[r]]
    return out


def view(buf, w, h, format="rgba", pitch=None):
    """A destination's pixels: RGBA [oh, ow, 4] (A = 255 for the planar format) cut out of `buf` (uint8 [total])."""
    ow, oh, pt, total = shape(w, h, format, pitch)
    if format == "rgba":
        return np.stack([buf[r * pt: r * pt + 4 * ow].reshape(ow, 4) for r in range(oh)])
    rgb = buf[:3 * ow * oh].reshape(3, oh, ow).transpose(1, 2, 0)
    return np.concatenate([rgb, np.full((oh, ow, 1), 255, dtype=np.uint8)], axis=2)
