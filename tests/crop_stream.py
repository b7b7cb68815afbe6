"""What a cropped decode (include/compeg_hip.h, "Cropped decode") must write, made on the host.  A plain module (Python and
numpy, no fixtures), shared by tests/test_crop_stream.py (the expectation pinned to the oracle's RGBA),
tests/test_crop_emulation.py (the emulated lane body and touch test) and tests/test_gpu_crop.py (the card).

The chain: the full RGBA of a frame and the mask of the pixels a decoded MCU covers -- ps.frame_planes (ps.file_planes for
real encoders' files and for frames with MCUs behind their last complete interval) through ps.colour, which for one
component is gs.expectation -- then the rectangle cut out of both and laid, in either format, into the destination over
whatever was there before.  compeg_crop_shape and the kernels' touch test are restated here, the latter by going through an
interval's MCUs one by one, and compared with the library in the tests."""
import numpy as np

import planes_stream as ps

FORMATS = ("rgba", "rgb_planar")
# 324 x 70 in every sampling (tests/planes_stream.py: sized): both edges cut an MCU.  The restart intervals divide the MCU
# counts 189 / 105 / 369 / 205 / 369; 9, 63, 5, 35 and 123 wrap over the end of an MCU row or span several; 0: no DRI.
DRIS = {"422": (1, 3, 9, 21, 63, 0), "420": (3, 5, 35), "444": (3, 9, 41, 123), "440": (5, 41), "gray": (3, 9)}
SIZE = (324, 70)
RECTS = ((0, 0, 324, 70),      # the whole frame
         (0, 0, 1, 1), (323, 69, 1, 1),   # one pixel
         (37, 11, 150, 41),    # off the MCU grid both ways, an odd x that splits a chroma pair
         (160, 16, 16, 16),    # MCU-aligned
         (100, 0, 3, 70),      # a column
         (0, 31, 324, 2),      # two rows astride an MCU row border for 8- and 16-row MCUs
         (300, 60, 24, 10))    # the cut corner


# ---- the shape, restated ---------------------------------------------------------------------------------------------

def shape(w, h, rect, format="rgba", pitch=None):
    """-> (pitch, total bytes of one image) for rect = (x, y, rw, rh) inside w x h: rgba rows of 4 rw bytes at `pitch` (None
    or 0: tight), the last row at its full pitch; rgb_planar a tight [3, rh, rw] block whose pitch is rw."""
    x, y, rw, rh = rect
    assert rw >= 1 and rh >= 1 and x >= 0 and y >= 0 and x + rw <= w and y + rh <= h
    if format == "rgb_planar":
        assert not pitch
        return rw, 3 * rw * rh
    pt = pitch or 4 * rw
    assert pt >= 4 * rw and pt % 4 == 0
    return pt, pt * rh


# ---- the full decode and what of it was decoded at all ---------------------------------------------------------------

def planes_rgba(planes, w, h, hs, vs):
    """Whole-MCU planes (ps.whole_planes) -> (RGBA [h, w, 4] with undecoded pixels zero, mask [h, w])."""
    y, cb, cr, (my, _) = planes
    return ps.colour(y, cb, cr, hs, vs, w, h, my), my[:h, :w]


def frame_rgba(f, ca=None):
    """A coefficient frame's full decode and mask.  A frame with MCUs behind its last complete interval ("/short" in its
    name) has a segment more in its scan than its header counts: what the reference makes of that is the oracle's to say,
    so it goes through ps.file_planes (ca: the package)."""
    comps, hs, vs = ps.sampling_of(f)
    if f.family == "sized" and "/short" in f.name:
        planes, _ = ps.file_planes(ca, f.jpeg(), **f.image_kw())
    else:
        planes = ps.frame_planes(f)
    return planes_rgba(planes, f.w, f.h, hs, vs)


def file_rgba(ca, jpeg, **kw):
    """A real encoder's file -> (RGBA, mask, (w, h, comps, hs, vs))."""
    planes, (w, h, comps, hs, vs) = ps.file_planes(ca, jpeg, **kw)
    return planes_rgba(planes, w, h, hs, vs) + ((w, h, comps, hs, vs),)


# ---- the destination -------------------------------------------------------------------------------------------------

def destination(rgba, mask, rect, format="rgba", pitch=None, before=None):
    """The destination's bytes after the decode: uint8 [total] -- `before` (that many bytes; default zeros) with the bytes of
    every pixel of the rectangle that a decoded MCU covers replaced."""
    h, w = mask.shape
    x, y, rw, rh = rect
    pt, total = shape(w, h, rect, format, pitch)
    px, m = rgba[y:y + rh, x:x + rw], mask[y:y + rh, x:x + rw]
    out = np.zeros(total, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8, copy=True)
    assert out.size == total
    for r in range(rh):
        if format == "rgba":
            row = out[r * pt: r * pt + 4 * rw].reshape(rw, 4)
            row[m[r]] = px[r][m[r]]
        else:
            for c in range(3):
                row = out[c * rw * rh + r * rw: c * rw * rh + (r + 1) * rw]
                row[m[r]] = px[r, :, c][m[r]]
    return out


def view(buf, rect, format="rgba", pitch=None):
    """A destination's pixels: RGBA [rh, rw, 4] (A = 255 for the planar format) cut out of `buf` (uint8 [total])."""
    x, y, rw, rh = rect
    if format == "rgba":
        pt = pitch or 4 * rw
        return np.stack([buf[r * pt: r * pt + 4 * rw].reshape(rw, 4) for r in range(rh)])
    rgb = buf[:3 * rw * rh].reshape(3, rh, rw).transpose(1, 2, 0)
    return np.concatenate([rgb, np.full((rh, rw, 1), 255, dtype=np.uint8)], axis=2)


# ---- the touch test, by going through the MCUs -----------------------------------------------------------------------

def mcu_box(rect, mcu_w, mcu_h):
    """(mx0, mx1, my0, my1): MCU columns mx0 .. mx1 - 1 and rows my0 .. my1 - 1 have a pixel in the rectangle."""
    x, y, rw, rh = rect
    return x // mcu_w, (x + rw - 1) // mcu_w + 1, y // mcu_h, (y + rh - 1) // mcu_h + 1


def reach(k, dri, total_mcus, wm, box):
    """Interval k holds MCUs k dri .. k dri + dri - 1 in raster order, cut at the image's MCUs (dri 0: all of them): the
    count from its first MCU up to and with its last one inside the box, 0 if none is -- the interval does not touch."""
    per = dri or total_mcus
    mx0, mx1, my0, my1 = box
    out = 0
    for m in range(k * per, min(k * per + per, total_mcus)):
        my, mx = divmod(m, wm)
        if mx0 <= mx < mx1 and my0 <= my < my1:
            out = m - k * per + 1
    return out


def touch_cases():
    """[(wm, total MCUs, dri as the kernels see it, box, interval, reach)] for every sampling's 324 x 70 frame, every DRI of
    the table and every rectangle of the list, every interval."""
    out = []
    for layout, dris in DRIS.items():
        hs, vs = ps.SAMPLINGS[layout]
        mw, mh = 8 * hs, 8 * vs
        wm, hm = -(-SIZE[0] // mw), -(-SIZE[1] // mh)
        for dri in dris:
            per = dri or wm * hm
            for rect in RECTS:
                box = mcu_box(rect, mw, mh)
                for k in range(wm * hm // per):
                    out.append((wm, wm * hm, per, box, k, reach(k, per, wm * hm, wm, box)))
    return out
