"""What a cropped decode of a region list (include/compeg_hip.h, "Cropped decode of a region list") must write, made on the
host.  A plain module (Python and numpy, no fixtures), shared by tests/test_crop_regions_stream.py (the expectation pinned
to tests/crop_stream.py's), tests/test_crop_regions_emulation.py (the emulated kernels) and tests/test_gpu_crop_regions.py
(the card).

The pieces are crop_stream's: a frame's full RGBA and the mask of the pixels a decoded MCU covers (crs.frame_rgba).  Per
region the rectangle is cut out of its image's two and laid at (dst_x, dst_y) of slot k over whatever was there.  The shape
and the grouping -- which regions go into which launch -- are restated here and compared with the library in the tests.
Also here: the mixed batch and the region list the three test files share."""
import numpy as np

import crop_stream as crs
import planes_stream as ps

FORMATS = crs.FORMATS
GROUPS = ("422", "444", "440", "420", "gray")   # the launches' order
GRID_ROWS = 65535


# ---- the shape, restated ---------------------------------------------------------------------------------------------

def shape(slot, format="rgba", pitch=None):
    """-> (pitch, bytes of one slot) for slots of slot = (width, height) pixels: rgba rows of 4 width bytes at `pitch` (None
    or 0: tight), the last row at its full pitch; rgb_planar a tight [3, height, width] block whose pitch is the width."""
    sw, sh = slot
    assert 1 <= sw <= 65535 and 1 <= sh <= 65535
    if format == "rgb_planar":
        assert not pitch
        return sw, 3 * sw * sh
    pt = pitch or 4 * sw
    assert pt >= 4 * sw and pt % 4 == 0
    return pt, pt * sh


def normal(region):
    """(image, (x, y, w, h), (dst_x, dst_y)) of either tuple form."""
    return (region[0], tuple(region[1]), tuple(region[2]) if len(region) == 3 else (0, 0))


def fits(slot, w, h, region):
    """Whether the library must accept the region for a w x h image: non-empty, inside the image, inside the slot."""
    _, (x, y, rw, rh), (dx, dy) = normal(region)
    return rw >= 1 and rh >= 1 and x + rw <= w and y + rh <= h and dx + rw <= slot[0] and dy + rh <= slot[1]


def slot_of(regions):
    """slot=None: the largest dst_x + w and dst_y + h of the list."""
    rs = [normal(r) for r in regions]
    return max(d[0] + r[2] for _, r, d in rs), max(d[1] + r[3] for _, r, d in rs)


# ---- the destination -------------------------------------------------------------------------------------------------

def destination(fulls, regions, slot, format="rgba", pitch=None, before=None):
    """The destination's bytes after the decode: uint8 [count * slot bytes] -- `before` (that many bytes; default zeros) with,
    per region, the bytes of every pixel of its rectangle that a decoded MCU covers replaced.  fulls[i]: image i's
    (RGBA, mask) -- crs.frame_rgba's."""
    pt, slot_bytes = shape(slot, format, pitch)
    sw, sh = slot
    out = np.zeros(len(regions) * slot_bytes, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8, copy=True)
    assert out.size == len(regions) * slot_bytes
    for k, region in enumerate(regions):
        image, (x, y, rw, rh), (dx, dy) = normal(region)
        rgba, mask = fulls[image]
        assert fits(slot, mask.shape[1], mask.shape[0], region)
        px, m = rgba[y:y + rh, x:x + rw], mask[y:y + rh, x:x + rw]
        one = out[k * slot_bytes:(k + 1) * slot_bytes]
        for r in range(rh):
            if format == "rgba":
                at = (dy + r) * pt + 4 * dx
                row = one[at:at + 4 * rw].reshape(rw, 4)
                row[m[r]] = px[r][m[r]]
            else:
                for c in range(3):
                    at = c * sw * sh + (dy + r) * sw + dx
                    row = one[at:at + rw]
                    row[m[r]] = px[r, :, c][m[r]]
    return out


# ---- the grouping, restated ------------------------------------------------------------------------------------------

def launches(layouts, regions, chunk=0):
    """[(layout, [region indices])]: one run of launches per sampling present among the images the regions name, in GROUPS'
    order, the regions of a group in the list's order, each group split at `chunk` regions (0: none) and at the grid's
    65535 rows.  layouts[i]: image i's layout name."""
    out = []
    step = min(chunk or GRID_ROWS, GRID_ROWS)
    for g in GROUPS:
        ks = [k for k, r in enumerate(regions) if layouts[r[0]] == g]
        out += [(g, ks[at:at + step]) for at in range(0, len(ks), step)]
    return out


# ---- the mixed batch and its region list -----------------------------------------------------------------------------

SHORT = 8   # the batch's index of the frame with an MCU behind its last complete interval
BIG = 7     # ... of the 640 x 384 frame


def mixed_batch():
    """[(frame, layout)]: 324 x 70 in each of the five samplings at restart intervals that wrap MCU rows (one without DRI),
    entropy modes alternating; 8 x 8; 1 x 1; 640 x 384 4:2:2 at DRI 1 (1920 intervals: untouched waves and workgroups);
    3 x 3 MCUs of 4:2:2 at DRI 4 with the ninth MCU behind the last complete interval."""
    w, h = crs.SIZE
    picks = (("422", 0), ("444", 9), ("440", 5), ("420", 35), ("gray", 9))   # (MCU rows of 21, 41, 41, 21 and 41)
    assert all(ri in crs.DRIS[lay] for lay, ri in picks)
    frames = [(ps.sized(lay, w, h, ri, standard=i % 2 == 1, seed=3 + i), lay) for i, (lay, ri) in enumerate(picks)]
    frames.append((ps.sized("420", 8, 8, 0, seed=1), "420"))
    frames.append((ps.sized("444", 1, 1, 0, standard=True, seed=2), "444"))
    frames.append((ps.sized("422", 640, 384, 1, seed=11), "422"))
    frames.append((ps.sized("422", 48, 23, 4, seed=2, short=3), "422"))
    assert frames[BIG][0].intervals == 1920 and "/short" in frames[SHORT][0].name
    return frames


def mixed_fulls(frames, ca):
    """crs.frame_rgba of every frame (ca: the package, for the short frame's oracle pass), the masks checked: all true but
    the short frame's, where exactly the ninth MCU is missing."""
    fulls = [crs.frame_rgba(f, ca=ca) for f, _ in frames]
    for i, (rgba, mask) in enumerate(fulls):
        if i != SHORT:
            assert mask.all(), frames[i][0].name
    want = np.ones((23, 48), dtype=bool)
    want[16:, 32:] = False
    assert np.array_equal(fulls[SHORT][1], want), "the short frame must lack exactly its ninth MCU"
    return fulls


SLOT = (325, 71)   # one more than the largest rectangle each way: a dst of 1 still fits the whole 324 x 70 frame


def mixed_regions():
    """The region list over mixed_batch(): crs.RECTS spread over the 324 x 70 frames; several regions on one image and none on
    another (the 1 x 1 frame's only region is dropped from image 5: the 8 x 8 frame has none); images and samplings out of
    order; a whole-image region and a one-pixel region; a region inside the undecoded MCU; dst of 0, of 1 (which breaks the
    16-byte alignment) and flush with the slot's right and bottom edge."""
    sw, sh = SLOT
    out = []
    for n, rect in enumerate(crs.RECTS):
        image = (3, 0, 4, 1, 2)[n % 5]   # neither images nor samplings in order
        place = ((0, 0), (1, 0), (sw - rect[2], sh - rect[3]), (1, 1), (0, 1))[n % 5]
        out.append((image, rect, place))
    out += [
        (BIG, (100, 85, 200, 19), (1, 3)),            # MCU rows 10 .. 12 of 1920 intervals: untouched waves and workgroups
        (SHORT, (33, 17, 14, 5), (2, 2)),             # inside the undecoded MCU: nothing may be written
        (6, (0, 0, 1, 1), (sw - 1, sh - 1)),          # the 1 x 1 frame, flush with the slot's corner
        (0, (37, 11, 150, 41), (sw - 150, 0)),        # image 0 again, flush right
        (SHORT, (0, 0, 48, 23), (0, sh - 23)),        # the whole short frame, flush bottom
        (BIG, (333, 200, 1, 1), (4, 0)),              # one pixel of the large frame
        (0, (0, 0, 324, 70), (0, 0)),                 # a whole image, aligned
        (2, (5, 3, 301, 60), (3, 2)),
    ]
    assert {r[0] for r in out} == {0, 1, 2, 3, 4, 6, BIG, SHORT}   # (image 5 is named by none)
    return out
