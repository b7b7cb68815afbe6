"""Expected values of the oriented tensor output (include/compeg_hip.h, "Oriented tensor output"), shared by the CPU
and GPU tests: filter_reference's slot T, put through the EXIF orientation as the header's table has it.  The table is
PIL's (Image.transpose, ImageOps.exif_transpose): tests/test_orient_reference.py holds `orient` against both."""
import numpy as np

import filter_reference as fr

ORIENTATIONS = (1, 2, 3, 4, 5, 6, 7, 8)
# what PIL calls each (Image.Transpose), for the tests that compare with it
PIL_TRANSPOSE = {2: "FLIP_LEFT_RIGHT", 3: "ROTATE_180", 4: "FLIP_TOP_BOTTOM", 5: "TRANSPOSE", 6: "ROTATE_270", 7: "TRANSVERSE", 8: "ROTATE_90"}
# EIGHT of the GPU and emulation tests: (image of region_reference.FIVE, src, dst in the upright 24 x 20 slot, orientation)
SLOT = (24, 20)
EIGHT = ((4, (101, 3, 64, 60), (2, 4, 20, 6), 1), (2, (3, 1, 45, 21), (0, 3, 24, 11), 2), (4, None, (0, 7, 24, 5), 3), (1, (5, 2, 12, 7), (7, 0, 9, 20), 4),
         (2, (3, 1, 45, 21), (1, 3, 11, 13), 5), (4, (101, 3, 120, 64), (2, 4, 20, 6), 6), (3, (2, 0, 20, 16), (23, 19, 1, 1), 7), (0, None, (0, 0, 24, 20), 8))


def transposes(o):
    return o >= 5


def orient(a, o):
    """U from T: the last two axes of `a` are (rows, columns) of T; the result's are U's."""
    assert o in ORIENTATIONS
    t = np.swapaxes(a, -1, -2) if transposes(o) else a   # U[y][x] = T[x][y]
    # (on the transposed array: 6 mirrors columns -- U[y][x] = T'[y][ow-1-x], T'[y][x] = T[x][y] --, 8 rows, 7 both)
    if o in (2, 3, 6, 7):
        t = t[..., :, ::-1]
    if o in (3, 4, 7, 8):
        t = t[..., ::-1, :]
    return np.ascontiguousarray(t)


def slot_extent(size, o):
    """T's (width, height) for the upright size = (ow, oh)."""
    return (size[1], size[0]) if transposes(o) else tuple(size)


def preimage(rect, o, size):
    """dst' in T of the rectangle rect = (dx, dy, dw, dh) of the upright slot of size = (ow, oh)."""
    (dx, dy, dw, dh), (ow, oh) = rect, size
    assert o in ORIENTATIONS and dx + dw <= ow and dy + dh <= oh
    fx, fy = ow - dx - dw, oh - dy - dh
    return {1: (dx, dy, dw, dh), 2: (fx, dy, dw, dh), 3: (fx, fy, dw, dh), 4: (dx, fy, dw, dh),
            5: (dy, dx, dh, dw), 6: (dy, fx, dh, dw), 7: (fy, fx, dh, dw), 8: (fy, dx, dh, dw)}[o]


def expected(rgba, size, k, dtype, scale, bias, order="rgb", kernel="bicubic", src=None, dst=None, pad=(0, 0, 0), o=1):
    """One upright slot, [3, oh, ow]: filter_reference.expected of {src, dst'} at T's extent, oriented."""
    ow, oh = size
    full = dst if dst is not None else (0, 0, ow, oh)
    t = fr.expected(rgba, slot_extent(size, o), k, dtype, scale, bias, order, kernel, src, preimage(full, o, size), pad)
    return orient(t, o)


def exif_app1(o, little=True, where="only", tag=0x0112, kind=3, count=1):
    """An APP1 segment (marker and length included) whose IFD0 holds the orientation entry first, last or alone among
    other entries ("absent": only the others)."""
    e = "<" if little else ">"
    import struct

    def entry(t, ty, n, value):
        return struct.pack(e + "HHI", t, ty, n) + (struct.pack(e + "HH", value, 0) if ty == 3 else struct.pack(e + "I", value))
    others = [entry(0x011A, 5, 1, 200), entry(0x0128, 3, 1, 2)]   # XResolution (an offset), ResolutionUnit
    mine = entry(tag, kind, count, o)
    entries = {"only": [mine], "first": [mine] + others, "last": others + [mine], "absent": others}[where]
    ifd = struct.pack(e + "H", len(entries)) + b"".join(entries) + struct.pack(e + "I", 0)
    tiff = (b"II*\0" if little else b"MM\0*") + struct.pack(e + "I", 8) + ifd
    tiff += b"\0" * (200 + 8 - len(tiff)) if len(tiff) < 208 else b""   # (room for the rational at offset 200)
    payload = b"Exif\0\0" + tiff
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def splice(jpeg, segment):
    """`segment` behind SOI."""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + segment + jpeg[2:]
