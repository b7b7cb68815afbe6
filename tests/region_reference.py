"""Expected values of the region tensor output (include/compeg_hip.h, "Region tensor output"), shared by the CPU and
GPU tests: the header's contract in numpy.  The inner rectangle of a slot is resize_reference.expected or
antialias_reference.expected at the inner extent, placed; every other element is the pad value put through the same
two rounded float32 operations and the same conversions."""
import numpy as np

import antialias_reference as ar
import resize_reference as rr
from resize_reference import (DTYPES, ELEM_BYTES, IDENTITY, IMAGENET_BIAS, IMAGENET_SCALE, U8_BIAS, U8_SCALE,  # noqa: F401
                              frame, from_bytes, params, pre_extent, same, store)

F32 = np.float32
FILTERS = ("nearest", "bilinear", "antialias")   # the third: bilinear with the antialias flag
# five images of five sizes, and seven regions over them, repeated and out of order: (image, src or None, dst or None)
# for a 24 x 20 output
FIVE = ((16, 8), (17, 9), (50, 26), (66, 26), (330, 70))
SEVEN = ((4, (101, 3, 200, 64), (2, 4, 20, 6)), (0, None, None), (2, (3, 1, 45, 21), (0, 3, 24, 11)), (4, None, (0, 7, 24, 5)),
         (2, (3, 1, 45, 21), (0, 3, 24, 11)), (1, (5, 2, 12, 7), (7, 0, 9, 20)), (3, (2, 0, 64, 26), (23, 19, 1, 1)))


def fit(src_size, out_size, align="center"):
    """compeg_region_fit in Python integers: (dx, dy, dw, dh)."""
    (sw, sh), (ow, oh) = src_size, out_size
    if ow * sh <= oh * sw:
        dw, dh = ow, min(max((2 * sh * ow + sw) // (2 * sw), 1), oh)
    else:
        dw, dh = min(max((2 * sw * oh + sh) // (2 * sh), 1), ow), oh
    return ((ow - dw) // 2, (oh - dh) // 2, dw, dh) if align == "center" else (0, 0, dw, dh)


def pad_values(pad, dtype, scale, bias, order="rgb"):
    """The stored pad element of each plane: v = (pad[ch] * scale[c]) + bias[c], ch the plane's source channel."""
    planes = []
    for c in range(3):
        v = np.array(F32(pad[c if order == "rgb" else 2 - c])) * F32(scale[c])
        v = v + F32(bias[c])
        assert v.dtype == F32
        planes.append(v)
    with np.errstate(over="ignore"):   # (a pad beyond f16 is an infinity, as on the card)
        return store(np.stack(planes), dtype)


def inner(rgba, extent, k, dtype, scale, bias, order="rgb", filter="bilinear", crop=None):
    """[3, dh, dw]: what compeg_*_pack_tensor_resized gives for the crop at the output extent (dw, dh)."""
    if filter == "antialias":
        return ar.expected(rgba, extent, k, dtype, scale, bias, order, crop)
    return rr.expected(rgba, extent, k, dtype, scale, bias, order, filter, crop)


def expected(rgba, size, k, dtype, scale, bias, order="rgb", filter="bilinear", src=None, dst=None, pad=(0, 0, 0)):
    """One slot, [3, oh, ow]: size = (ow, oh), src = (x, y, w, h) or None (the whole image), dst = (dx, dy, dw, dh) or
    None (the whole output)."""
    ow, oh = size
    dx, dy, dw, dh = dst if dst is not None else (0, 0, ow, oh)
    assert dw >= 1 and dh >= 1 and dx + dw <= ow and dy + dh <= oh
    p = pad_values(pad, dtype, scale, bias, order)
    out = np.empty((3, oh, ow), p.dtype)
    out[:] = p[:, None, None]
    out[:, dy:dy + dh, dx:dx + dw] = inner(rgba, (dw, dh), k, dtype, scale, bias, order, filter, src)
    return out
