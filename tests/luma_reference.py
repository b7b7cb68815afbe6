"""Expected values of the luma tensor output (include/compeg_hip.h, "Luma tensor output"), shared by the CPU and GPU
tests: the header's integer formula per source pixel, then orient_reference's upright slot of the RGBA whose R, G and B
are that L, in the order RGB with scale, bias and pad tripled, plane 0 kept.  Nothing of the resampling is restated.
tests/test_luma_reference.py holds the formula against PIL's convert("L")."""
import numpy as np

import orient_reference as orf

fr = orf.fr
BT601, BT709 = (19595, 38470, 7471), (13933, 46871, 4732)
PRESETS = {"bt601": BT601, "bt709": BT709, "r": (65536, 0, 0), "g": (0, 65536, 0), "b": (0, 0, 65536)}


def weights_of(weights):
    return PRESETS[weights] if isinstance(weights, str) else tuple(int(w) for w in weights)


def luma(rgba, weights=BT601):
    """[h, w] uint8 from [h, w, 3 or 4]: L = (wR R + wG G + wB B + 32768) >> 16 in unsigned 32-bit arithmetic."""
    wr, wg, wb = (np.uint32(w) for w in weights_of(weights))
    assert int(wr) + int(wg) + int(wb) == 65536
    p = rgba.astype(np.uint32)
    acc = p[..., 0] * wr + p[..., 1] * wg + p[..., 2] * wb + np.uint32(32768)
    assert acc.dtype == np.uint32
    return (acc >> np.uint32(16)).astype(np.uint8)


def grey_rgba(l):
    """The RGBA whose R, G and B are the plane l."""
    out = np.empty(l.shape + (4,), np.uint8)
    out[..., :3] = l[..., None]
    out[..., 3] = 255
    return out


def expected_of(l, size, k, dtype, scale, bias, kernel="bicubic", src=None, dst=None, pad=0.0, o=1):
    """One upright slot, [oh, ow], of the plane l of source-pixel values: plane 0 of orient_reference.expected on grey_rgba;
    scale, bias and pad are numbers."""
    return orf.expected(grey_rgba(l), size, k, dtype, (scale,) * 3, (bias,) * 3, "rgb", kernel, src, dst, (pad,) * 3, o)[0]


def expected(rgba, size, k, dtype, scale, bias, weights=BT601, kernel="bicubic", src=None, dst=None, pad=0.0, o=1):
    """One upright slot, [oh, ow]: expected_of the frame's L."""
    return expected_of(luma(rgba, weights), size, k, dtype, scale, bias, kernel, src, dst, pad, o)
