"""Expected values of the filtered tensor output (include/compeg_hip.h, "Filtered tensor output"), shared by the CPU
and GPU tests: the header's contract in numpy, the tables in float64 as the host makes them, the taps in float32 with
one array operation per line.  Prefilter, scale, bias, order and the conversions are resize_reference's, the pad and
the placement region_reference's."""
import math

import numpy as np

import region_reference as gr
from region_reference import (DTYPES, ELEM_BYTES, IDENTITY, IMAGENET_BIAS, IMAGENET_SCALE, U8_BIAS, U8_SCALE, fit,  # noqa: F401
                              frame, from_bytes, pad_values, params, pre_extent, same, store)
from resize_reference import prefilter

F32 = np.float32
KERNELS = ("box", "triangle", "bicubic", "lanczos3")
TWICE_SUPPORT = {"box": 1, "triangle": 2, "bicubic": 4, "lanczos3": 6}   # 2S
MAX_TAPS_RATIO = 128   # an axis is rejected when n * 2S > 128 * o


_sin = np.frompyfunc(math.sin, 1, 1)


def _f(kernel, z):
    """The kernel function on a float64 array."""
    if kernel == "box":
        return np.where((z > -0.5) & (z <= 0.5), 1.0, 0.0)
    if kernel == "triangle":
        return np.maximum(0.0, 1.0 - np.abs(z))
    if kernel == "bicubic":
        a, q = -0.5, np.abs(z)
        near = ((a + 2.0) * q - (a + 3.0)) * q * q + 1.0
        far = (((q - 5.0) * q + 8.0) * q - 4.0) * a
        return np.where(q < 1.0, near, np.where(q < 2.0, far, 0.0))
    assert kernel == "lanczos3"

    def sinc(v):   # (math.sin: the C library's, as the host has it; numpy's own may differ in the last bit)
        pv = np.pi * np.where(v == 0.0, 1.0, v)
        return np.where(v == 0.0, 1.0, _sin(pv).astype(np.float64) / pv)
    return np.where((z >= -3.0) & (z < 3.0), sinc(z) * sinc(z / 3.0), 0.0)


def axis_ok(kernel, n_in, n_out):
    return n_in * TWICE_SUPPORT[kernel] <= MAX_TAPS_RATIO * n_out


def axis_table(kernel, n_out, n_in):
    """(first[n_out], count[n_out], w[T][n_out]) of one axis, T the largest count; a weight past an output's own count
    is 0."""
    s = float(n_in) / float(n_out)
    sc = max(s, 1.0)
    sup = (TWICE_SUPPORT[kernel] / 2.0) * sc
    inv = 1.0 / sc
    c = s * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum((c - sup + 0.5).astype(np.int64), 0)     # (astype truncates toward zero)
    hi = np.minimum((c + sup + 0.5).astype(np.int64), n_in)
    count = hi - lo
    assert count.min() >= 1
    t = np.arange(int(count.max()), dtype=np.int64)[:, None]
    u = _f(kernel, ((t + lo).astype(np.float64) - c + 0.5) * inv)
    u[np.broadcast_to(t, u.shape) >= count] = 0.0
    total = u[0].copy()
    for row in u[1:]:
        total = total + row
    w = (u / total).astype(F32)
    return lo, count, w


def _accumulate(acc, p, w, fused):
    if fused:   # the mutant: what a compiler's fma would give
        return (p.astype(np.float64) * w.astype(np.float64) + acc.astype(np.float64)).astype(F32)
    q = p * w
    return acc + q


def resample(p, size, kernel, fused=False):
    """m[3][oh][ow] from P, float32, horizontal first, every operation rounded on its own.  An output's taps are its
    own count of them: a tap past it is not added (it would read beyond the axis)."""
    ow, oh = size
    ph, pw = p.shape[1:]
    fx, cx, wx = axis_table(kernel, ow, pw)
    fy, cy, wy = axis_table(kernel, oh, ph)
    h = p[:, :, fx] * wx[0]
    for t in range(1, len(wx)):
        more = _accumulate(h, p[:, :, np.minimum(fx + t, pw - 1)], wx[t], fused)
        h = np.where(t < cx, more, h)
    m = h[:, fy] * wy[0][:, None]
    for t in range(1, len(wy)):
        more = _accumulate(m, h[:, np.minimum(fy + t, ph - 1)], wy[t][:, None], fused)
        m = np.where((t < cy)[:, None], more, m)
    assert m.dtype == F32
    return m


def inner(rgba, extent, k, dtype, scale, bias, order="rgb", kernel="bicubic", crop=None, fused=False):
    """[3, dh, dw]: the crop, prefiltered and resampled to the extent (dw, dh), scaled, biased and converted."""
    m = resample(prefilter(rgba, k, crop), extent, kernel, fused)
    planes = []
    for c in range(3):
        v = m[c if order == "rgb" else 2 - c] * F32(scale[c])
        v = v + F32(bias[c])
        planes.append(v)
    return store(np.stack(planes), dtype)


def expected(rgba, size, k, dtype, scale, bias, order="rgb", kernel="bicubic", src=None, dst=None, pad=(0, 0, 0), fused=False):
    """One slot, [3, oh, ow]: size = (ow, oh), src = (x, y, w, h) or None (the whole image), dst = (dx, dy, dw, dh) or
    None (the whole output)."""
    ow, oh = size
    dx, dy, dw, dh = dst if dst is not None else (0, 0, ow, oh)
    assert dw >= 1 and dh >= 1 and dx + dw <= ow and dy + dh <= oh
    p = pad_values(pad, dtype, scale, bias, order)
    out = np.empty((3, oh, ow), p.dtype)
    out[:] = p[:, None, None]
    out[:, dy:dy + dh, dx:dx + dw] = inner(rgba, (dw, dh), k, dtype, scale, bias, order, kernel, crop=src, fused=fused)
    return out


def taps(kernel, n_out, n_in):
    """The largest tap count of an axis."""
    return int(axis_table(kernel, n_out, n_in)[1].max())


def abs_weight_sum(kernel, n_out, n_in):
    """The largest sum of |w_t| over an axis' outputs."""
    return float(np.abs(axis_table(kernel, n_out, n_in)[2].astype(np.float64)).sum(axis=0).max())
