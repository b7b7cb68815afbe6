"""Expected values of the antialiased resized tensor output (include/compeg_hip.h, "Antialiased bilinear"), shared by
the CPU and GPU tests: the header's contract in numpy, the tables in float64 as the host makes them, the taps in
float32 with one array operation per line.  Prefilter, scale, bias, order and the conversions are resize_reference's."""
import numpy as np

import resize_reference as rr
from resize_reference import (DTYPES, ELEM_BYTES, IMAGENET_BIAS, IMAGENET_SCALE, frame, from_bytes, params, pre_extent,  # noqa: F401
                              prefilter, same, store)

F32 = np.float32
MAX_RATIO = 64   # the flag is rejected when pw > 64 * ow or ph > 64 * oh


def axis_table(n_out, n_in):
    """(first[n_out], count[n_out], w[T][n_out]) of one axis, T the largest count; a weight past an output's own count
    is 0."""
    if n_in <= n_out:   # the axis does not shrink: plain bilinear's two taps
        i0, _, w0, w1 = rr.axis_taps(n_out, n_in, "bilinear")
        return i0, np.full(n_out, 2, np.int64), np.stack([w0, w1])
    s = float(n_in) / float(n_out)
    c = s * (np.arange(n_out, dtype=np.float64) + 0.5)
    lo = np.maximum((c - s + 0.5).astype(np.int64), 0)     # (astype truncates toward zero)
    hi = np.minimum((c + s + 0.5).astype(np.int64), n_in)
    count = hi - lo
    assert count.min() >= 1
    t = np.arange(int(count.max()), dtype=np.int64)[:, None]
    inv = 1.0 / s
    u = np.maximum(0.0, 1.0 - np.abs((t + lo - c + 0.5) * inv))
    u[t >= count] = 0.0
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


def resample(p, size, fused=False):
    """m[3][oh][ow] from P, float32, horizontal first, every operation rounded on its own."""
    ow, oh = size
    ph, pw = p.shape[1:]
    fx, _, wx = axis_table(ow, pw)
    fy, _, wy = axis_table(oh, ph)
    h = p[:, :, np.minimum(fx, pw - 1)] * wx[0]
    for t in range(1, len(wx)):
        h = _accumulate(h, p[:, :, np.minimum(fx + t, pw - 1)], wx[t], fused)
    m = h[:, np.minimum(fy, ph - 1)] * wy[0][:, None]
    for t in range(1, len(wy)):
        m = _accumulate(m, h[:, np.minimum(fy + t, ph - 1)], wy[t][:, None], fused)
    assert m.dtype == F32
    return m


def expected(rgba, size, k, dtype, scale, bias, order="rgb", crop=None, fused=False):
    """[3, oh, ow] as the header defines it; size = (ow, oh), crop = (x, y, w, h) or None."""
    m = resample(prefilter(rgba, k, crop), size, fused)
    planes = []
    for c in range(3):
        v = m[c if order == "rgb" else 2 - c] * F32(scale[c])
        v = v + F32(bias[c])
        planes.append(v)
    return store(np.stack(planes), dtype)


def taps(n_out, n_in):
    """The largest tap count of an axis."""
    return int(axis_table(n_out, n_in)[1].max())
