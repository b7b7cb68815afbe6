"""Expected values of the resized tensor output (include/compeg_hip.h, "Resized tensor output"), shared by the CPU
and GPU tests: the oracle's RGBA put through the header's formula in numpy float32, one array operation per line of
the header.  Frames, parameters, the comparison and the element types are tensor_reference's."""
import numpy as np

import tensor_reference as tr
from tensor_reference import (DTYPES, ELEM_BYTES, IDENTITY, IMAGENET_BIAS, IMAGENET_SCALE, U8_BIAS, U8_SCALE,  # noqa: F401
                              frame, from_bytes, ks_for, same)

FILTERS = ("nearest", "bilinear")
F32 = np.float32


def prefilter(rgba, k, crop=None):
    """P[3][ph][pw] (source channel order), float32: the block mean of the crop, anchored at the crop's origin."""
    h, w = rgba.shape[:2]
    cx, cy, cw, ch = crop if crop is not None else (0, 0, w, h)
    assert cw >= k and ch >= k and cx + cw <= w and cy + ch <= h
    pw, ph = cw // k, ch // k
    px = rgba[cy:cy + ph * k, cx:cx + pw * k, :3].astype(np.uint32)
    s = px.reshape(ph, k, pw, k, 3).sum(axis=(1, 3), dtype=np.uint32)
    p = s.astype(F32) * F32(1.0 / (k * k))
    return np.ascontiguousarray(p.transpose(2, 0, 1))


def ratio(n_in, n_out):
    return F32(float(n_in) / float(n_out))   # float(double(pw) / double(ow))


def axis_taps(n_out, n_in, filter):
    """(i0, i1, w0, w1) of every output coordinate of one axis; nearest: i1 = i0, w0 = 1, w1 = 0."""
    a = np.arange(n_out, dtype=np.uint32).astype(F32) + F32(0.5)
    b = a * ratio(n_in, n_out)
    assert b.dtype == F32
    if filter == "nearest":
        i = np.minimum(np.floor(b).astype(np.int64), n_in - 1)
        return i, i, np.ones(n_out, F32), np.zeros(n_out, F32)
    s = np.maximum(b - F32(0.5), F32(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = s - i0.astype(F32)
    w0 = F32(1.0) - w1
    assert w0.dtype == F32 and w1.dtype == F32
    return i0, i1, w0, w1


def resample(p, size, filter):
    """m[3][oh][ow] from P, float32, every operation rounded on its own."""
    ow, oh = size
    ph, pw = p.shape[1:]
    i0, i1, wx0, wx1 = axis_taps(ow, pw, filter)
    j0, j1, wy0, wy1 = axis_taps(oh, ph, filter)
    if filter == "nearest":
        return p[:, j0][:, :, i0]
    p00, p01 = p[:, j0][:, :, i0], p[:, j0][:, :, i1]
    p10, p11 = p[:, j1][:, :, i0], p[:, j1][:, :, i1]
    t0 = p00 * wx0
    t1 = p01 * wx1
    top = t0 + t1
    b0 = p10 * wx0
    b1 = p11 * wx1
    bot = b0 + b1
    mt = top * wy0[:, None]
    mb = bot * wy1[:, None]
    m = mt + mb
    assert m.dtype == F32
    return m


def store(v, dtype):
    """tensor_reference.expected's conversions (bf16 as uint16 bit patterns)."""
    assert v.dtype == F32
    if dtype == "f32":
        return v
    if dtype == "f16":
        return v.astype(np.float16)
    if dtype == "bf16":
        u = np.ascontiguousarray(v).view(np.uint32)
        return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.rint(v).clip(0, 255).astype(np.uint8)


def expected(rgba, size, k, dtype, scale, bias, order="rgb", filter="bilinear", crop=None):
    """[3, oh, ow] as the header defines it; size = (ow, oh), crop = (x, y, w, h) or None."""
    m = resample(prefilter(rgba, k, crop), size, filter)
    planes = []
    for c in range(3):
        v = m[c if order == "rgb" else 2 - c] * F32(scale[c])
        v = v + F32(bias[c])
        planes.append(v)
    return store(np.stack(planes), dtype)


def pre_extent(w, h, k, crop=None):
    cw, ch = (crop[2], crop[3]) if crop is not None else (w, h)
    return cw // k, ch // k


def params(dtype, identity=False):
    if identity:
        return tr.IDENTITY
    return (tr.U8_SCALE, tr.U8_BIAS) if dtype == "u8" else (tr.IMAGENET_SCALE, tr.IMAGENET_BIAS)
