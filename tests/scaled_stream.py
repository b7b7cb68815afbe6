"""What a scaled decode (include/compeg_hip.h, "Scaled decode") must write, made on the host.  A plain module (Python and
numpy, no fixtures), shared by tests/test_scaled_stream.py (the expectation anchored to the cosine formula and to exact
integers), tests/test_scaled_emulation.py (the emulated lane body) and tests/test_gpu_scaled.py (the card).

The chain: the dequantised coefficients the reference keeps (cs.predict for frames written from coefficients;
rs.file_coefficients, the oracle's own entropy pass, for real encoders' files and for frames with an undecoded tail) -> the
N x N lowest-frequency corner of every data unit -> the pinned f32 transform, one operation a line -> N x N samples a data
unit -> planes at each component's own resolution, masks included -> ps.colour at the scaled extent -> the two formats laid
into the destination over whatever was there before.  compeg_scaled_shape is restated here and compared with the library
in the tests."""
import numpy as np

import coef_stream as cs
import planes_stream as ps
import reduced_stream as rs

FORMATS = ("rgba", "rgb_planar")
DENOMINATORS = (2, 4, 8)
A = np.float32(1.306562965)   # sqrt2 cos(pi / 8)
B = np.float32(0.541196100)   # sqrt2 cos(3 pi / 8)
MUTANTS = ("swap_ab", "bias_in_columns")


# ---- the shape, restated ---------------------------------------------------------------------------------------------

def shape(w, h, den, format="rgba", pitch=None):
    """-> (ow, oh, pitch, total bytes of one image): ow x oh = ceil(w / den) x ceil(h / den); rgba rows at `pitch` (None or
    0: tight, 4 ow), the last row at its full pitch; rgb_planar a tight [3, oh, ow] block whose pitch is ow."""
    assert den in DENOMINATORS
    ow, oh = -(-w // den), -(-h // den)
    if format == "rgb_planar":
        assert not pitch
        return ow, oh, ow, 3 * ow * oh
    pt = pitch or 4 * ow
    assert pt >= 4 * ow and pt % 4 == 0
    return ow, oh, pt, pt * oh


# ---- the pinned transform --------------------------------------------------------------------------------------------

def corner(coef, n):
    """int32 [data units, 64] dequantised coefficients (zig-zag order) -> int32 [data units, n, n]: F[v][u], v the vertical
    frequency, natural index v * 8 + u."""
    return np.asarray(coef)[:, cs.ZIGZAG].reshape(-1, 8, 8)[:, :n, :n].astype(np.int32)


def _pass(i, n, bias, swap):
    """One pass over i[0 .. n - 1] (float32 arrays): the header's statements, one operation a line."""
    in0 = i[0]
    if bias:
        in0 = in0 + np.float32(128.5)
    if n == 1:
        return [in0]
    if n == 2:
        return [in0 + i[1], in0 - i[1]]
    a, b = (B, A) if swap else (A, B)
    e0 = in0 + i[2]
    e1 = in0 - i[2]
    p = i[1] * a
    q = i[3] * b
    o0 = p + q
    p = i[1] * b
    q = i[3] * a
    o1 = p - q
    return [e0 + o0, e1 + o1, e1 - o1, e0 - o0]


def samples(coef, n, mutant=None):
    """int32 [data units, 64] -> uint8 [data units, n, n]: the scaled decode's samples.  mutant: "swap_ab" (the two
    constants exchanged) or "bias_in_columns" (128.5 added in the column pass, not the row pass)."""
    assert mutant in (None,) + MUTANTS
    f = corner(coef, n).astype(np.float32)
    f = f * np.float32(0.125)                      # (level * q is exact in f32: the product of the kernel's two steps)
    early = mutant == "bias_in_columns"
    cols = _pass([f[:, v, :] for v in range(n)], n, early, mutant == "swap_ab")     # over v; each [data units, u]
    ws = np.stack(cols, axis=1)                                                     # [data units, y, u]
    rows = _pass([ws[:, :, u] for u in range(n)], n, not early, mutant == "swap_ab")
    px = np.stack(rows, axis=2)                                                     # [data units, y, x]
    px = np.minimum(np.maximum(px, np.float32(0)), np.float32(255))
    return np.trunc(px).astype(np.uint8)


def cosine_f64(coef, n):
    """The formula itself in f64, before clamp and truncation: float64 [data units, n, n]."""
    F = corner(coef, n).astype(np.float64)
    k = np.arange(n)
    c = np.where(k == 0, 1 / np.sqrt(2), 1.0)
    basis = c[None, :] * np.cos((2 * k[:, None] + 1) * k[None, :] * np.pi / (2 * n))   # [x, u]
    return 0.25 * np.einsum("yv,nvu,xu->nyx", basis, F, basis) + 128.5


# ---- samples into planes ---------------------------------------------------------------------------------------------

def whole_planes(smp, n, dpm, hs, vs, mcus_w, mcus_h):
    """uint8 samples [data units, n, n] of the decoded MCUs -> (Y, Cb, Cr, mask): whole-MCU planes at each component's own
    scaled resolution and the bool mask (luma resolution) of the samples a decoded MCU covers.  dpm = 1: luma only."""
    mcus = smp.shape[0] // dpm
    smp = smp[:mcus * dpm].reshape(mcus, dpm, n, n)
    y = np.zeros((mcus_h * n * vs, mcus_w * n * hs), dtype=np.uint8)
    mask = np.zeros(y.shape, dtype=bool)
    cb = cr = None
    if dpm > 1:
        cb, cr = np.zeros((mcus_h * n, mcus_w * n), dtype=np.uint8), np.zeros((mcus_h * n, mcus_w * n), dtype=np.uint8)
    for m in range(mcus):
        r, c = divmod(m, mcus_w)
        if r >= mcus_h:
            break
        sl = (slice(r * n * vs, (r + 1) * n * vs), slice(c * n * hs, (c + 1) * n * hs))
        y[sl] = np.block([[smp[m, v * hs + h] for h in range(hs)] for v in range(vs)])
        mask[sl] = True
        if dpm > 1:
            sc = (slice(r * n, r * n + n), slice(c * n, c * n + n))
            cb[sc], cr[sc] = smp[m, dpm - 2], smp[m, dpm - 1]
    return y, cb, cr, mask


def scaled_planes(coef, den, dpm, hs, vs, mcus_w, mcus_h, mutant=None):
    n = 8 // den
    return whole_planes(samples(coef, n, mutant), n, dpm, hs, vs, mcus_w, mcus_h)


def frame_coefficients(f, ca=None):
    """A coefficient frame's dequantised coefficients; a frame with MCUs behind its last complete interval takes them
    from the oracle's entropy pass, as rs.frame_reduced does (ca: the package)."""
    if f.family == "sized" and "/short" in f.name:
        return rs.file_coefficients(ca, f.jpeg(), **f.image_kw())[0]
    return cs.predict(f)


def frame_scaled(f, den, mutant=None, ca=None):
    comps, hs, vs = ps.sampling_of(f)
    return scaled_planes(frame_coefficients(f, ca), den, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h, mutant)


def file_scaled(ca, jpeg, den, **kw):
    """-> (scaled planes, (w, h, comps, hs, vs))."""
    coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), _ = rs.file_coefficients(ca, jpeg, **kw)
    return scaled_planes(coef, den, dpm, hs, vs, mcus_w, mcus_h), (w, h, comps, hs, vs)


def rgba(planes, w, h, den, hs, vs):
    """Scaled planes -> (RGBA [oh, ow, 4] with undecoded pixels zero, mask [oh, ow]): chroma nearest neighbour, the
    integer colour step, A = 255."""
    y, cb, cr, mask = planes
    ow, oh = -(-w // den), -(-h // den)
    return ps.colour(y, cb, cr, hs, vs, ow, oh, mask), mask[:oh, :ow]


# ---- the destination -------------------------------------------------------------------------------------------------

def destination(planes, w, h, den, hs, vs, format="rgba", pitch=None, before=None):
    """The destination's bytes after the decode: uint8 [total] -- `before` (that many bytes; default zeros) with the bytes
    of every pixel a decoded MCU covers inside ow x oh replaced."""
    ow, oh, pt, total = shape(w, h, den, format, pitch)
    px, mask = rgba(planes, w, h, den, hs, vs)
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


def view(buf, w, h, den, format="rgba", pitch=None):
    """A destination's pixels: RGBA [oh, ow, 4] (A = 255 for the planar format) cut out of `buf` (uint8 [total])."""
    ow, oh, pt, total = shape(w, h, den, format, pitch)
    if format == "rgba":
        return np.stack([buf[r * pt: r * pt + 4 * ow].reshape(ow, 4) for r in range(oh)])
    rgb = buf[:3 * ow * oh].reshape(3, oh, ow).transpose(1, 2, 0)
    return np.concatenate([rgb, np.full((oh, ow, 1), 255, dtype=np.uint8)], axis=2)
