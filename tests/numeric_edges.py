"""Frames, (scale, bias) sets and reference mutants that take the tensor output's arithmetic and conversions
(compeg_amd/csrc/tensor_body.h, resize_body.h) to their edges: ties, subnormals, overflow, infinities, the clamp and
denormal float32.  Shared by tests/test_numeric_edges.py, both emulation tests and both GPU workers.

The conversions have a software form (what g++ builds for the emulation) and a device form (v_cvt_f16_f32, v_rndne_f32
+ v_med3_f32, the device pass's contraction and denormal mode); the ordinary cases feed them pixels through the
ImageNet scale and bias, about -2.2 .. 2.7, where none of the two forms' branches or modes can differ.  The sets here
reach them.  The mutants are the reference with one rule changed -- what a wrong mode or branch would compute --
and tests/test_numeric_edges.py shows that each of them changes the expectation of a case below in many elements, so
a device that had the mutant's behaviour would fail that case.

NaN cannot arise and there is no NaN case: every scale and bias is finite (the API refuses others), every block mean
is >= 0, a finite product plus a finite bias is finite or an infinity, and an infinity plus a finite number is that
infinity; 0 * 3e38 is 0.  The resize's weights lie in 0..1 and its taps are >= 0, so the same holds there."""
import functools

import numpy as np

import resize_reference as rr
import tensor_reference as tr
from oracle import oracle as orc
from tools import synth

F32 = np.float32
RAMP_W, RAMP_H = 256, 128
NOISY = (330, 70)


def _f(x):
    """x rounded to float32 once, as a Python float: what the API, struct.pack and numpy all then agree on."""
    return float(F32(x))


# ---------------------------------------------------------------------------------------------------------- frames

def _ramp_rgb():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)            # tile v: row v // 16, column v % 16
    gray = np.repeat(np.repeat(v, 8, axis=0), 16, axis=1)         # flat tiles of 16 x 8 pixels: one 4:2:2 MCU each
    assert gray.shape == (RAMP_H, RAMP_W)
    return np.ascontiguousarray(np.stack([gray] * 3, axis=-1))


def _encoded_flat_gray(rgb, quality=100):
    """(jpeg, the oracle's RGBA) of a frame of flat gray MCUs, which the oracle must give back exactly."""
    jpeg = synth.encode(rgb, quality=quality, ri=4)
    rgba = orc.ImageData(jpeg).decode()
    assert rgba.shape == rgb.shape[:2] + (4,)
    # a condition of the cases built on it, not a hope: every level 0..255 arrives, in every channel, as it was put in
    assert np.array_equal(rgba[..., :3], rgb), f"the oracle does not decode the gray ramp exactly at q={quality}"
    for c in range(3):
        assert np.unique(rgba[..., c]).size == 256
    rgba.setflags(write=False)
    return jpeg, rgba


@functools.lru_cache(maxsize=None)
def ramp(quality=100):
    """256 x 128: 256 flat 16 x 8 tiles, tile v of gray level v."""
    return _encoded_flat_gray(_ramp_rgb(), quality)


@functools.lru_cache(maxsize=None)
def ramp_flipped():
    """The ramp mirrored left to right (the second image of the batch case)."""
    return _encoded_flat_gray(np.ascontiguousarray(_ramp_rgb()[:, ::-1]))


@functools.lru_cache(maxsize=None)
def noisy():
    """tensor_reference.frame(330, 70): its block sums take every residue mod k^2 at k = 2 and k = 8, so every
    fraction a block mean can have is present."""
    jpeg, rgba = tr.frame(*NOISY)
    for k in (2, 8):
        h, w = rgba.shape[0] // k * k, rgba.shape[1] // k * k
        s = rgba[:h, :w, :3].astype(np.uint32).reshape(h // k, k, w // k, k, 3).sum(axis=(1, 3))
        assert np.unique(s % (k * k)).size == k * k, f"block sums at k={k} miss a residue mod {k * k}"
    return jpeg, rgba


FRAMES = {"ramp": ramp, "ramp_flipped": ramp_flipped, "noisy": noisy}
EXTENT = {"ramp": (RAMP_W, RAMP_H), "ramp_flipped": (RAMP_W, RAMP_H), "noisy": NOISY}   # (w, h), without making the frame
# (frame, k) of every pack_tensor case
PACKS = (("ramp", 1), ("noisy", 2), ("noisy", 8))


# ------------------------------------------------------------------------------------------------------ edge sets
# name -> (element types, scale[3], bias[3]); all finite, so the API accepts them
SETS = {
    # ulp 2 and 4: every other value an exact tie, both signs
    "f16_ties": (("f16",), (1.0, 1.0, 1.0), (2048.0, 4096.0, -2048.0)),
    # 65519 -> 65504; 65520 (a tie) -> +inf; -65520 -> -inf
    "f16_overflow": (("f16",), (256.0, 256.0, -256.0), (239.0, 240.0, -240.0)),
    # below 2^-25 -> 0, ties at odd multiples of 2^-25, crossing 2^-14 at m = 128
    "f16_subnormal": (("f16",), (2.0 ** -26, 2.0 ** -21, -2.0 ** -26), (0.0, 0.0, 0.0)),
    # float32 +-inf and huge finite values -> +-inf
    "f16_inf": (("f16",), (_f(3e38), _f(-3e38), _f(1e36)), (0.0, 0.0, 0.0)),
    "bf16_ties": (("bf16",), (1.0, 1.0, 1.0), (256.0, 512.0, -256.0)),
    # finite float32 that rounds up to the bf16 infinity; float32 infinities
    "bf16_overflow": (("bf16",), (_f(3.4e38 / 255), _f(3e38), _f(-3e38)), (0.0, 0.0, 0.0)),
    # a denormal scale (an input), a denormal product of normal inputs (k >= 2: means below 1), a denormal difference
    # of normals, negative denormals
    "f32_denormal": (("f32", "bf16"), (2.0 ** -140, 1.5 * 2.0 ** -126, 2.0 ** -126), (0.0, 0.0, -0.75 * 2.0 ** -126)),
    "f32_inf": (("f32",), (_f(3e38), _f(-3e38), 1.0), (0.0, 0.0, 0.0)),
    # x.5 everywhere: half to even
    "u8_ties": (("u8",), (0.5, 1.0, 1.5), (0.0, 0.5, -0.5)),
    # below 0, above 255, +inf -> 255, 0 * 3e38 = 0
    "u8_clamp": (("u8",), (2.0, -1.0, _f(3e38)), (-128.0, 100.0, 0.0)),
    # -inf -> 0, -0.5 -> 0, just over a tie
    "u8_clamp2": (("u8",), (_f(-3e38), 1.0, 1.0), (0.0, _f(0.5001), -255.5)),
    # the contraction probe: only as float32 does a fused m * scale + bias show
    "imagenet_f32": (("f32",), tr.IMAGENET_SCALE, tr.IMAGENET_BIAS),
}
for _name, (_dtypes, _scale, _bias) in SETS.items():
    assert all(np.isfinite(F32(x)) and float(F32(x)) == x for x in _scale + _bias), _name

# (set, element type), in a fixed order
SET_DTYPES = tuple((name, dtype) for name, (dtypes, _, _) in SETS.items() for dtype in dtypes)


def denormals_kept():
    """numpy keeps float32 denormals here (the guard of the f32_denormal expectation)."""
    return F32(2.0 ** -140) * F32(3) != 0


def expected(rgba, k, name, dtype, order="rgb"):
    """tensor_reference.expected of a set (overflow to infinity is what these sets are for)."""
    _, scale, bias = SETS[name]
    with np.errstate(over="ignore"):
        return tr.expected(rgba, k, dtype, scale, bias, order)


def expected_resized(rgba, size, k, name, dtype, order="rgb", filter="bilinear", crop=None):
    _, scale, bias = SETS[name]
    with np.errstate(over="ignore"):
        return rr.expected(rgba, size, k, dtype, scale, bias, order, filter, crop)


# -------------------------------------------------------------------------------------------------------- mutants
# The reference with one rule changed.  pack(..., mutant=None) is tensor_reference.expected itself and
# resized(..., mutant=None) resize_reference.expected (test_numeric_edges.py holds them to that).

def _ftz(x):
    x = np.asarray(x, dtype=F32)
    return np.where(np.abs(x) < F32(2.0 ** -126), F32(0), x).astype(F32)


def _scale_bias(m, scale, bias, mutant):
    scale, bias = F32(scale), F32(bias)
    if mutant == "fused_scale_bias":   # one rounding: an FMA (exact in float64 up to its own, far finer, rounding)
        return (m.astype(np.float64) * np.float64(scale) + np.float64(bias)).astype(F32)
    if mutant == "f32_flush":          # denormal inputs and results are zero
        return _ftz(_ftz(_ftz(m) * _ftz(scale)) + _ftz(bias))
    v = m * scale
    return v + bias


def _f16_toward_zero(v):
    h = v.astype(np.float16)
    finite = np.isfinite(v)
    over = finite & (np.abs(h.astype(np.float64)) > np.abs(v.astype(np.float64)))   # rounded away from zero (inf included)
    return np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)


def _f16(v, mutant):
    h = v.astype(np.float16)
    if mutant == "f16_truncate":
        return _f16_toward_zero(v)
    if mutant == "f16_half_away":
        lo = _f16_toward_zero(v)                                   # the neighbour towards zero
        lo64, a = np.abs(lo.astype(np.float64)), np.abs(v.astype(np.float64))
        ulp = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(lo64, 2.0 ** -14))) - 10), 2.0 ** -24)
        with np.errstate(invalid="ignore"):                        # (inf - inf where v is an infinity: no tie)
            tie = np.isfinite(v) & (a - lo64 == ulp / 2)
        away = np.nextafter(lo, np.where(np.signbit(v), np.float16(-np.inf), np.float16(np.inf)).astype(np.float16))
        return np.where(tie, away, h).astype(np.float16)
    if mutant == "f16_flush_subnormals":
        return np.where(np.abs(h) < np.float16(2.0 ** -14), np.float16(0), h).astype(np.float16)
    if mutant == "f16_saturate":
        return np.where(np.isinf(h) & np.isfinite(v), np.copysign(np.float16(65504), h), h).astype(np.float16)
    return h


def _u8(v, mutant):
    if mutant == "u8_half_away":
        r = np.copysign(np.floor(np.abs(v) + F32(0.5)), v)
    elif mutant == "u8_truncate":
        r = np.trunc(v)
    else:
        r = np.rint(v)
    if mutant == "u8_wrap":   # the low byte of the integer instead of the clamp
        return (np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64) & 255).astype(np.uint8)
    return r.clip(0, 255).astype(np.uint8)


def _store(v, dtype, mutant):
    assert v.dtype == F32
    if dtype == "f32":
        return _ftz(v) if mutant == "f32_flush" else v
    if dtype == "f16":
        return _f16(v, mutant)
    if dtype == "bf16":
        u = np.ascontiguousarray(v).view(np.uint32)
        if mutant == "bf16_truncate":
            return (u >> np.uint32(16)).astype(np.uint16)
        return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return _u8(v, mutant)


PACK_MUTANTS = ("fused_scale_bias", "f32_flush", "f16_truncate", "f16_half_away", "f16_flush_subnormals", "f16_saturate",
                "bf16_truncate", "u8_half_away", "u8_truncate", "u8_wrap")
RESIZE_MUTANTS = ("fused_taps", "fused_lerp")


def pack(rgba, k, name, dtype, order="rgb", mutant=None):
    """tensor_reference.expected of a set, with one rule changed if mutant names one."""
    assert mutant is None or mutant in PACK_MUTANTS
    _, scale, bias = SETS[name]
    m = rr.prefilter(rgba, k)
    with np.errstate(over="ignore"):
        v = np.stack([_scale_bias(m[c if order == "rgb" else 2 - c], scale[c], bias[c], mutant) for c in range(3)])
        return _store(v, dtype, mutant)


def _taps(n_out, n_in, mutant):
    a = np.arange(n_out, dtype=np.uint32).astype(F32) + F32(0.5)
    if mutant == "fused_taps":   # b - 0.5 with b = a * ratio unrounded
        d = (a.astype(np.float64) * np.float64(rr.ratio(n_in, n_out)) - 0.5).astype(F32)
    else:
        d = a * rr.ratio(n_in, n_out) - F32(0.5)
    s = np.maximum(d, F32(0))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = s - i0.astype(F32)
    return i0, i1, F32(1.0) - w1, w1


def _lerp(p0, w0, p1, w1, mutant):
    t1 = p1 * w1
    if mutant == "fused_lerp":   # the first product unrounded into the addition
        return (p0.astype(np.float64) * w0.astype(np.float64) + t1.astype(np.float64)).astype(F32)
    t0 = p0 * w0
    return t0 + t1


def resized(rgba, size, k, name, dtype, order="rgb", crop=None, mutant=None):
    """resize_reference.expected (bilinear) of a set, with one rule changed if mutant names one."""
    assert mutant is None or mutant in RESIZE_MUTANTS
    _, scale, bias = SETS[name]
    p = rr.prefilter(rgba, k, crop)
    ow, oh = size
    i0, i1, wx0, wx1 = _taps(ow, p.shape[2], mutant)
    j0, j1, wy0, wy1 = _taps(oh, p.shape[1], mutant)
    top = _lerp(p[:, j0][:, :, i0], wx0, p[:, j0][:, :, i1], wx1, mutant)
    bot = _lerp(p[:, j1][:, :, i0], wx0, p[:, j1][:, :, i1], wx1, mutant)
    m = _lerp(top, wy0[:, None], bot, wy1[:, None], mutant)
    with np.errstate(over="ignore"):
        v = np.stack([_scale_bias(m[c if order == "rgb" else 2 - c], scale[c], bias[c], None) for c in range(3)])
        return _store(v, dtype, None)


# the bilinear cases of the resize: (frame, k, size, crop)
RESIZE_EDGE = ("ramp", 1, (257, 129), (15, 3, 226, 120))   # taps straddle tiles; every set
# imagenet_f32.  On its flat tiles the ramp at 257 x 129 shows a fused tap (519 elements) but hardly a fused lerp (4: both
# taps of most elements are one level, and their weights sum to 1 exactly), so the ramp goes to 299 x 299 as well
RESIZE_CONTRACTION = (("noisy", 1, (224, 224), None), ("ramp", 2, (224, 224), None), ("ramp", 1, (257, 129), None),
                      ("ramp", 1, (299, 299), None))


def changed(a, b, dtype):
    """Elements in which two expectations differ as tensor_reference.same compares them (values: +0 is -0)."""
    if dtype == "bf16":
        a = (a.astype(np.uint32) << np.uint32(16)).view(F32)
        b = (b.astype(np.uint32) << np.uint32(16)).view(F32)
    return int((a != b).sum())
