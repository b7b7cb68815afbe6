"""The scaled decode where no device is needed (include/compeg_hip.h, "Scaled decode").

The expectation itself (tests/scaled_stream.py: the pinned f32 transform, one operation a line) is anchored to two things
that are not the code under test.  N = 4: the cosine formula of the header in f64 -- every sample within 1 of
trunc(clamp(f64)), the count of differing samples printed (the f32 factorisation is within 2e-4 of the f64 value in front
of the truncation, which can carry a sample across an integer, never further).  N = 2: the exact integer form
clamp((a +- b +- c +- d + 1028) >> 3, 0, 255) with an arithmetic shift -- the pass has no constants, so while the terms
stay below 2^20 every f32 step is exact and equality is required.  Then the orientation of the corner, DC-only frames
against the reduced decode's expectation, two mutants of the transform, compeg_scaled_shape against its restatement, and
the refusals that need no device.  (What needs a decoder or a batch needs a device: tests/test_gpu_scaled.py.)"""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import coef_stream as cs
import gray_stream as gs
import planes_stream as ps
import reduced_stream as rs
import scaled_stream as ss
from compeg_amd._lib import ScaledSpec, lib
from conftest import GOLDEN

FAMILIES = ("dc_cats", "dc_hostile", "q1_underflow", "dc_wrap", "dc_sweep", "saturated", "gamut", "random_dense", "texture", "basis")


def _dense():
    out = [f for f in cs.cases() if f.family == "random_dense"]
    assert out
    return out


def _coefficient_sets():
    """(name, int32 [data units, 64]) of random_dense frames and of the golden files: dequantised terms below 2^20."""
    sets = [(f.name, cs.predict(f)) for f in _dense()]
    for name, j, kw in ps.golden_files(ca, GOLDEN):
        sets.append((name, rs.file_coefficients(ca, j, **kw)[0]))
    for name, coef in sets:
        assert np.abs(coef.astype(np.int64)).max() < 1 << 20, name
    return sets


# ---- the anchors -----------------------------------------------------------------------------------------------------

def test_four_point_samples_are_within_one_of_the_cosine_formula():
    total = differing = 0
    worst = 0
    for name, coef in _coefficient_sets():
        got = ss.samples(coef, 4).astype(np.int64)
        want = np.trunc(np.clip(ss.cosine_f64(coef, 4), 0, 255)).astype(np.int64)
        d = np.abs(got - want)
        total, differing, worst = total + d.size, differing + int((d != 0).sum()), max(worst, int(d.max()))
        assert d.max() <= 1, f"{name}: a sample is {int(d.max())} from the formula's"
    print(f"N = 4: {differing} of {total} samples differ from trunc(clamp(f64 formula)), none by more than {worst}")
    assert total > 20000


def test_two_point_samples_are_the_exact_integer_form():
    total = 0
    for name, coef in _coefficient_sets():
        F = ss.corner(coef, 2).astype(np.int64)
        a, b, c, d = F[:, 0, 0], F[:, 0, 1], F[:, 1, 0], F[:, 1, 1]   # (b: horizontal frequency 1, c: vertical frequency 1)
        want = np.empty((F.shape[0], 2, 2), dtype=np.int64)
        for y, sy in ((0, 1), (1, -1)):
            for x, sx in ((0, 1), (1, -1)):
                want[:, y, x] = np.clip((a + sx * b + sy * c + sx * sy * d + 1028) >> 3, 0, 255)
        got = ss.samples(coef, 2)
        total += got.size
        assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} samples differ from the integer form"
    print(f"N = 2: {total} samples equal the integer form")
    assert total > 5000


@pytest.mark.parametrize("n", [2, 4])
def test_the_corner_is_not_transposed(n):
    """Only F[0][1] (horizontal frequency 1, zig-zag position 1): every row the same, the columns differ; only F[1][0]
    (zig-zag position 2): the reverse.  Exact."""
    coef = np.zeros((2, 64), dtype=np.int32)
    coef[0, 1] = 400    # natural index 1 = F[0][1]
    coef[1, 2] = 400    # natural index 8 = F[1][0]
    assert cs.ZIGZAG[1] == 1 and cs.ZIGZAG[8] == 2
    s = ss.samples(coef, n)
    h, v = s[0], s[1]
    assert (h == h[:1, :]).all() and len(set(h[0])) == n, h
    assert (v == v[:, :1]).all() and len(set(v[:, 0])) == n, v
    assert np.array_equal(h, v.T) and h[0, 0] > h[0, n - 1]


def _all_frames():
    colour = [f for f in cs.cases() if f.family in FAMILIES]
    assert {f.layout for f in colour} == {"422", "444", "440", "420"}
    gray = [f for f in gs.cases() if f.family in FAMILIES]
    assert gray
    return colour + gray


@pytest.mark.parametrize("den", [2, 4])
def test_dc_only_frames_repeat_the_reduced_pixel(den):
    """With every AC term zero each N x N block is the reduced decode's pixel, in every sampling: the DC term passes
    through sums with zero only."""
    n, seen = 8 // den, set()
    for f in _all_frames():
        comps, hs, vs = ps.sampling_of(f)
        z = rs.zero_ac(cs.predict(f))
        red = rs.reduced_planes(z, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
        got = ss.scaled_planes(z, den, f.dus_per_mcu, hs, vs, f.mcus_w, f.mcus_h)
        for g, r in zip(got, red):
            assert (g is None) == (r is None)
            if g is not None:
                assert np.array_equal(g, np.repeat(np.repeat(r, n, axis=0), n, axis=1)), f.name
        a, _ = ss.rgba(got, f.w, f.h, den, hs, vs)
        b, _ = rs.rgba(red, f.w, f.h, hs, vs)
        up = np.repeat(np.repeat(b, n, axis=0), n, axis=1)[:a.shape[0], :a.shape[1]]
        assert np.array_equal(a, up), f.name
        seen.add((comps, hs, vs))
    assert seen == {(3, 2, 1), (3, 1, 1), (3, 1, 2), (3, 2, 2), (1, 1, 1)}
    # (and the transform at N = 1 is the reduced sample itself)
    f = cs.dc_sweep()
    assert np.array_equal(ss.samples(cs.predict(f), 1)[:, 0, 0], rs.dc_sample(cs.predict(f)[:, 0]))


@pytest.mark.parametrize("mutant", ss.MUTANTS)
def test_mutants_of_the_transform_change_random_dense(mutant):
    changed = {}
    for den in (2, 4):
        if mutant == "swap_ab" and den == 4:
            continue   # (the 2-point pass has no constants to swap)
        for f in _dense():
            comps, hs, vs = ps.sampling_of(f)
            right = ss.destination(ss.frame_scaled(f, den), f.w, f.h, den, hs, vs)
            wrong = ss.destination(ss.frame_scaled(f, den, mutant=mutant), f.w, f.h, den, hs, vs)
            changed[den] = changed.get(den, 0) + int((right != wrong).sum())
    print(f"{mutant}: bytes of random_dense's expectation that change, by denominator: {changed}")
    assert changed and all(changed.values())


def test_the_expectation_is_not_the_block_mean_of_the_full_decode():
    f = cs.texture()
    comps, hs, vs = ps.sampling_of(f)
    full = cs.expectation(f).astype(np.float64)
    for den in (2, 4):
        got, _ = ss.rgba(ss.frame_scaled(f, den), f.w, f.h, den, hs, vs)
        mean = full.reshape(f.h // den, den, f.w // den, den, 4).mean(axis=(1, 3))
        differ = int((np.rint(mean)[..., :3] != got[..., :3]).sum())
        print(f"texture 1/{den}: {differ} of {got[..., :3].size} channel values differ from the rounded block mean")
        assert differ > 0


# ---- the shape call --------------------------------------------------------------------------------------------------

def _shape(spec, w, h):
    ow, oh, pt, total = C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd), C.c_uint64(0xdddddddddddddddd)
    rc = lib.compeg_scaled_shape(C.byref(spec) if spec is not None else None, w, h, C.byref(ow), C.byref(oh), C.byref(pt), C.byref(total))
    return rc, (ow.value, oh.value, pt.value, total.value)


def test_struct_size_and_names():
    assert C.sizeof(ScaledSpec) == 12
    assert ca.SCALED_FORMATS == {"rgba": 0, "rgb_planar": 1} and ss.FORMATS == tuple(ca.SCALED_FORMATS)
    assert ca.DECODE_KERNEL_NAMES[12] == "scaled" and ca.DECODE_KERNEL_NAMES[:12] == ca.ALL_KERNEL_NAMES and len(ca.DECODE_KERNEL_NAMES) == 13
    assert len(ca.ALL_KERNEL_NAMES) == 12 and len(ca.KERNEL_NAMES) == 10
    for name in ("ScaledSpec", "SCALED_FORMATS", "scaled_shape", "DECODE_KERNEL_NAMES"):
        assert name in ca.__all__ and hasattr(ca, name)
    assert hasattr(ca.Decoder, "decode_scaled") and hasattr(ca.Batch, "decode_scaled")


def test_shape_against_the_restatement():
    sizes = [(w, h) for w in range(1, 34) for h in range(1, 34)] + [(3840, 2160), (1920, 1080), (324, 70), (65535, 1), (1, 65535)]
    for den in ss.DENOMINATORS:
        for w, h in sizes:
            for format in ss.FORMATS:
                assert ca.scaled_shape(w, h, den, format) == ss.shape(w, h, den, format), (w, h, den, format)
            ow = -(-w // den)
            for pitch in (4 * ow, 4 * ow + 4, 4 * ow + 64):
                assert ca.scaled_shape(w, h, den, "rgba", pitch) == ss.shape(w, h, den, "rgba", pitch), (w, h, den, pitch)
    assert ca.scaled_shape(3840, 2160, 4) == (960, 540, 3840, 2073600) and ca.scaled_shape(3840, 2160, 2) == (1920, 1080, 7680, 8294400)
    assert ca.scaled_shape(324, 70, 4, "rgb_planar") == (81, 18, 81, 4374) and ca.scaled_shape(324, 70, 2, "rgb_planar") == (162, 35, 162, 17010)
    # (any output may be NULL)
    spec = ScaledSpec(4, 0, 0)
    assert lib.compeg_scaled_shape(C.byref(spec), 17, 9, None, None, None, None) == 0


def test_denominator_8_has_the_reduced_shape():
    for w, h in [(w, h) for w in range(1, 20) for h in (1, 7, 8, 9, 70)] + [(3840, 2160), (324, 70)]:
        for format in ss.FORMATS:
            assert ca.scaled_shape(w, h, 8, format) == ca.reduced_shape(w, h, format)
        pitch = 4 * -(-w // 8) + 12
        assert ca.scaled_shape(w, h, 8, "rgba", pitch) == ca.reduced_shape(w, h, "rgba", pitch)


def _refused(spec, w, h, *words):
    rc, out = _shape(spec, w, h)
    text = lib.compeg_last_error().decode()
    assert rc == ca.E_INVALID_ARG and all(x in text for x in words) and "COMPEG_" not in text, (rc, text)
    assert out == (0xdddddddd, 0xdddddddd, 0xdddddddd, 0xdddddddddddddddd), "an output was written on failure"


def test_refusals_that_need_no_device():
    _refused(None, 16, 16, "spec is NULL")
    for den in (0, 1, 3, 5, 6, 16, 0xffffffff):
        _refused(ScaledSpec(den, 0, 0), 16, 16, f"denominator {den}", "2, 4, 8", "built")
    for den in ss.DENOMINATORS:
        ow = -(-324 // den)
        _refused(ScaledSpec(den, 2, 0), 16, 16, "scaled spec", "format 2")
        _refused(ScaledSpec(den, 1, 8), 16, 16, "pitch 8", "planar")
        _refused(ScaledSpec(den, 0, 4 * ow - 4), 324, 70, f"pitch {4 * ow - 4}", str(4 * ow))   # (below 4 ow)
        _refused(ScaledSpec(den, 0, 4 * ow + 2), 324, 70, f"pitch {4 * ow + 2}", "multiple of 4")
        _refused(ScaledSpec(den, 0, 0), 0, 16, "no pixels")
        _refused(ScaledSpec(den, 0, 0), 16, 0, "no pixels")
    with pytest.raises(ca.Error, match="unknown scaled format"):
        ca.scaled_shape(16, 16, 4, "bgr")
    with pytest.raises(ca.Error, match="denominator 16"):
        ca.scaled_shape(16, 16, 16)
    # (the reduced spec's refusals are what they were)
    with pytest.raises(ca.Error, match="only one built"):
        ca.check(lib.compeg_reduced_shape(C.byref(ca._reduced_spec("rgba", None, denominator=4)), 16, 16, None, None, None, None))
