"""The reduced decode where no device is needed (include/compeg_hip.h, "Reduced-size decode").

The expectation itself (tests/reduced_stream.py) is pinned to the oracle's own passes: for frames of every sampling,
grayscale through its 4:4:4 twin, and for the golden files the front end accepts, the post-entropy coefficients with
their AC terms set to zero go through orc_dct_pass and orc_finalize_pass, and pixel (8x, 8y) of that is the expectation,
byte for byte.  Every data unit of those decodes is flat -- which is what makes the one-sample formula the transform's.
Two mutants of the formula change dc_sweep's expectation; the expectation is not the 8 x 8 mean of the full decode; then
compeg_reduced_shape against its restatement and the refusals that need no device.  (What needs a decoder or a batch needs
a device: tests/test_gpu_reduced.py.)"""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import coef_stream as cs
import gray_stream as gs
import planes_stream as ps
import reduced_stream as rs
from compeg_amd._lib import ReducedSpec, lib
from conftest import GOLDEN
from oracle import oracle as orc

FAMILIES = ("dc_cats", "dc_hostile", "q1_underflow", "dc_wrap", "dc_sweep", "saturated", "gamut", "random_dense", "texture")


def _oracle_reduced(md, coef, w, h):
    """The oracle's transform and colour step over `coef` with its AC terms zeroed.  -> (pixel (8x, 8y) of the RGBA
    [oh, ow, 4], whether every data unit came out flat)."""
    z = np.ascontiguousarray(rs.zero_ac(coef)[:, :32].astype(np.int32)).ravel()
    block = np.frombuffer(md, dtype=np.uint8).copy()
    orc.lib().orc_dct_pass(block.ctypes.data, z.ctypes.data, z.size)
    smp = np.ascontiguousarray(z.reshape(-1, 32)[:, :16]).view(np.uint8).reshape(-1, 64)
    flat = bool((smp == smp[:, :1]).all())
    out = np.zeros((h, w, 4), dtype=np.uint8)
    orc.lib().orc_finalize_pass(block.ctypes.data, z.ctypes.data, z.size, out.ctypes.data, w, h)
    return out[::8, ::8], flat


def _frames():
    colour = [f for f in cs.cases() if f.family in FAMILIES]
    assert {f.layout for f in colour} == {"422", "444", "440", "420"} and {f.standard for f in colour} == {False, True}
    return colour


@pytest.mark.parametrize("name", [f.name for f in _frames()])
def test_expectation_is_the_oracles_decode_of_the_zeroed_ac_frame(name):
    f = cs.case(name)
    comps, hs, vs = ps.sampling_of(f)
    got, _ = rs.rgba(rs.frame_reduced(f), f.w, f.h, hs, vs)
    want, flat = _oracle_reduced(orc.ImageData(f.jpeg(), **f.image_kw()).metadata(), cs.predict(f), f.w, f.h)
    assert flat, f"{name}: a data unit without AC terms did not come out flat"
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"


def _twin_serves(f):
    """Neither the frame's reader nor its twin's runs dry (quirk Q1): where one does their bit positions differ and the
    twin's chroma is not flat -- tests/test_gray_stream.py makes the same cut."""
    a, b = {}, {}
    cs.predict(f, facts=a)
    cs.predict(gs.twin(f), facts=b)
    return not a["dry"] and not b["dry"]


GRAY = [f.name for f in gs.cases() if f.family in FAMILIES and _twin_serves(f)]


def test_enough_grayscale_cases_meet_their_twin():
    assert len(GRAY) >= 8 and {gs.case(n).family for n in GRAY} >= {"dc_cats", "dc_sweep", "gamut", "saturated", "dc_wrap"}, GRAY


@pytest.mark.parametrize("name", GRAY)
def test_grayscale_expectation_is_the_oracles_decode_of_the_twin(name):
    f = gs.case(name)
    got, _ = rs.rgba(rs.frame_reduced(f), f.w, f.h, 1, 1)
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])
    t = gs.twin(f)
    want, flat = _oracle_reduced(orc.ImageData(t.jpeg(), **t.image_kw()).metadata(), cs.predict(t), t.w, t.h)
    assert flat and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"


def test_expectation_of_the_golden_files_is_the_oracles_decode_of_the_zeroed_ac_file():
    files = ps.golden_files(ca, GOLDEN)
    samplings = set()
    for name, j, kw in files:
        coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), md = rs.file_coefficients(ca, j, **kw)
        samplings.add((comps, hs, vs))
        got, mask = rs.rgba(rs.reduced_planes(coef, dpm, hs, vs, mcus_w, mcus_h), w, h, hs, vs)
        assert got.shape == (-(-h // 8), -(-w // 8), 4)
        if comps == 1:
            continue   # (the oracle's colour step takes three components; the card's own RGBA is compared in tests/test_gpu_reduced.py)
        want, flat = _oracle_reduced(md, coef, w, h)
        assert flat and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"
    assert {(3, 2, 1), (3, 1, 1)} <= samplings, samplings


def test_sized_frames_with_cut_mcus_and_an_undecoded_tail():
    """The frames the card's tests are made of: 324 x 70 in every sampling, and a frame whose last MCUs no interval covers."""
    for layout, ri in (("422", 21), ("444", 41), ("440", 5), ("420", 3)):
        f = ps.sized(layout, 324, 70, ri, seed=3)
        comps, hs, vs = ps.sampling_of(f)
        got, mask = rs.rgba(rs.frame_reduced(f), f.w, f.h, hs, vs)
        want, flat = _oracle_reduced(orc.ImageData(f.jpeg(), **f.image_kw()).metadata(), cs.predict(f), f.w, f.h)
        assert got.shape == (9, 41, 4) and mask.all() and flat and np.array_equal(got, want), f.name
    f = ps.sized("422", 48, 23, 4, seed=2, short=3)
    coef, (w, h, comps, hs, vs, dpm, mcus_w, mcus_h), md = rs.file_coefficients(ca, f.jpeg(), **f.image_kw())
    got, mask = rs.rgba(rs.frame_reduced(f, ca=ca), w, h, hs, vs)
    want, flat = _oracle_reduced(md, coef, w, h)
    assert not mask.all() and (got[~mask] == 0).all() and flat and np.array_equal(got, want)


def test_the_formula_is_the_chains_sample():
    """dc_sample, the header's formula, gives what cs.samples gives for a data unit with its DC term alone."""
    for f in (cs.dc_sweep(), cs.dc_wrap(), cs.saturated(), cs.texture("420")):
        dc = rs.zero_ac(cs.predict(f))
        assert np.array_equal(rs.dc_sample(dc[:, 0]), cs.samples(dc)[:, 0, 0]), f.name


@pytest.mark.parametrize("mutant", ["rint", "bias128"])
def test_mutants_of_the_formula_change_dc_sweep(mutant):
    f = cs.dc_sweep()
    comps, hs, vs = ps.sampling_of(f)
    right = rs.destination(rs.frame_reduced(f), f.w, f.h, hs, vs)
    same = rs.destination(rs.frame_reduced(f, mutant="none"), f.w, f.h, hs, vs)   # (dc_sample itself, no mutation)
    wrong = rs.destination(rs.frame_reduced(f, mutant=mutant), f.w, f.h, hs, vs)
    changed = int((right != wrong).sum())
    print(f"{mutant}: {changed} of {right.size} bytes of dc_sweep's expectation change")
    assert np.array_equal(right, same) and changed > 0


def test_the_expectation_is_not_the_block_mean_of_the_full_decode():
    """Documents that 1/8 from the DC terms and the 8 x 8 mean of the full decode are different things: the transform
    truncates per sample and the colour step clamps per pixel."""
    f = cs.texture()
    comps, hs, vs = ps.sampling_of(f)
    got, _ = rs.rgba(rs.frame_reduced(f), f.w, f.h, hs, vs)
    full = orc.ImageData(f.jpeg(), **f.image_kw()).decode().astype(np.float64)
    mean = full.reshape(f.h // 8, 8, f.w // 8, 8, 4).mean(axis=(1, 3))
    differ = int((np.rint(mean)[..., :3] != got[..., :3]).sum())
    print(f"texture: {differ} of {got[..., :3].size} channel values differ from the rounded block mean")
    assert differ > 0


# ---- the shape call --------------------------------------------------------------------------------------------------

def _shape(spec, w, h):
    ow, oh, pt, total = C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd), C.c_uint64(0xdddddddddddddddd)
    rc = lib.compeg_reduced_shape(C.byref(spec) if spec is not None else None, w, h, C.byref(ow), C.byref(oh), C.byref(pt), C.byref(total))
    return rc, (ow.value, oh.value, pt.value, total.value)


def test_struct_size_and_names():
    assert C.sizeof(ReducedSpec) == 12
    assert ca.REDUCED_FORMATS == {"rgba": 0, "rgb_planar": 1} and rs.FORMATS == tuple(ca.REDUCED_FORMATS)
    assert ca.ALL_KERNEL_NAMES[10] == "reduced" and ca.ALL_KERNEL_NAMES[:10] == ca.KERNEL_NAMES
    for name in ("ReducedSpec", "REDUCED_FORMATS", "reduced_shape"):
        assert name in ca.__all__ and hasattr(ca, name)


def test_shape_against_the_restatement():
    sizes = [(w, h) for w in range(1, 41) for h in range(1, 41)] + [(3840, 2160), (65535, 1), (1, 65535)]
    for w, h in sizes:
        for format in rs.FORMATS:
            assert ca.reduced_shape(w, h, format) == rs.shape(w, h, format), (w, h, format)
        ow = -(-w // 8)
        for pitch in (4 * ow, 4 * ow + 4, 4 * ow + 64):
            assert ca.reduced_shape(w, h, "rgba", pitch) == rs.shape(w, h, "rgba", pitch), (w, h, pitch)
    assert ca.reduced_shape(3840, 2160) == (480, 270, 1920, 518400) and ca.reduced_shape(324, 70, "rgb_planar") == (41, 9, 41, 1107)
    # (any output may be NULL)
    spec = ReducedSpec(8, 0, 0)
    assert lib.compeg_reduced_shape(C.byref(spec), 17, 9, None, None, None, None) == 0


def _refused(spec, w, h, *words):
    rc, out = _shape(spec, w, h)
    text = lib.compeg_last_error().decode()
    assert rc == ca.E_INVALID_ARG and all(x in text for x in words) and "COMPEG_" not in text, (rc, text)
    assert out == (0xdddddddd, 0xdddddddd, 0xdddddddd, 0xdddddddddddddddd), "an output was written on failure"


def test_refusals_that_need_no_device():
    _refused(None, 16, 16, "spec is NULL")
    for den in (0, 1, 2, 4, 16):
        _refused(ReducedSpec(den, 0, 0), 16, 16, f"denominator {den}", "1/8", "DC-only", "only one built")
    _refused(ReducedSpec(8, 2, 0), 16, 16, "format 2")
    _refused(ReducedSpec(8, 1, 8), 16, 16, "pitch 8", "planar")
    _refused(ReducedSpec(8, 0, 160), 324, 70, "pitch 160", "164")   # (below 4 ow)
    _refused(ReducedSpec(8, 0, 166), 324, 70, "pitch 166", "multiple of 4")
    _refused(ReducedSpec(8, 0, 0), 0, 16, "no pixels")
    _refused(ReducedSpec(8, 0, 0), 16, 0, "no pixels")
    with pytest.raises(ca.Error, match="unknown reduced format"):
        ca.reduced_shape(16, 16, "bgr")
    with pytest.raises(ca.Error, match="denominator 4"):
        ca.check(lib.compeg_reduced_shape(C.byref(ca._reduced_spec("rgba", None, denominator=4)), 16, 16, None, None, None, None))
