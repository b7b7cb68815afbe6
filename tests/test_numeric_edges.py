"""That the numeric-edge cases (tests/numeric_edges.py) can fail: on the CPU, every mutant of the reference -- a
flushed denormal, a truncated or saturated f16, a wrapped u8, a contracted multiply-add ... -- changes the expectation
of at least one case the GPU workers run, in at least 64 elements.  And that the reference itself is right at these
edges: numpy's conversions against torch's on the CPU and against integer arithmetic."""
import numpy as np
import pytest
import torch

import gpu_resize_worker
import gpu_tensor_worker
import numeric_edges as ne
import resize_reference as rr
import tensor_reference as tr

BAR = 64   # elements a mutant has to change in some case


def test_frames_cover_what_the_cases_rest_on():
    """(asserted inside the module as the frames are made: all 256 levels exact, every residue of the block sums)"""
    for q in (100, 95, 85):
        rgba = ne.ramp(q)[1]
        assert rgba.shape == (ne.RAMP_H, ne.RAMP_W, 4)
        assert np.array_equal(rgba[::8, ::16, 0].ravel(), np.arange(256))
    assert np.array_equal(ne.ramp_flipped()[1], ne.ramp()[1][:, ::-1])
    assert ne.noisy()[1].shape == (70, 330, 4)


def test_the_gpu_workers_run_every_set():
    for worker in (gpu_tensor_worker, gpu_resize_worker):
        assert worker.EDGE_SETS == tuple(ne.SETS)
        assert all(f"numeric_edges[{name}]" in worker.CASES for name in ne.SETS)
    assert "numeric_edges_batch" in gpu_tensor_worker.CASES


def test_numpy_keeps_float32_denormals():
    assert ne.denormals_kept()
    want = ne.expected(ne.ramp()[1], 1, "f32_denormal", "f32")
    tiny = (want != 0) & (np.abs(want) < np.float32(2.0 ** -126))
    # plane 0: all but level 0; plane 2: the tiles of levels 0 (negative) and 1.  (Plane 1's product is denormal only
    # where a block mean lies below 2 / 3, which a frame may not have.)
    assert tiny[0].sum() == 255 * 128 and tiny[2].sum() == 256 and (want[2] < 0).sum() == 128


@pytest.mark.parametrize("name,dtype", ne.SET_DTYPES)
def test_unmutated_variants_are_the_references(name, dtype):
    for frame, k in ne.PACKS:
        rgba = ne.FRAMES[frame]()[1]
        for order in ("rgb", "bgr"):
            assert np.array_equal(ne.pack(rgba, k, name, dtype, order), ne.expected(rgba, k, name, dtype, order), equal_nan=True)
    frame, k, size, crop = ne.RESIZE_EDGE
    rgba = ne.FRAMES[frame]()[1]
    assert np.array_equal(ne.resized(rgba, size, k, name, dtype, "bgr", crop),
                          ne.expected_resized(rgba, size, k, name, dtype, "bgr", "bilinear", crop), equal_nan=True)


def test_no_case_holds_a_nan():
    for name, dtype in ne.SET_DTYPES:
        if dtype in ("f32", "f16"):
            for frame, k in ne.PACKS:
                assert not np.isnan(ne.expected(ne.FRAMES[frame]()[1], k, name, dtype)).any(), name


def _pack_changes(mutant):
    """(elements changed, set, dtype) of the k = 1 ramp's packs, the most first."""
    rgba = ne.ramp()[1]
    found = [(ne.changed(ne.pack(rgba, 1, name, dtype, mutant=mutant), ne.expected(rgba, 1, name, dtype), dtype), name, dtype)
             for name, dtype in ne.SET_DTYPES]
    return sorted(found, reverse=True)


@pytest.mark.parametrize("mutant", ne.PACK_MUTANTS)
def test_every_conversion_mutant_changes_a_ramp_case(mutant):
    found = _pack_changes(mutant)
    print(mutant, [f for f in found if f[0]])
    assert found[0][0] >= BAR, (mutant, found[:3])


@pytest.mark.parametrize("mutant,name", (("f16_truncate", "f16_ties"), ("f16_half_away", "f16_ties"), ("f16_flush_subnormals", "f16_subnormal"),
                                         ("f16_saturate", "f16_overflow"), ("bf16_truncate", "bf16_ties"), ("f32_flush", "f32_denormal"),
                                         ("u8_half_away", "u8_ties"), ("u8_truncate", "u8_ties"), ("u8_wrap", "u8_clamp"),
                                         ("fused_scale_bias", "imagenet_f32")))
def test_the_set_made_for_a_mutant_sees_it(mutant, name):
    got = {n: count for count, n, _ in _pack_changes(mutant)}
    assert got[name] >= BAR, (mutant, name, got[name])


@pytest.fixture(scope="module")
def resize_changes():
    """(mutant, case index) -> elements of the contraction case that the mutant changes."""
    found = {}
    for i, (frame, k, size, crop) in enumerate(ne.RESIZE_CONTRACTION):
        rgba = ne.FRAMES[frame]()[1]
        want = ne.expected_resized(rgba, size, k, "imagenet_f32", "f32", crop=crop)
        assert np.array_equal(ne.resized(rgba, size, k, "imagenet_f32", "f32", crop=crop), want)
        for mutant in ne.RESIZE_MUTANTS:
            found[mutant, i] = ne.changed(ne.resized(rgba, size, k, "imagenet_f32", "f32", crop=crop, mutant=mutant), want, "f32")
    print(found)
    return found


@pytest.mark.parametrize("mutant", ne.RESIZE_MUTANTS)
def test_every_resize_mutant_changes_the_contraction_cases(resize_changes, mutant):
    """Every mutant in at least three of the four cases, one of them on each frame."""
    seen = [i for i in range(len(ne.RESIZE_CONTRACTION)) if resize_changes[mutant, i] >= BAR]
    assert len(seen) >= 3 and {ne.RESIZE_CONTRACTION[i][0] for i in seen} == {"noisy", "ramp"}, (mutant, resize_changes)


@pytest.mark.parametrize("index", range(len(ne.RESIZE_CONTRACTION)))
def test_every_contraction_case_sees_a_resize_mutant(resize_changes, index):
    assert max(resize_changes[mutant, index] for mutant in ne.RESIZE_MUTANTS) >= BAR, (ne.RESIZE_CONTRACTION[index], resize_changes)


# ------------------------------------------------------------------- the reference against second opinions

def _values(name):
    """The float32 values of a set in front of the conversion, over every pack case."""
    _, scale, bias = ne.SETS[name]
    with np.errstate(over="ignore"):
        return np.concatenate([tr.expected(ne.FRAMES[frame]()[1], k, "f32", scale, bias).ravel() for frame, k in ne.PACKS])


@pytest.mark.parametrize("name", [n for n, d in ne.SET_DTYPES if d == "f16"])
def test_f16_cast_is_torchs(name):
    v = _values(name)
    with np.errstate(over="ignore"):
        mine = v.astype(np.float16)
    theirs = torch.from_numpy(v.copy()).to(torch.float16).numpy()
    assert np.array_equal(mine.view(np.uint16), theirs.view(np.uint16))
    if name == "f16_overflow":
        assert np.isposinf(mine).any() and np.isneginf(mine).any() and (mine == np.float16(65504)).any()
    if name == "f16_subnormal":
        sub = (mine != 0) & (np.abs(mine) < np.float16(2.0 ** -14))
        assert sub.sum() > 1000 and ((mine == 0) & (v != 0)).any()
    if name == "f16_inf":
        assert np.isinf(v).any() and (np.isinf(mine) & np.isfinite(v)).any()


@pytest.mark.parametrize("name", [n for n, d in ne.SET_DTYPES if d == "bf16"])
def test_bf16_formula_is_torchs(name):
    v = _values(name)
    mine = rr.store(v, "bf16")
    theirs = torch.from_numpy(v.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(mine, theirs)
    if name == "bf16_overflow":
        assert ((mine & 0x7fff) == 0x7f80).sum() > (np.isinf(v)).sum() > 0   # finite float32 that became the bf16 infinity


@pytest.mark.parametrize("name", [n for n, d in ne.SET_DTYPES if d == "u8"])
def test_u8_rule_in_integers_on_exact_halves(name):
    v = _values(name)
    mine = rr.store(v, "u8")
    assert np.array_equal(mine[np.isposinf(v)], np.full(int(np.isposinf(v).sum()), 255)) and not mine[np.isneginf(v)].any()
    finite = np.isfinite(v)
    twice = v[finite].astype(np.float64) * 2
    halves = twice == np.floor(twice)            # integers and exact halves: 2v is an integer
    if name == "u8_ties":
        assert (twice % 2 == 1).sum() > 10000
    halves &= np.abs(twice) < 2.0 ** 32          # (what an int64 holds; beyond it there is only the clamp)
    t = twice[halves].astype(np.int64)
    q, r = t >> 1, t & 1                         # v = q + r / 2 (floor division: negative v too)
    nearest = np.where(r == 0, q, q + (q & 1))   # a half goes to the even neighbour
    assert np.array_equal(mine[finite][halves], np.clip(nearest, 0, 255))
