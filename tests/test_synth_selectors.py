"""The synthetic encoder's table selectors (tools/synth.py: SELECTOR_SETS) and the walk route's sharing predicate.

Every decode route turns a component's Huffman and quantiser selectors into per-image state (desc.cpp: fill_desc,
coop_body.h: coop_tables, walk_body.h: walk_tabs).  The tests of the routes with other selectors than the encoder's
usual ones rest on two things checked here: that the encoder writes what it is asked to with nothing else changed,
and that desc.cpp's walk_state_shared -- may two images share one set of walk tables and the walk's flat grid --
tells such images apart."""
import os
import subprocess

import numpy as np
import pytest

import compeg_amd
from conftest import ROOT
from oracle import oracle as orc
from tools import synth

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
RUNNER = os.path.join(EMUL_DIR, "emul_runner")

W, H, RI = 160, 48, 4


def _segments(jpeg, marker):
    """The bytes of every segment with this marker in front of the scan, in order."""
    out, i = [], 2
    while i + 4 <= len(jpeg) and jpeg[i] == 0xFF and jpeg[i + 1] != 0xDA:
        n = int.from_bytes(jpeg[i + 2:i + 4], "big")
        if jpeg[i + 1] == marker:
            out.append(jpeg[i:i + 2 + n])
        i += 2 + n
    return out


def _components(img):
    """(Td, Ta, Tq) of every component, from the parsed metadata (front.h: Metadata)."""
    md = np.frombuffer(img.metadata(), dtype=np.uint32)
    comps = md[257:257 + 15].reshape(3, 5)   # vsample, hsample, qtable, dchuff = 2 Td, achuff = 2 Ta + 1
    return [(int(c[3]) >> 1, int(c[4]) >> 1, int(c[2])) for c in comps]


def _frame(tables=synth.DEFAULT_TABLES, qtables=synth.DEFAULT_QTABLES, quality=85, flags=0, seed=3, kind=0):
    return synth.make_jpeg(W, H, seed=seed, kind=kind, quality=quality, ri=RI, tables=tables, qtables=qtables, flags=flags)


def test_default_selectors_are_the_old_encoder():
    """make_jpeg's defaults give the bytes synth_encode (the entry point without selectors) gives."""
    for (w, h, q, sampling, ri, flags, kind) in [(W, H, 85, (2, 1), RI, 0, 0), (33, 17, 100, (1, 1), 1, 0, 1),
                                                 (250, 70, 50, (2, 2), 3, synth.JFIF, 0), (96, 32, 95, (1, 2), 0, synth.NO_DHT, 2)]:
        rgb = synth.fill(w, h, 5, kind)
        cap = w * h * 3 + 4096
        out = np.empty(cap, dtype=np.uint8)
        n = synth.lib().synth_encode(rgb.ctypes.data, w, h, q, sampling[0], sampling[1], ri, flags, out.ctypes.data, cap)
        assert 0 < n <= cap
        assert synth.encode(rgb, q, sampling, ri, flags) == out[:n].tobytes()
        assert synth.encode(rgb, q, sampling, ri, flags, tables=synth.SELECTOR_SETS["default"]) == out[:n].tobytes()


@pytest.mark.parametrize("name", sorted(synth.SELECTOR_SETS))
def test_selector_sets_recode_the_same_coefficients(name):
    """Only SOS changes: the DHT and DQT segments, the LUT bytes are those of the default frame; the parsed metadata
    carries the selectors asked for; and the standard-entropy decode (no quirk of the reference's reader) is the
    default frame's -- the same coefficients, coded with other tables."""
    tables = synth.SELECTOR_SETS[name]
    for kind, quality, seed in ((0, 85, 3), (1, 100, 4), (2, 60, 5)):
        base = _frame(quality=quality, seed=seed, kind=kind)
        j = _frame(tables=tables, quality=quality, seed=seed, kind=kind)
        assert _segments(j, 0xC4) == _segments(base, 0xC4) and len(_segments(j, 0xC4)) == 4
        assert _segments(j, 0xDB) == _segments(base, 0xDB)
        a, b = compeg_amd.ImageData(j), compeg_amd.ImageData(base)
        assert a.huffman_l1() == b.huffman_l1() and a.huffman_l2() == b.huffman_l2()
        assert _components(a) == [(td, ta, tq) for (td, ta), tq in zip(tables, synth.DEFAULT_QTABLES)]
        want = orc.ImageData(base, standard_entropy=True).decode()
        assert np.array_equal(orc.ImageData(j, standard_entropy=True).decode(), want), (name, kind)
        if name == "default":
            assert j == base


@pytest.mark.parametrize("qtables", [(1, 0, 0), (0, 0, 0), (1, 1, 1), (0, 1, 0)])
def test_quantiser_selectors(qtables):
    """Tq: the DQT and DHT segments stay, the metadata says which table each component takes, and the oracle's
    pixels move (the coefficients are quantised by another table)."""
    base = _frame()
    j = _frame(qtables=qtables)
    assert _segments(j, 0xDB) == _segments(base, 0xDB) and len(_segments(j, 0xDB)) == 2
    assert _segments(j, 0xC4) == _segments(base, 0xC4)
    assert [c[2] for c in _components(compeg_amd.ImageData(j))] == list(qtables)
    assert not np.array_equal(orc.ImageData(j).decode(), orc.ImageData(base).decode())


def test_no_zrl_tables():
    """NO_ZRL: both AC tables lose their ZRL symbol (one code each), and no data unit needs it -- the stream decodes
    in both entropy modes; the mode does not change the LUT bytes then."""
    j = _frame(flags=synth.NO_ZRL, kind=1, quality=100)
    dht = _segments(j, 0xC4)
    assert [len(s) for s in dht] == [len(s) - (s[4] >> 4) for s in _segments(_frame(), 0xC4)]
    for s in dht:
        if s[4] >> 4:   # AC tables
            assert 0xF0 not in s[5 + 16:]
    a, b = compeg_amd.ImageData(j), compeg_amd.ImageData(j, standard_entropy=True)
    assert a.huffman_l1() == b.huffman_l1() and a.huffman_l2() == b.huffman_l2()
    orc.ImageData(j).decode()
    orc.ImageData(j, standard_entropy=True).decode()


@pytest.fixture(scope="module")
def runner():
    import fcntl
    with open(os.path.join(EMUL_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", EMUL_DIR, "-s"])
    return RUNNER


def _walk_shared(runner, tmp_path, a, b, std_a=False, std_b=False):
    pa, pb = tmp_path / "a.jpg", tmp_path / "b.jpg"
    pa.write_bytes(a)
    pb.write_bytes(b)
    r = subprocess.run([runner, "--walk-shared", str(pa), str(int(std_a)), str(pb), str(int(std_b))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert r.stdout.startswith("shared "), r.stdout
    return r.stdout.split()[1] == "1"


def test_walk_state_shared(runner, tmp_path):
    """desc.cpp: walk_state_shared -- the condition of the walk route's flat grid (beside the same LUT bytes)."""
    default = _frame()
    assert _walk_shared(runner, tmp_path, default, default)
    assert _walk_shared(runner, tmp_path, default, _frame(quality=60, seed=9))   # other coefficients, other quantisers
    assert _walk_shared(runner, tmp_path, default, _frame(qtables=(1, 0, 0)))
    for name, tables in synth.SELECTOR_SETS.items():
        if name != "default":
            assert not _walk_shared(runner, tmp_path, default, _frame(tables=tables)), name
            assert not _walk_shared(runner, tmp_path, _frame(tables=tables), default), name
            assert _walk_shared(runner, tmp_path, _frame(tables=tables), _frame(tables=tables, seed=8)), name
    # the entropy modes
    nz = _frame(flags=synth.NO_ZRL)
    assert _walk_shared(runner, tmp_path, nz, nz)
    assert not _walk_shared(runner, tmp_path, nz, nz, False, True)
    assert not _walk_shared(runner, tmp_path, default, default, True, False)
    assert _walk_shared(runner, tmp_path, default, default, True, True)
