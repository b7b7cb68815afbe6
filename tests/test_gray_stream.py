"""Grayscale frames (tests/gray_stream.py) against the oracle's decode of their 4:4:4 twins and the host front end (no GPU).

The definition of "right": a grayscale image decodes to what the decoder gives for its twin -- the same file with two more
components of flat data units.  Where neither stream runs the reference's reader dry (quirk Q1) the restatement
(gs.expectation) must equal the oracle's pixels for the twin bit for bit; where one does, their bit positions differ and
the restatement stands alone -- such a case exists, found by search.  Real encoders' files (the six golden fixtures, PIL's
`L` images) round-trip through gs.from_jpeg, which makes their expectation.  Then the front end: what is accepted and
rejected with which message, that flag 0 changes nothing, the metadata block field by field, the LUTs against the oracle's
for the twin, and the oracle's own entropy pass over the block against cs.predict."""
import ctypes as C
import io

import numpy as np
import pytest

import coef_stream as cs
import compeg_amd as ca
import gray_stream as gs
from conftest import read_golden
from oracle import oracle as orc

NAMES = [f.name for f in gs.cases()]
FIXTURES = ("grayscale_square", "grayscale_long", "grayscale_large", "grayscale_16x24_sampling2x2", "grayscale_24x16_sampling2x2",
            "blank_800x280")


def fixture(name):
    return read_golden("parser", name + ".jpg")


def pil_l(w, h, quality, blocks, seed=3):
    from PIL import Image
    rng = np.random.default_rng(seed + w * 31 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.clip(96 + 60 * np.sin(xx / 3.0) + 50 * np.cos(yy / 2.0) + rng.integers(-40, 41, (h, w)), 0, 255).astype(np.uint8)
    out = io.BytesIO()
    kw = dict(restart_marker_blocks=blocks) if blocks else {}
    Image.fromarray(img, "L").save(out, "JPEG", quality=quality, **kw)
    return out.getvalue()


def both_facts(f):
    a, b = {}, {}
    cs.predict(f, facts=a)
    cs.predict(gs.twin(f), facts=b)
    return a, b


# ---- the twin ---------------------------------------------------------------------------------------------------------

MET = [f.name for f in gs.cases() if not any(x["dry"] for x in both_facts(f))]   # (neither reader runs dry)


@pytest.mark.parametrize("name", MET)
def test_expectation_is_the_oracles_decode_of_the_twin(name):
    f = gs.case(name)
    t = gs.twin(f)
    want = orc.ImageData(t.jpeg(), **t.image_kw()).decode(strict=True)
    got = gs.expectation(f)
    assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} pixels differ"
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2]) and (got[..., 3] == 255).all()


def test_enough_cases_meet_the_twin_and_some_cannot():
    """Both entropy modes, every DRI and every width of the issue's list among the cases compared with the oracle; and a
    reference-mode case whose own reader runs dry (found by search over a filler coefficient's size), where the twin
    cannot serve."""
    assert all(n in MET for n in NAMES if "/standard" in n), "a topped-up reader never runs dry"
    assert all(n in MET for n in NAMES if n.startswith("random_gray/")), "8-bit codes: neither reader runs dry"
    met = {(f.standard, f.ri, f.mcus_w) for f in map(gs.case, MET)}
    for std in (False, True):
        assert {ri for s, ri, _ in met if s == std} >= {0, 1, 2, 3, 7}, (std, sorted(met))
        assert {w for s, _, w in met if s == std} >= {1, 2, 5, 6}, (std, sorted(met))
    found = None
    huff = cs.table_set("long", range(16), [0x00] + list(range(1, 16)))
    for size in range(1, 16):
        dus = [(0, [cs.ac(0, 1 << (size - 1)), cs.EOB]), (20000, [cs.EOB]), (-3, [cs.EOB]), (5, [cs.EOB])]
        f = gs.GrayFrame(f"dry/size{size}", "gray", 2, 2, dus, huff, ri=4, quant=(1, 1), sel=((0, 0, 0),) * 3)
        facts = {}
        cs.predict(f, facts=facts)
        if facts["dry"]:
            found = found or (f, facts)
    assert found, "no filler size leaves the reader short at the next DC code"
    f, facts = found
    assert facts["dry"] >= 1 and facts["underflow_left"]
    assert ca.ImageData(f.jpeg(), **f.image_kw()).parallelism() == 1
    assert gs.expectation(f).shape == (16, 16, 4)


# ---- real encoders' files ---------------------------------------------------------------------------------------------

PIL_FILES = [(w, h, q, b) for (w, h) in ((8, 8), (10, 10), (17, 9), (40, 24)) for q in (50, 95) for b in (0, 1, 2, 3)]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_round_trips(name):
    j = fixture(name)
    f = gs.from_jpeg(j, name)
    assert gs.scan_bytes(f) == gs.file_scan(j)
    img = ca.ImageData(j, allow_grayscale=True)
    assert (img.width(), img.height(), img.components()) == (f.w, f.h, 1)
    assert img.parallelism() == f.intervals


@pytest.mark.parametrize("w,h,quality,blocks", PIL_FILES)
def test_pil_file_round_trips(w, h, quality, blocks):
    j = pil_l(w, h, quality, blocks)
    f = gs.from_jpeg(j)
    assert gs.scan_bytes(f) == gs.file_scan(j)
    assert (f.ri, f.w, f.h) == (blocks, w, h)
    # (its own writer's file parses to the same picture as the encoder's)
    a, b = ca.ImageData(j, allow_grayscale=True), ca.ImageData(f.jpeg(), allow_grayscale=True)
    assert a.huffman_l1() == b.huffman_l1() and a.metadata() == b.metadata()


# ---- the front end ----------------------------------------------------------------------------------------------------

def _message(jpeg, **kw):
    with pytest.raises(ca.Error) as e:
        ca.ImageData(jpeg, **kw)
    return str(e.value)


def _frame():
    return gs.case(NAMES[0])


def _with_sof(j, comp_bytes=None, ncomp=None):
    at = j.index(b"\xff\xc0")
    body = bytearray(j[at + 4:at + 2 + int.from_bytes(j[at + 2:at + 4], "big")])
    if comp_bytes is not None:
        body[6:9] = comp_bytes
    if ncomp is not None:
        body[5] = ncomp
        body = body[:6] + bytes([1, 0x11, 0, 2, 0x11, 0, 3, 0x11, 0, 4, 0x11, 0])[:3 * ncomp]
    return j[:at] + b"\xff\xc0" + (len(body) + 2).to_bytes(2, "big") + bytes(body) + j[at + 2 + int.from_bytes(j[at + 2:at + 4], "big"):]


def test_accepts_and_rejects_with_its_messages():
    f = _frame()
    j = f.jpeg()
    assert ca.ImageData(j, allow_grayscale=True).components() == 1
    for kw in (dict(allow_sampling=True), dict(standard_entropy=True), dict(allow_sampling=True, standard_entropy=True)):
        assert ca.ImageData(j, allow_grayscale=True, **kw).components() == 1
    for hv in (0x11, 0x22, 0x41, 0x14, 0x44, 0x23):
        img = ca.ImageData(_with_sof(j, bytes([1, hv, 0])), allow_grayscale=True)
        assert (img.width(), img.height(), img.parallelism()) == (f.w, f.h, f.intervals)
    assert "invalid sampling factors 0x1 for the only component" in _message(_with_sof(j, bytes([1, 0x01, 0])), allow_grayscale=True)
    assert "invalid sampling factors 5x1 for the only component" in _message(_with_sof(j, bytes([1, 0x51, 0])), allow_grayscale=True)
    assert "invalid sampling factors 1x0 for the only component" in _message(_with_sof(j, bytes([1, 0x10, 0])), allow_grayscale=True)
    assert "invalid quantization table selection [4]" in _message(_with_sof(j, bytes([1, 0x11, 4])), allow_grayscale=True)
    assert "frame with 2 components not supported" in _message(_with_sof(j, ncomp=2), allow_grayscale=True)
    assert "frame with 4 components not supported" in _message(_with_sof(j, ncomp=4), allow_grayscale=True)
    assert "scan with 3 components not supported (the frame has 1 component)" in _message(gs.write(f, ncomp_in_scan=3), allow_grayscale=True)
    assert "scan component index mismatch (expected component [1], got [2])" in _message(gs.write(f, scan_id=2), allow_grayscale=True)
    # a colour frame under the flag: as without it
    c = cs.case("dc_cats/short/422/reference/dri1")
    assert ca.ImageData(c.jpeg(), allow_grayscale=True).components() == 3
    assert ca.ImageData(c.jpeg(), allow_grayscale=True).metadata() == ca.ImageData(c.jpeg()).metadata()
    # the C ABI takes the flag and no unknown one
    h = C.c_void_p()
    buf = np.frombuffer(j, dtype=np.uint8)
    assert ca.lib.compeg_image_parse_ext(buf.ctypes.data, buf.nbytes, 1, 8, C.byref(h)) != 0
    assert ca.lib.compeg_image_parse_ext(buf.ctypes.data, buf.nbytes, 1, 4 | 2 | 1, C.byref(h)) == 0
    assert ca.lib.compeg_image_components(h) == 1
    ca.lib.compeg_image_free(h)


def test_without_the_flag_every_message_is_todays():
    files = [fixture(n) for n in FIXTURES] + [_frame().jpeg(), pil_l(17, 9, 50, 0)]
    for j in files:
        for kw in ({}, dict(allow_sampling=True), dict(standard_entropy=True)):
            assert "frame with 1 components not supported (only 3 components are supported)" in _message(j, **kw)
            with pytest.raises(orc.OracleError) as e:
                orc.ImageData(j, **kw)
            assert str(e.value) in _message(j, **kw)


def _block(f, tq_rows):
    md = np.zeros(278, dtype=np.uint32)
    for t, row in tq_rows.items():
        md[64 * t:64 * t + 64] = row
    td, ta, tq = f.sel[0]
    md[256] = f.interval                                   # restart_interval
    md[257:262] = (1, 1, tq, 2 * td, 2 * ta + 1)           # component 0: vsample, hsample, qtable, dchuff, achuff
    md[272] = f.intervals                                  # total_restart_intervals (components 1 and 2: zero)
    md[273] = f.mcus_w                                     # width_mcus
    md[274:278] = (1, 1, 1, 32)                            # max_hsample, max_vsample, dus_per_mcu, retained_coefficients
    return md.tobytes()


@pytest.mark.parametrize("name", NAMES[:12] + list(FIXTURES[3:5]))
def test_metadata_block_and_luts(name):
    if name in FIXTURES:
        j = fixture(name)
        f = gs.from_jpeg(j, name)
    else:
        f = gs.case(name)
        j = f.jpeg()
    img = ca.ImageData(j, **f.image_kw())
    rows = {t: f.qtable(t) for t in range(len(f.quant))}
    assert len(img.metadata()) == 1112 and img.metadata() == _block(f, rows)
    assert img.components() == 1
    if name in FIXTURES:
        return
    t = gs.twin(f)
    o = orc.ImageData(t.jpeg(), **t.image_kw())
    assert img.huffman_l1() == o.l1() and img.huffman_l2() == o.l2()
    off, n = img.scan_range()
    assert j[off:off + n] == gs.scan_bytes(f)


@pytest.mark.parametrize("name", [n for n in NAMES if "/standard" not in n][:24])
def test_oracles_entropy_pass_over_the_block_gives_the_predicted_coefficients(name):
    """orc_huffman_pass is generic over a metadata block (reference entropy): fed the one-component block, LUTs and
    preprocessed scan of the product's front end it keeps cs.predict's coefficients."""
    f = gs.case(name)
    if f.standard:
        pytest.skip("orc_huffman_pass is the reference's entropy mode")
    img = ca.ImageData(f.jpeg(), allow_grayscale=True)
    off, n = img.scan_range()
    sb = orc.ScanBuffer()
    sb.process(f.jpeg()[off:off + n], img.parallelism())
    words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32).copy()
    starts = np.frombuffer(sb.start_positions(), dtype=np.uint32).copy()
    md, l1, l2 = (np.frombuffer(b, dtype=np.uint8).copy() for b in (img.metadata(), img.huffman_l1(), img.huffman_l2() or b"\0\0"))
    ndus = f.intervals * f.interval
    coef = np.zeros(ndus * 32, dtype=np.int32)
    orc.lib().orc_huffman_pass(md.ctypes.data, l1.ctypes.data, l2.ctypes.data, len(img.huffman_l2()), words.ctypes.data, words.size,
                               starts.ctypes.data, starts.size, coef.ctypes.data, coef.size)
    pred = cs.predict(f)
    assert np.array_equal(coef.reshape(-1, 32), pred[:, :32])
