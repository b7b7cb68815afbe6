"""Every decode route at narrow, extreme and truncated geometries on the card (the cells of tests/route_matrix.py).

ROUTES below is the answer to "which route does X take": caller, layout, DRI class, launch class, preprocessing and
content give the kernel `last_kernel()` names, read off runtime.cpp's dispatch (compeg_decoder::enqueue near the
`route` condition; use_coop_kernel, coop_preferred, use_mcu_route, use_stream_kernel, use_pair_kernel;
compeg_batch::decode) and confirmed on the MI355X.  Every decode asserts its row, and every decode is compared with the
oracle: a fresh Decoder per cell (the whole output), one Decoder reused through all cells (textures grow and are
reused: the W x H corner, without the MCUs no complete restart interval covers), batches that reach each batch route
with narrow images (unchunked and chunked unevenly, preprocessing 0 / 1 / 2, one Batch object per mode re-uploaded
across route changes), and the laboratory build's route switches in subprocesses.  A counter of (kernel, layout, width
class, DRI class, entropy) fails the module if a route the table reaches has no decode in some width or DRI class."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import route_matrix as rm

pytestmark = pytest.mark.gpu

ANY = "*"
LAYOUTS = ("422", "444", "440", "420")
EXT = ("444", "440", "420")
# (caller, layouts, DRI classes, launch class, preprocessing, content) -> kernel: the first row that matches is the one.
#   launch class -- decoder: "small" (tests/route_matrix.py small_cells), "strip", "extreme"; batch: the recipe's name
#   (BATCHES), "/chunked" behind it for the uneven chunks.  preprocessing -- decoder: host / device; batch: 0 / 1 / 2.
ROUTES = [
    # no complete restart interval: nothing is launched, a fresh texture stays all zeros
    ("decoder", LAYOUTS, ("beyond",), ANY, ANY, ANY, ("none",)),
    # 4:2:2 up to 64 MCUs an interval, and small frames without DRI (one interval of at most 9 MCUs): a launch far below
    # the cooperative kernel's limit, which it is preferred for (coop_preferred: DRI < 8, or all teams resident at once)
    ("decoder", ("422",), ("1", "2-9", "trunc", "8", "40", "41", "64"), ANY, ANY, ANY, ("coop_team",)),
    ("decoder", ("422",), ("none",), ("small",), ANY, ANY, ("coop_team",)),
    # DRI = 65 on the strips: the cooperative kernel, but dense scans preprocessed on the device plan its windows from an
    # estimated span (coop_spans_estimate), which leaves no usable plan: the streamed kernel then
    ("decoder", ("422",), ("65",), ("strip",), ANY, ANY, ("coop_team", "fused_stream")),
    # DRI = 256: no usable cooperative plan for these one-MCU strips; paired or streamed kernel by the window the span
    # asks for (use_stream_kernel: window_cut)
    ("decoder", ("422",), ("256",), ("strip",), ANY, ANY, ("pair", "fused_stream")),
    # longer than kCoopMaxRestart (no DRI: the whole image one interval): the walk + lane-per-MCU route where its terms
    # hold (mcu_words_avg <= 24, the walk tables take the image), else the paired or the streamed kernel
    ("decoder", ("422",), ("257", "none"), ("strip", "extreme"), ANY, ANY, ("walk_mcu", "pair", "fused_stream")),
    # extension layouts: intervals of one MCU have no streamed form in 4:4:4 / 4:4:0 (layout_has_stream_kernel)
    ("decoder", ("444", "440"), ("1",), ANY, ANY, ANY, ("fused_layout",)),
    # ... long intervals cut the whole-interval windows: streamed
    ("decoder", EXT, ("long",), ("strip",), ANY, ANY, ("fused_stream",)),
    # ... else whole windows or streamed as the largest word span of 64 intervals fits the LDS window (window_cut; on
    # the device path the span is an estimate, twice the average)
    ("decoder", EXT, ANY, ANY, ANY, ANY, ("fused_layout", "fused_stream")),
    # batches: the recipes of BATCHES, each built for its route
    ("batch", ("422",), ANY, ("fused", "fused/chunked"), ANY, ANY, ("fused",)),
    ("batch", ("422",), ANY, ("pair", "pair/chunked"), ANY, ANY, ("pair",)),
    ("batch", ("422",), ANY, ("coop", "coop/chunked"), ANY, ANY, ("coop_team",)),
    ("batch", ("422",), ANY, ("stream", "stream/chunked"), ANY, ANY, ("fused_stream",)),
    ("batch", ("422",), ANY, ("walk", "walk_long", "walk_long/chunked"), ANY, ANY, ("walk_mcu",)),
    # (chunks of 170 and 130 images: the smallest launch is within the cooperative kernel's limit, so use_mcu_route
    # keeps the cooperative kernel for every launch of the decode -- the records are planned for the whole batch)
    ("batch", ("422",), ANY, ("walk/chunked",), ANY, ANY, ("coop_team",)),
    # 4:4:4 at DRI 2 / 3: whole windows; 4:4:0 and 4:2:0 (16-pixel MCU columns: twice the words an interval) streamed
    ("batch", ("444",), ANY, ("layout", "layout/chunked"), ANY, ANY, ("fused_layout",)),
    ("batch", ("440", "420"), ANY, ("layout", "layout/chunked"), ANY, ANY, ("fused_stream",)),
    ("batch", EXT, ANY, ("layout_stream", "layout_stream/chunked"), ANY, ANY, ("fused_stream",)),
    ("batch", LAYOUTS, ANY, ("mixed", "mixed/chunked"), ANY, ANY, ("generic",)),
]


def expected(caller, layout, dri, launch, prep, content):
    for c, lays, dris, launches, preps, contents, kernel in ROUTES:
        if (c == caller and layout in lays and (dris == ANY or dri in dris) and (launches == ANY or launch in launches)
                and (preps == ANY or prep in preps) and (contents == ANY or content in contents)):
            return kernel
    raise AssertionError(f"no row of ROUTES for {(caller, layout, dri, launch, prep, content)}")


COUNT = collections.Counter()   # (kernel, layout, width class, DRI class, entropy) over every decode of this module
SEEN = {}                       # row key -> kernels seen (printed: the table as the card has it)
FAILS = []


@pytest.fixture(scope="module")
def ca():
    import compeg_amd
    return compeg_amd


@pytest.fixture(scope="module")
def gpu(ca):
    return ca.Gpu.open(0)


def _note(key, got, cells):
    SEEN.setdefault(key, set()).add(got)
    want = expected(*key)
    if got not in want:
        FAILS.append(f"route: {key}: last_kernel() = {got}, ROUTES says {'/'.join(want)}; {cells[0].name}")
    for c in cells:
        COUNT[(got, c.layout, c.width_class, c.dri_class, c.entropy)] += 1


def _compare(got, want, what, mask=None):
    if got.shape != want.shape:
        FAILS.append(f"pixels: {what}: shape {got.shape} != {want.shape}")
        return
    diff = (got != want).any(axis=2)
    if mask is not None:
        diff &= mask
    if diff.any():
        ys, xs = np.nonzero(diff)
        FAILS.append(f"pixels: {what}: {int(diff.sum())} differ, first at x={xs[0]} y={ys[0]}")


def _launch(cell):
    if cell in rm.small_cells(cell.layout):
        return "small"
    return "extreme" if rm.EXTREME in (cell.w, cell.h) else "strip"


def _decode_cells(ca, gpu, layout, device):
    prep = "device" if device else "host"
    reused = ca.Decoder(gpu)
    reused.set_device_preprocess(device)
    for cell in rm.cells(layout):
        img = ca.ImageData(cell.jpeg(), **cell.image_kw())
        want = rm.want(cell)
        key = ("decoder", layout, cell.dri_class, _launch(cell), prep, cell.content)
        fresh = ca.Decoder(gpu)
        fresh.set_device_preprocess(device)
        for dec, tag in ((fresh, "fresh"), (reused, "reused")):
            for blocking in (True, False):
                if blocking:
                    dec.decode_blocking(img)
                else:
                    dec.start_decode(img).wait()
                _note(key, dec.last_kernel(), [cell])
                got = dec.read_texture(cell.w, cell.h)
                what = f"decoder {tag} {prep} {'blocking' if blocking else 'start_decode'}: {cell.name}"
                _compare(got, want, what, None if tag == "fresh" else cell.covered_mask())
        if cell.dri_class == "beyond":
            assert not fresh.read_texture(cell.w, cell.h).any(), cell.name


@pytest.mark.parametrize("layout", LAYOUTS)
def test_decoder_cells(ca, gpu, layout):
    """Every cell of the layout, blocking and start_decode, host and device preprocessing: a fresh Decoder (the whole
    output) and one reused through the cells in order (the corner; uncovered MCUs masked)."""
    FAILS.clear()
    for device in (False, True):
        _decode_cells(ca, gpu, layout, device)
    assert not FAILS, f"{len(FAILS)} failures:\n" + "\n".join(FAILS[:60])


def _tall(layout, ri, content="clean", mcus=540, std_every=2, seed=0):
    """Cells of every width class, one to three MCUs across, `mcus` MCUs each (equal interval counts: a flat grid)."""
    mw, mh = 8 * rm.LAYOUTS[layout][0], 8 * rm.LAYOUTS[layout][1]
    out = []
    for k, wc in enumerate(rm.SIZE_CLASSES):
        w = rm.size_of(wc, mw)
        wm = (w + mw - 1) // mw
        out.append(rm.Cell(layout, w, (mcus // wm) * mh - k % 2 - seed % 2, ri, k % std_every == 1, content))
    return out


def _cycle(cells, n):
    return [cells[i % len(cells)] for i in range(n)]


# name -> (cells of the batch, chunk): narrow images at counts that reach each batch route
BATCHES = {
    # DRI 1, 9 waves an image, 260 images: beyond the cooperative kernel's launches (4 x 540 x 260 data units) and the
    # paired kernel's (2340 waves); chunks of 250 the same, the last (10 images) the cooperative kernel's
    "fused": (lambda: _cycle(_tall("422", 1), 260), 250),
    # DRIs of 1 and 2 mixed: no common interval for the cooperative kernel, a one-MCU DRI in the batch closes the walk
    # (clean frames: the dense ones' windows would be cut -- streamed)
    "pair": (lambda: _cycle(_tall("422", 1) + _tall("422", 2, seed=1), 24), 7),
    "coop": (lambda: _cycle(_tall("422", 7) + _tall("422", 7, "q100", seed=1), 12), 5),
    # intervals longer than kCoopMaxRestart, dense: the walk's rows cannot hold them; whole windows cut -- streamed
    "stream": (lambda: _cycle(_tall("422", 0, "q100") + _tall("422", 257, "q100", seed=1), 24), 7),
    # ... clean: the walk route for any count (no cooperative kernel for these DRIs)
    "walk_long": (lambda: _cycle(_tall("422", 0) + _tall("422", 257, seed=1), 24), 7),
    # DRI 65, 8 intervals of 540 MCUs: 300 images are beyond the cooperative kernel (8 x 300 x 4 x 65 data units)
    "walk": (lambda: _cycle(_tall("422", 65), 300), 170),
    "layout": (lambda: [c for lay in EXT for c in _cycle(_tall(lay, 2) + _tall(lay, 3, seed=1), 16)], None),
    "layout_stream": (lambda: [c for lay in EXT for c in _cycle(_tall(lay, 0, "q100"), 16)], None),
    "mixed": (lambda: _cycle([c for lay in LAYOUTS for c in _tall(lay, 3)], 40), 9),
}


def _decode_batch(ca, batch, cells, chunk, launch, mode):
    batch.set_chunk(0)
    imgs = [ca.ImageData(c.jpeg(), allow_sampling=True, standard_entropy=c.standard) for c in cells]
    batch.upload(imgs)
    for ch in (0, chunk):
        batch.set_chunk(ch)
        batch.decode()
        batch.wait()
        what = launch + ("/chunked" if ch else "")
        layout = cells[0].layout if len({c.layout for c in cells}) == 1 else "422"
        _note(("batch", layout, cells[0].dri_class, what, mode, cells[0].content), batch.last_kernel(), cells)
        for i, c in enumerate(cells):
            _compare(batch.read_output(i), rm.want(c), f"batch {what} mode={mode} slot {i}: {c.name}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_batch_cells(ca, gpu, mode):
    """The recipes of BATCHES through one Batch object (re-uploaded across route changes), unchunked and chunked; the
    extension layouts' recipes one layout per batch."""
    FAILS.clear()
    batch = ca.Batch(gpu)
    batch.set_device_preprocess(mode)
    for name, (make, chunk) in BATCHES.items():
        cells = make()
        if name.startswith("layout"):
            for lay in EXT:
                part = [c for c in cells if c.layout == lay]
                _decode_batch(ca, batch, part, chunk or 5, name, mode)
        else:
            _decode_batch(ca, batch, cells, chunk, name, mode)
    assert not FAILS, f"{len(FAILS)} failures:\n" + "\n".join(FAILS[:60])


# The laboratory build's route switches (compeg_amd/csrc/lab.h): each knob set in a fresh process, the small cells of
# every layout through a Decoder and through a batch of the layout's cells; (the 4:2:2 cells below DRI 8, where the
# decoder's walk route is not possible).  Only switches that turn routes off or choose among routes that take every
# input of their layout.
LAB = [
    ({"COMPEG_PIPELINE": "split"}, {"422": "split", "ext": "generic"}, {"422": "split", "ext": "generic"}),
    ({"COMPEG_COOP": "0", "COMPEG_PAIR": "0", "COMPEG_STREAM": "0", "COMPEG_WALK": "0"},
     {"422": "fused", "ext": "fused_layout"}, {"422": "fused", "ext": "fused_layout"}),
    ({"COMPEG_COOP": "0", "COMPEG_PAIR": "1", "COMPEG_STREAM": "0", "COMPEG_WALK": "0", "COMPEG_NO_DECODER_ROUTE": "1"},
     {"422": "pair", "ext": "fused_layout"}, {"422": "pair", "ext": "fused_layout"}),
    ({"COMPEG_COOP": "0", "COMPEG_STREAM": "1", "COMPEG_WALK": "0", "COMPEG_NO_DECODER_ROUTE": "1"},
     {"422": "fused_stream", "ext": "stream_or_layout"}, {"422": "fused_stream", "ext": "stream_or_layout"}),
]

_LAB_CODE = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import compeg_amd as ca
import route_matrix as rm
gpu = ca.Gpu.open(0)
for layout in ("422", "444", "440", "420"):
    cells = [c for c in rm.small_cells(layout) if c.dri_class != "beyond" and (layout != "422" or (c.ri or c.mcus) < 8)]
    dec = ca.Decoder(gpu)
    for c in cells:
        dec.decode_blocking(ca.ImageData(c.jpeg(), **c.image_kw()))
        ok = bool(np.array_equal(dec.read_texture(c.w, c.h)[c.covered_mask()], rm.want(c)[c.covered_mask()]))
        print(json.dumps(["decoder", layout, c.w, c.h, c.ri, c.standard, c.content, dec.last_kernel(), ok]), flush=True)
    b = ca.Batch(gpu)
    b.upload([ca.ImageData(c.jpeg(), allow_sampling=True, standard_entropy=c.standard) for c in cells])
    b.decode()
    b.wait()
    k = b.last_kernel()
    for i, c in enumerate(cells):
        print(json.dumps(["batch", layout, c.w, c.h, c.ri, c.standard, c.content, k,
                          bool(np.array_equal(b.read_output(i), rm.want(c)))]), flush=True)
print("lab done")
'''


def _lab_ok(kernel, want, cell):
    if want == "stream_or_layout":   # (the streamed form exists for 4:2:0 and the paired 4:4:4 / 4:4:0 kernels)
        paired = cell.layout == "420" or (cell.ri or cell.mcus) >= 2
        return kernel == ("fused_stream" if paired else "fused_layout")
    return kernel == want


def test_lab_route_switches(ca, gpu):
    lab = os.path.join(os.path.dirname(ca.LIB_PATH), "libcompeg_hip_lab.so")
    assert os.path.exists(lab), "make -C compeg_amd/csrc lab (__graft_entry__.build() does)"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    FAILS.clear()
    for knobs, dec_want, batch_want in LAB:
        r = subprocess.run([sys.executable, "-c", _LAB_CODE, root], env=dict(os.environ, COMPEG_LIB=lab, **knobs),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "lab done" in r.stdout, (knobs, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        for line in r.stdout.splitlines():
            if not line.startswith("["):
                continue
            caller, layout, w, h, ri, std, content, kernel, ok = json.loads(line)
            cell = rm.Cell(layout, w, h, ri, std, content)
            want = (dec_want if caller == "decoder" else batch_want)["422" if layout == "422" else "ext"]
            if caller == "batch" and layout != "422":
                want = "fused_stream" if want == "stream_or_layout" and layout == "420" else want
            if not _lab_ok(kernel, want, cell) and not (caller == "batch" and want == "stream_or_layout"):
                FAILS.append(f"lab {knobs} {caller}: {kernel}, expected {want}: {cell.name}")
            if not ok:
                FAILS.append(f"lab {knobs} {caller} {kernel}: pixels differ: {cell.name}")
            COUNT[(kernel, layout, cell.width_class, cell.dri_class, cell.entropy)] += 1
    assert not FAILS, f"{len(FAILS)} failures:\n" + "\n".join(FAILS[:60])


def test_route_coverage():
    """Every (kernel, layout) pair ROUTES reaches has decodes in every width class and in every DRI class of its rows.
    (Runs behind the module's decodes; alone, it fails: nothing counted.)"""
    print("route matrix counter:")
    for k, v in sorted(COUNT.items()):
        print("  ", k, v)
    print("routes seen (key -> kernels):")
    for k, v in sorted(SEEN.items()):
        print("  ", k, sorted(v))
    reach = collections.defaultdict(set)
    for caller, lays, dris, launches, preps, contents, kernels in ROUTES:
        for lay in lays:
            for kernel in kernels:
                reach[(kernel, lay)] |= set() if dris == ANY else set(dris)
    empty = []
    for (kernel, lay), dris in sorted(reach.items()):
        got = [key for key in COUNT if key[0] == kernel and key[1] == lay]
        for w in sorted(set(rm.SIZE_CLASSES) - {key[2] for key in got}):
            empty.append((kernel, lay, "width", w))
        for d in sorted(dris - {key[3] for key in got}):
            empty.append((kernel, lay, "dri", d))
    assert not empty, f"reachable routes without a decode: {empty}"
