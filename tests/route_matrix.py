"""Decode cells at narrow, extreme and truncated geometries, shared by tests/test_route_matrix_emulation.py (the emulated
kernel bodies) and tests/test_gpu_route_matrix.py (the shipped dispatch on the card).  A plain module, no fixtures.

A cell is one synthetic frame: a layout (MCU = 8 hs x 8 vs pixels), a width and a height from the size classes below,
a restart interval (DRI), an entropy mode and a content.  Every cell carries its seed; `cell.name` says all of it, so a
failure message can name the frame to rebuild."""
import zlib
from dataclasses import dataclass

import numpy as np

from oracle import oracle as orc
from tools import synth

LAYOUTS = {"422": (2, 1), "444": (1, 1), "440": (1, 2), "420": (2, 2)}

# size classes of one axis, in MCUs of that axis (m): 1 pixel, one MCU less a pixel, one MCU, one pixel more, two MCUs,
# three less a pixel, three (an odd count of MCUs a row)
SIZE_CLASSES = ("1px", "mcu-1", "mcu", "mcu+1", "2mcu", "3mcu-1", "3mcu")
STRIP_MCUS = 520      # the strips' long axis: >= 200 MCUs, and room for two intervals of 257 and a truncated third
EXTREME = 65528       # the largest extent front.cpp accepts (w + 7 must fit 16 bits)
SMALL_DRIS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
EDGE_DRIS = (8, 40, 41, 64, 65, 256, 257)      # 4:2:2's dispatch edges (coop_shape, kCoopLeanMaxRestart, kCoopMaxRestart)
LAYOUT_STRIP_DRIS = (0, 1, 2, 3, 9, 64, 65)
CONTENTS = ("clean", "q100")


def size_of(cls, m):
    return {"1px": 1, "mcu-1": m - 1, "mcu": m, "mcu+1": m + 1, "2mcu": 2 * m, "3mcu-1": 3 * m - 1, "3mcu": 3 * m}[cls]


def size_class(n, m):
    """The class of an extent of n pixels on an axis of m-pixel MCUs (the strips' long axis: "strip")."""
    if n == EXTREME:
        return "extreme"
    for c in SIZE_CLASSES:
        if size_of(c, m) == n:
            return c
    return "strip" if n >= 200 * m else "other"


def dri_class(layout, ri, mcus):
    """none: no DRI (one interval: the whole image); beyond: a DRI above the MCU count (no complete interval); 4:2:2's
    dispatch edges by value; otherwise 1, 2-9 (dividing the MCU count), trunc (the last interval cut short), long."""
    if ri == 0:
        return "none"
    if ri > mcus:
        return "beyond"
    if layout == "422" and ri in EDGE_DRIS:
        return str(ri)
    if ri == 1:
        return "1"
    if mcus % ri:
        return "trunc"
    return "2-9" if ri <= 9 else "long"


@dataclass(frozen=True)
class Cell:
    layout: str
    w: int
    h: int
    ri: int
    standard: bool
    content: str

    @property
    def mcu(self):
        hs, vs = LAYOUTS[self.layout]
        return 8 * hs, 8 * vs

    @property
    def mcus_wh(self):
        mw, mh = self.mcu
        return (self.w + mw - 1) // mw, (self.h + mh - 1) // mh

    @property
    def mcus(self):
        a, b = self.mcus_wh
        return a * b

    @property
    def intervals(self):
        return 1 if self.ri == 0 else self.mcus // self.ri

    @property
    def width_class(self):
        return size_class(self.w, self.mcu[0])

    @property
    def height_class(self):
        return size_class(self.h, self.mcu[1])

    @property
    def dri_class(self):
        return dri_class(self.layout, self.ri, self.mcus)

    @property
    def entropy(self):
        return "standard" if self.standard else "reference"

    @property
    def seed(self):
        return zlib.crc32(f"{self.layout} {self.w} {self.h} {self.ri} {self.standard} {self.content}".encode()) & 0x3FFFFFFF

    @property
    def name(self):
        return (f"{self.layout} {self.w}x{self.h} ({self.width_class} x {self.height_class}) DRI={self.ri} "
                f"({self.dri_class}) {self.entropy} {self.content} seed={self.seed}")

    def jpeg(self):
        q100 = self.content == "q100"
        return synth.make_jpeg(self.w, self.h, seed=self.seed, kind=1 if q100 else self.seed % 3, quality=100 if q100 else 85,
                               ri=self.ri, sampling=LAYOUTS[self.layout], flags=synth.NO_ZRL if self.standard else 0)

    def image_kw(self):
        return dict(allow_sampling=self.layout != "422", standard_entropy=self.standard)

    def covered_mask(self):
        """Pixels of the MCUs some complete restart interval covers (a reused texture keeps the others from earlier
        images, like the reference's; the oracle starts from zeros: tools/fuzz_gpu.py)."""
        mw, mh = self.mcu
        wm, _ = self.mcus_wh
        covered = self.intervals * self.ri if self.ri else self.mcus
        mask = np.zeros((self.h, self.w), dtype=bool)
        full_rows = covered // wm
        mask[:full_rows * mh] = True
        if covered % wm:
            mask[full_rows * mh:(full_rows + 1) * mh, :(covered % wm) * mw] = True
        return mask


_WANT = {}


def want(cell_or_jpeg, standard=False, sampling=True):
    """The oracle's decode (cached by frame bytes)."""
    if isinstance(cell_or_jpeg, Cell):
        jpeg, standard = cell_or_jpeg.jpeg(), cell_or_jpeg.standard
    else:
        jpeg = cell_or_jpeg
    key = (jpeg, standard, sampling)
    if key not in _WANT:
        _WANT[key] = orc.ImageData(jpeg, allow_sampling=sampling, standard_entropy=standard).decode()
    return _WANT[key]


def small_cells(layout):
    """Every width class against every DRI (none, 1-9, one beyond the MCU count); the height class walks round the
    classes so that portrait and landscape frames, odd MCU counts a row and truncated last intervals all come up;
    entropy mode and content alternate."""
    m = LAYOUTS[layout]
    out = []
    dris = SMALL_DRIS + (-1,)   # -1: one more than the MCU count
    for i, wc in enumerate(SIZE_CLASSES):
        for j, ri in enumerate(dris):
            hc = SIZE_CLASSES[(i + 2 * j + 1) % len(SIZE_CLASSES)]
            w, h = size_of(wc, 8 * m[0]), size_of(hc, 8 * m[1])
            if ri == -1:
                ri = ((w + 8 * m[0] - 1) // (8 * m[0])) * ((h + 8 * m[1] - 1) // (8 * m[1])) + 1
            out.append(Cell(layout, w, h, ri, bool((i + j) % 2), "q100" if (i + 3 * j) % 4 == 0 else "clean"))
    return out


def strip_cells(layout):
    """One MCU across and STRIP_MCUS rows of them (tall), one MCU row of STRIP_MCUS (wide): the long DRIs (4:2:2's
    dispatch edges), a DRI beyond the MCU count."""
    mw, mh = 8 * LAYOUTS[layout][0], 8 * LAYOUTS[layout][1]
    dris = (0, 1, 3) + EDGE_DRIS if layout == "422" else LAYOUT_STRIP_DRIS
    out = []
    for k, ri in enumerate(dris + (STRIP_MCUS + 1,)):
        std, content = bool(k % 2), ("clean", "q100")[k % 3 == 1]
        out.append(Cell(layout, mw, STRIP_MCUS * mh - k % 2, ri, std, content))
        out.append(Cell(layout, STRIP_MCUS * mw - (k + 1) % 2, mh, ri, not std, content))
    return out


def extreme_cells(layout):
    """EXTREME pixels on one axis, a few on the other (an MCU less a pixel, one pixel)."""
    mw, mh = 8 * LAYOUTS[layout][0], 8 * LAYOUTS[layout][1]
    return [Cell(layout, EXTREME, mh - 1, 5, False, "clean"), Cell(layout, 1, EXTREME, 0, True, "clean"),
            Cell(layout, EXTREME, 1, 1, True, "q100"), Cell(layout, mw - 1, EXTREME, 9, False, "clean")]


def rejected_frames():
    """EXTREME + 1 pixels on either axis: both parsers reject the frame."""
    return [(layout, w, h, synth.make_jpeg(w, h, seed=5, ri=4, sampling=s))
            for layout, s in LAYOUTS.items() for (w, h) in ((EXTREME + 1, 8), (8, EXTREME + 1))]


def cells(layout):
    return small_cells(layout) + strip_cells(layout) + extreme_cells(layout)
