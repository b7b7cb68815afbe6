"""What the levels decode (compeg_*_decode_levels: a file's quantised DCT coefficients as int16 blocks) must make of a
frame.  A plain module (Python and numpy, no fixtures), shared by tests/test_levels_stream.py (the layout, the oracle and
the mutants), tests/test_levels_emulation.py (the emulated lane body) and tests/gpu_levels_worker.py (the card).

The levels of a tests/coef_stream.py Frame are cs.predict of the same frame under quantisers of 1 with all 64 positions
retained: the entropy segment does not depend on the quantiser, so the "dequantised" values of that frame are the levels.
Position 0 is the 32-bit DC predictor there; the decode stores its low 16 bits.  The data units, in scan order, are then
scattered into one raster of blocks per component (whole MCUs), in zig-zag or in natural order.

Grayscale frames are tests/gray_stream.py's GrayFrame (a cs.Frame with one data unit an MCU and a one-component writer
made of cs's pieces): gray() makes them from 4:4:4 frames."""
import dataclasses

import numpy as np

import coef_stream as cs
import gray_stream as gs
import planes_stream as ps

ORDERS = ("zigzag", "natural")
MUTANTS = ("cut32", "zrl16", "natural_twice")


def gray(f444, **kw):
    """The one-component frame of a 4:4:4 frame's luma data units (gs.gray_of)."""
    return gs.gray_of(f444, **kw)


def shape(w, h, components=3, hs=2, vs=1):
    """compeg_levels_shape restated: ([offset, blocks_w, blocks_h, width_in_blocks, height_in_blocks] per component as
    dicts, total_bytes)."""
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    out, at = [], 0
    for c in range(components):
        hc, vc = (hs, vs) if c == 0 else (1, 1)
        cw, ch = -(-w * hc // hs), -(-h * vc // vs)
        out.append({"offset": at, "blocks_w": mw * hc, "blocks_h": mh * vc, "width_in_blocks": -(-cw // 8), "height_in_blocks": -(-ch // 8)})
        at += mw * hc * mh * vc * 128
    return tuple(out), at


def low16(v):
    """The low 16 bits of 32-bit values, as int16."""
    return (np.asarray(v).astype(np.int64) & 0xFFFF).astype(np.uint16).view(np.int16)


def frame_levels(f, mutant=None):
    """int16 [data units of the complete intervals, 64], zig-zag order, scan order.  mutant: "cut32" (quirk Q3 acting),
    "zrl16" (a ZRL advancing one position less or more than the frame's entropy mode says)."""
    g = dataclasses.replace(f, quant=(1, 1), _jpeg=None)
    kw = {"cut32": dict(retained=32), "zrl16": dict(zrl=17 if f.standard else 16)}.get(mutant, {})
    lv = cs.predict(g, **{"retained": 64, **kw}).astype(np.int64)
    assert np.abs(lv[:, 1:]).max(initial=0) <= 32767, "an AC level is 15 magnitude bits at the most"
    out = lv.astype(np.int16)
    out[:, 0] = low16(lv[:, 0])
    return out


def scan_words(ca, jpeg, **kw):
    """(words MSB-first, start positions, complete intervals) of a file as the library's front end and the oracle's scan
    preprocessing make them (ca: the package; no device is opened)."""
    from oracle import oracle as orc
    img = ca.ImageData(jpeg, **kw)
    off, n = img.scan_range()
    sb = orc.ScanBuffer()
    try:
        sb.process(jpeg[off:off + n], img.parallelism())
    except orc.OracleError:
        pass   # (a count mismatch leaves the truncated result in place, as in the reference)
    words = np.frombuffer(sb.processed_scan_data(), dtype=np.uint32).byteswap()
    starts = np.frombuffer(sb.start_positions(), dtype=np.uint32)
    return [int(w) for w in words], [int(x) for x in starts], int(np.frombuffer(img.metadata(), dtype=np.uint32)[272])


def reader_levels(f, words, starts, intervals):
    """frame_levels by the reference's reader alone (cs._Reader, the arithmetic cs.predict falls back to), over a
    preprocessed scan: for frames whose scan holds a segment more than their header counts ("/short" in the name), where
    what the preprocessing leaves is the oracle's to say."""
    dpm, comps = f.dus_per_mcu, f.comp_of_du
    by_code = {t: {v: k for k, v in cs.canonical(l)[2].items()} for t, l in f.huff.items()}
    zrl = 16 if f.standard else 17
    out = np.zeros((intervals * f.interval * dpm, 64), dtype=np.int64)
    for iv in range(intervals):
        pred, b = [0, 0, 0], cs._Reader(words, starts[iv])
        for du in range(iv * f.interval * dpm, (iv + 1) * f.interval * dpm):
            comp = comps[du % dpm]
            td, ta, _ = f.sel[comp]
            if f.standard:
                b.refill()
            size = b.symbol(by_code[2 * td])
            pred[comp] = cs.wrap32(pred[comp] + cs.extend(b.take(size), size))
            out[du, 0] = pred[comp]
            pos = 1
            while pos < 64:
                b.refill()
                rs = b.symbol(by_code[2 * ta + 1])
                if rs == 0:
                    break
                if rs == 0xF0:
                    pos += zrl
                    continue
                pos += rs >> 4
                if pos < 64:
                    out[du, pos] = cs.extend(b.take(rs & 15), rs & 15)
                else:
                    b.take(rs & 15)
                pos += 1
    res = out.astype(np.int16)
    res[:, 0] = low16(out[:, 0])
    return res


def any_frame_levels(f, ca=None):
    """frame_levels, or reader_levels over the oracle's preprocessed scan for a "/short" frame (ca: the package)."""
    if f.family == "sized" and "/short" in f.name:
        return reader_levels(f, *scan_words(ca, f.jpeg(), **f.image_kw()))
    return frame_levels(f)


def predictors(f):
    """The 32-bit DC predictors behind every data unit (what position 0 holds the low half of)."""
    return cs.predict(dataclasses.replace(f, quant=(1, 1), _jpeg=None), retained=1)[:, 0]


def ordered(levels, order, mutant=None):
    """[..., 64] zig-zag -> the order's: natural index v * 8 + u holds zig-zag position cs.ZIGZAG[v * 8 + u]."""
    if order == "zigzag":
        return levels
    out = levels[..., cs.ZIGZAG]
    return out[..., cs.ZIGZAG] if mutant == "natural_twice" else out


def rasters(units, mcus_w, mcus_h, components, hs, vs, fill=0):
    """[data units in scan order, 64] -> per component ([blocks_h, blocks_w, 64] with `fill` where no unit landed,
    [blocks_h, blocks_w] bool: a unit landed)."""
    dpm = 1 if components == 1 else hs * vs + 2
    luma = 1 if components == 1 else hs * vs
    n = np.arange(units.shape[0])
    m, k = n // dpm, n % dpm
    my, mx = m // mcus_w, m % mcus_w
    out = []
    for c in range(components):
        hc, vc = ((hs, vs) if components == 3 else (1, 1)) if c == 0 else (1, 1)
        sel = k < luma if c == 0 else k == luma + c - 1
        kk = np.where(sel, k, 0)
        by = my * vc + (kk // hc if c == 0 else 0)
        bx = mx * hc + (kk % hc if c == 0 else 0)
        grid = np.full((mcus_h * vc, mcus_w * hc, 64), fill, dtype=units.dtype)
        mask = np.zeros((mcus_h * vc, mcus_w * hc), dtype=bool)
        assert by[sel].max(initial=0) < mcus_h * vc
        grid[by[sel], bx[sel]] = units[sel]
        mask[by[sel], bx[sel]] = True
        out.append((grid, mask))
    return out


def destination(levels, mcus_w, mcus_h, components, hs, vs, order="zigzag", before=None, mutant=None):
    """One image's destination bytes: the components' rasters one after the other, int16 little endian; blocks no decoded
    unit landed in keep `before` (uint8 [total_bytes]; zeros without it)."""
    total = sum(g.size * 2 for g, _ in rasters(levels[:0], mcus_w, mcus_h, components, hs, vs))
    out = np.zeros(total, dtype=np.uint8) if before is None else np.array(before, dtype=np.uint8)
    assert out.size == total
    at = 0
    for grid, mask in rasters(ordered(levels, order, mutant), mcus_w, mcus_h, components, hs, vs):
        view = out[at:at + grid.size * 2].view(np.int16).reshape(grid.shape)
        view[mask] = grid[mask]
        at += grid.size * 2
    return out


def frame_geometry(f):
    """(mcus_w, mcus_h, components, hs, vs) of a frame, as destination() and shape() take them."""
    comps, hs, vs = ps.sampling_of(f)
    return f.mcus_w, f.mcus_h, comps, hs, vs


def frame_destination(f, order="zigzag", before=None, mutant=None):
    return destination(frame_levels(f, mutant if mutant != "natural_twice" else None), *frame_geometry(f), order=order, before=before,
                       mutant=mutant)


def views(buf, w, h, components, hs, vs):
    """A destination's bytes (uint8 [total_bytes]) -> per component int16 [blocks_h, blocks_w, 64]."""
    comps, total = shape(w, h, components, hs, vs)
    assert buf.size == total
    return [buf[c["offset"]:c["offset"] + c["blocks_w"] * c["blocks_h"] * 128].view(np.int16).reshape(c["blocks_h"], c["blocks_w"], 64) for c in comps]


def dequantised_low(blocks, q, order):
    """int16 [..., 64] levels in `order` x 64 factors in zig-zag order -> int32 [..., 32]: wrap32(level * q) at zig-zag
    positions 0..31, what the oracle's want_coefficients buffer holds."""
    inverse = np.argsort(cs.ZIGZAG) if order == "natural" else np.arange(64)   # zig-zag position -> index in `order`
    z = blocks[..., inverse[:32]].astype(np.int64) * np.asarray(q, dtype=np.int64)[:32]
    return (((z + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)).astype(np.int32)
