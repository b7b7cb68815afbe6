// Per-lane body of the orient_tensor_* kernels (orient_kernels.hip): the filtered tensor output of filter_body.h with an
// EXIF orientation (1..8) per slot (include/compeg_hip.h, "Oriented tensor output").
//
// Written like filter_body.h, whose launch record, row walk, pad, table layout, conversions and stores it uses: what one
// lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_orient compiles the very same
// code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and there is no LDS.
//
// Contract.  The slot T has the extent (tw, th) = (ow, oh) for the orientations 1..4 and (oh, ow) for
// 5..8, and is what filter_body.h stores for the slot's record (its inner rectangle dst' lies in T).  The slot written is
// U, ow x oh, every plane alike: element (y', x') of T is U's
//   1: (y', x')              2: (y', ow-1-x')            3: (oh-1-y', ow-1-x')      4: (oh-1-y', x')
//   5: (x', y')              6: (x', ow-1-y')            7: (oh-1-x', ow-1-y')      8: (oh-1-x', y')
//
// Shape: computed in T's coordinates -- a lane owns column x' of T and a band of R rows, bands counted from the inner
// rectangle's first row; the source walk, the R x 3 sums, the operations and their order are filter_body.h's, so the bits
// are its bits.  (Computing in U's coordinates would set the lanes of a wave a row pitch apart in the source, and the loads
// are where these kernels spend their time.)  Only the stores go through the orientation, which is the workgroup's:
//   1..4: one element per lane and row, as in filter_body.h, at the mirrored column or row; a wave still covers 64
//         neighbouring elements of a row of U.
//   5..8: the lane's R outputs are neighbours in one row of U, ascending (5, 8) or descending (6, 7) in x.  The lane puts
//         them into output order, cuts the run to the band's rows that belong to the slot (band 0 may begin above it, the
//         last one may end early; pad rows go out in the same run) and stores it with tensor_store_run, whose aligned
//         pieces take whatever alignment the row's address has.  The 64 lanes of a wave write into 64 rows.
// A call may mix orientations: the grid gives every slot the larger lane count that the call needs (bands(oh) * ow or
// bands(ow) * oh), and the lanes beyond a slot's own count return.  Register indices are constants throughout.
#pragma once

#include "filter_body.h"
#include "region_types.h"

namespace compeg {

// One slot of a launch: filter_body.h's record in T's coordinates, the orientation and T's extent.
struct alignas(8) OrientSlot {
    RegionAntialiasSlot rs;
    uint32_t orientation; // 1..8
    uint16_t tw, th;      // (ow, oh), or (oh, ow) for 5..8
};
static_assert(sizeof(OrientSlot) == 56, "the host writes these records as the kernels read them");
constexpr size_t kOrientSlotWords = sizeof(OrientSlot) / 4u;

// The launch is a FilterPack: `slots` OrientSlot records, ow x oh the upright slot, items_per_slot the larger lane count
// (above), bands_per_slot that count's bands.

// The record of the workgroup's slot: wave-uniform loads.
CG_DEV OrientSlot orient_slot(const void *slots, uint32_t slot)
{
    const OrientSlot *p = static_cast<const OrientSlot *>(slots) + slot;
    OrientSlot s;
#if defined(__HIP_DEVICE_COMPILE__)
    const auto *q = CG_GLOBAL(const uint64_t, reinterpret_cast<const uint64_t *>(p));
    const uint64_t w[7] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6]};
    __builtin_memcpy(&s, w, sizeof s);
#else
    memcpy(&s, p, sizeof s);
#endif
    return s;
}

// v[0 .. R-1] moved down by `by` (< R) places: v[i] = v[i + by] where that exists.  Constant indices: a stage per bit.
template <uint32_t R>
CG_DEV void orient_shift_down(uint32_t (&v)[R], uint32_t by)
{
#pragma unroll
    for (uint32_t step = 1u; step < R; step <<= 1) {
        const bool on = (by & step) != 0u;
#pragma unroll
        for (uint32_t i = 0; i < R; i++) {
            const uint32_t far = i + step < R ? v[i + step < R ? i + step : i] : 0u;
            v[i] = on ? far : v[i];
        }
    }
}

// Lane `item` of slot `slot`: band item / tw, column item % tw of T.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void orient_tensor_lane(const FilterPack &t, uint32_t slot, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    // (the slot is the workgroup's: these are wave-uniform loads)
    const OrientSlot os = orient_slot(t.slots, slot);
    const AntialiasImage &im = os.rs.im;
    const uint32_t tw = os.tw, th = os.th, o = os.orientation;
    const uint32_t lanes = ((th + R - 1u) / R + 1u) * tw; // the slot's own count
    if (item >= t.items_per_slot || item >= lanes)
        return;
    const uint32_t band = item / tw, x = item - band * tw;
    const uint32_t dx = os.rs.dx, dy = os.rs.dy, dw = os.rs.dw, dh = os.rs.dh;
    // Band `lead` begins at the rectangle's first row; band 0 begins `shift` rows above the slot.
    const uint32_t shift = (R - dy % R) % R, lead = (dy + shift) / R;
    const uint32_t yi0 = band >= lead ? (band - lead) * R : dh; // the band's first row, counted in the rectangle
    const bool inside = x >= dx && x - dx < dw && yi0 < dh;
    const uint32_t rows = !inside ? 0u : (dh - yi0 < R ? dh - yi0 : R); // band rows 0 .. rows - 1 are the rectangle's

    // ---- filter_body.h's lane, word for word, with T for the slot -------------------------------------------------
    float m[R][3]; // by source channel
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        m[r][0] = m[r][1] = m[r][2] = 0.0f;
    if (rows != 0u) {
        const uint32_t xi = x - dx;
        // (axis tables: first[o], count[o], then a row of o weights per t)
        const uint32_t *xtab = t.tables + im.xtab, *ytab = t.tables + im.ytab;
        const uint32_t xfirst = antialias_word(xtab + xi), xcount = antialias_word(xtab + dw + xi);
        const uint32_t *wx = xtab + 2u * size_t(dw) + xi, *wy = ytab + 2u * size_t(dh) + yi0;
        uint32_t from[R], to[R]; // band row r taps source rows from[r] .. to[r] - 1 (not the rectangle's: none)
        uint32_t jend = 0u;
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            from[r] = to[r] = 0u;
            if (r < rows) {
                from[r] = antialias_word(ytab + yi0 + r);
                to[r] = from[r] + antialias_word(ytab + dh + yi0 + r);
            }
            jend = to[r] > jend ? to[r] : jend;
        }
        const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + (size_t(im.cx) + size_t(xfirst) * K) * 4u;
        for (uint32_t j = from[0]; j < jend; j++) {
            float h[3] = {0.0f, 0.0f, 0.0f};
            filter_row<K>(h, origin + size_t(j) * K * im.pitch, im.pitch, xcount, wx, dw);
#pragma unroll
            for (uint32_t r = 0; r < R; r++) {
                if (j >= from[r] && j < to[r]) {
                    const float w = antialias_weight(wy + size_t(j - from[r]) * dh + r);
#pragma unroll
                    for (uint32_t ch = 0; ch < 3u; ch++) {
                        const float q = h[ch] * w;
                        const float sum = m[r][ch] + q;
                        m[r][ch] = j == from[r] ? q : sum;
                    }
                }
            }
        }
    }

    // ---- the stores, through the orientation ------------------------------------------------------------------------
    const float pad[3] = {filter_pad(t, 0u), filter_pad(t, 1u), filter_pad(t, 2u)};
    const size_t plane = size_t(t.oh) * t.ow;
    const uint32_t y0 = band * R - shift; // the band's first row in T (band 0: wraps where it begins above the slot)
    if (o < 5u) {
        const bool flip_x = o == 2u || o == 3u, flip_y = o == 3u || o == 4u;
        const uint32_t ux = flip_x ? t.ow - 1u - x : x;
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            const uint32_t y = y0 + r;
            if (y >= th)
                continue;
            const uint32_t uy = flip_y ? t.oh - 1u - y : y;
#pragma unroll
            for (uint32_t ch = 0; ch < 3u; ch++) {
                const uint32_t c = t.bgr ? 2u - ch : ch;
                // (constant indices: the launch's arguments stay in scalar registers)
                const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
                const float scaled = m[r][ch] * scale;
                const float filtered = scaled + bias;
                const float val = r < rows ? filtered : pad[ch];
                uint8_t *p = t.dst + ((size_t(slot) * 3u + c) * plane + size_t(uy) * t.ow + ux) * kElem;
                tensor_store_run(p, TensorVec{{tensor_bits<DTYPE>(val), 0u, 0u, 0u}}, kElem);
            }
        }
        return;
    }

    // Band rows r0 .. r1 - 1 are rows of T (th = ow: they are columns of U); the rest are nobody's.
    const uint32_t r0 = band == 0u ? shift : 0u;
    const uint32_t first = y0 + r0; // the row of T that band row r0 is (no wrap any more)
    if (first >= th)
        return; // (the last band of the grid may lie below T altogether)
    const uint32_t count = th - first < R - r0 ? th - first : R - r0;
    const uint32_t r1 = r0 + count;
    const bool descending = o == 6u || o == 7u;
    const uint32_t uy = o == 5u || o == 6u ? x : t.oh - 1u - x;
    // the run's first column in U, and how many places its first element lies from the front once in output order
    const uint32_t ux = descending ? t.ow - (y0 + r1) : y0 + r0;
    const uint32_t skip = descending ? R - r1 : r0;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const uint32_t c = t.bgr ? 2u - ch : ch;
        // (constant indices: the launch's arguments stay in scalar registers)
        const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
        uint32_t bits[R], run[R];
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            const float scaled = m[r][ch] * scale;
            const float filtered = scaled + bias;
            const float val = r < rows ? filtered : pad[ch];
            bits[r] = tensor_bits<DTYPE>(val);
        }
#pragma unroll
        for (uint32_t r = 0; r < R; r++)
            run[r] = descending ? bits[R - 1u - r] : bits[r];
        orient_shift_down<R>(run, skip);
        uint8_t *p = t.dst + ((size_t(slot) * 3u + c) * plane + size_t(uy) * t.ow + ux) * kElem;
        // 16 bytes a vector: R * kElem bytes are one of them (two for f32 at R = 8)
        constexpr uint32_t kPerVec = 16u / kElem, kVecs = (R + kPerVec - 1u) / kPerVec;
#pragma unroll
        for (uint32_t v = 0; v < kVecs; v++) {
            TensorVec out{{0u, 0u, 0u, 0u}};
#pragma unroll
            for (uint32_t e = 0; e < kPerVec; e++)
                if (v * kPerVec + e < R)
                    out.w[e * kElem / 4u] |= run[v * kPerVec + e] << (8u * (e * kElem % 4u));
            const uint32_t done = v * kPerVec, here = count > done ? (count - done < kPerVec ? count - done : kPerVec) : 0u;
            tensor_store_run(p + size_t(done) * kElem, out, here * kElem);
        }
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_slot workgroups for every slot, one slot behind the
// other.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void orient_tensor_block_lane(const FilterPack &t, uint32_t block, uint32_t lane)
{
    const uint32_t slot = block / t.blocks_per_slot;
    orient_tensor_lane<DTYPE, K, R>(t, slot, (block - slot * t.blocks_per_slot) * kTensorThreads + lane);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

// The records of a launch into the upright ow x oh and behind them its axis tables, like plan_filter_slots: a source's
// region.dst is dst', inside T.  False: what plan_filter_slots refuses, an orientation outside 1..8, or a dst' that
// leaves T.
inline bool plan_orient_slots(std::vector<uint32_t> &blob, size_t &tables_at, size_t &axes, const OrientSource *sources, uint32_t slots,
                              uint32_t k, uint32_t kernel, uint32_t ow, uint32_t oh)
{
    if (kernel >= kFilterKernels || k == 0u || ow == 0u || oh == 0u || ow > 65535u || oh > 65535u)
        return false;
    FilterTables tables(kernel, size_t(slots) * kOrientSlotWords);
    for (uint32_t i = 0; i < slots; i++) {
        const RegionSource &s = sources[i].region;
        const uint32_t o = sources[i].orientation;
        if (o < 1u || o > 8u)
            return false;
        const uint32_t tw = o < 5u ? ow : oh, th = o < 5u ? oh : ow;
        if (s.dst.width == 0u || s.dst.height == 0u || uint64_t(s.dst.x) + s.dst.width > tw || uint64_t(s.dst.y) + s.dst.height > th ||
            s.crop.width < k || s.crop.height < k)
            return false;
        OrientSlot r{};
        r.rs.im.src = static_cast<const uint8_t *>(s.src);
        r.rs.im.pitch = s.pitch;
        r.rs.im.cx = s.crop.x;
        r.rs.im.cy = s.crop.y;
        r.rs.im.pw = s.crop.width / k;
        r.rs.im.ph = s.crop.height / k;
        if (!filter_taps_ok(kernel, r.rs.im.pw, s.dst.width) || !filter_taps_ok(kernel, r.rs.im.ph, s.dst.height) ||
            !tables.axis(r.rs.im.pw, s.dst.width, r.rs.im.xtab) || !tables.axis(r.rs.im.ph, s.dst.height, r.rs.im.ytab))
            return false;
        r.rs.dx = uint16_t(s.dst.x);
        r.rs.dy = uint16_t(s.dst.y);
        r.rs.dw = uint16_t(s.dst.width);
        r.rs.dh = uint16_t(s.dst.height);
        r.orientation = o;
        r.tw = uint16_t(tw);
        r.th = uint16_t(th);
        memcpy(tables.words.data() + i * kOrientSlotWords, &r, sizeof r); // (after the tables grew)
    }
    tables_at = size_t(slots) * sizeof(OrientSlot);
    axes = tables.axes.size();
    blob.swap(tables.words);
    return true;
}

// The launch of one pack, like plan_filter_pack.  `upright`: some slot has an orientation in 1..4, `transposed`: some
// slot one in 5..8 (neither: as if upright); every slot gets the larger lane count that the call needs.
inline bool plan_orient_pack(FilterPack &t, uint32_t &grid_blocks, uint32_t slots, const compeg_tensor_spec &spec,
                             const compeg_filter_spec &filter, const float *pad, void *dst, uint32_t band, bool upright, bool transposed)
{
    // (the specs, and everything of t but the grid, with one slot's grid, which always fits)
    if (slots == 0u || !plan_filter_pack(t, grid_blocks, 1u, spec, filter, pad, dst, band))
        return false;
    // (65537 bands of 65535 columns at the most: a slot's lanes, the last workgroup's beyond it included, fit 32 bits;
    // the grid's workgroups must fit 31)
    const uint64_t bands_u = (uint64_t(t.oh) + band - 1u) / band + 1u, bands_t = (uint64_t(t.ow) + band - 1u) / band + 1u;
    const uint64_t items_u = bands_u * t.ow, items_t = bands_t * t.oh;
    const bool wider = transposed && (!upright || items_t > items_u);
    const uint64_t items = wider ? items_t : items_u;
    const uint64_t blocks = (items + kTensorThreads - 1u) / kTensorThreads;
    if (items > 0xffffffffull - kTensorThreads || blocks * slots > 0x7fffffffull)
        return false;
    t.bands_per_slot = uint32_t(wider ? bands_t : bands_u);
    t.items_per_slot = uint32_t(items);
    t.blocks_per_slot = uint32_t(blocks);
    grid_blocks = uint32_t(blocks * slots);
    return true;
}

} // namespace compeg
