// Per-lane body of the luma_tensor_* kernels (luma_kernels.hip): the oriented tensor output of orient_body.h with one
// channel a slot, the weighted sum of a source pixel's R, G and B (include/compeg_hip.h, "Luma tensor output").
//
// Written like orient_body.h and nhwc_body.h, whose records, axis tables, planners, grid, band walk, pad, conversions and
// stores it uses: what one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_luma
// compiles the very same code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and
// there is no LDS.
//
// Contract.  A source pixel (R, G, B, A) has L = (wR * R + wG * G + wB * B + 32768) >> 16 in unsigned
// 32-bit arithmetic, the weights 0 .. 65536 with a sum of 65536, so L <= 255 and R = G = B gives L = R whatever the
// weights.  The destination is [slots][1][oh][ow], tight.  Element (s, 0, y, x) is element (s, 0, y, x) of what
// orient_body.h stores in the order RGB with scale[0], bias[0] and the pad {p, p, p} if every source pixel's R were its
// L: the prefilter is P[j][i] = float(sum of L over the k x k block) * (1 / k^2), L per pixel before the block mean.
//
// Shape: orient_body.h's -- a lane owns column x' of T and a band of R rows -- with one sum a band row instead of three.
// What is new is the hot loop: luma_block forms L per pixel in integers (the weights are the launch's, in scalar
// registers, and masked to 24 bits so that a pixel takes three 24-bit multiply-adds) and returns the block's sum, at
// most 64 * 255; luma_row is the contract's x walk with one running sum, for k = 1 with four taps' loads in flight as in
// filter_row.
//   1..4: one element per lane and row at the mirrored column or row; a wave covers 64 neighbouring elements of a row.
//   5..8: the lane's R elements are a run along a row of U: orient_body.h's single-plane form.
// Register indices are constants throughout.
#pragma once

#include "orient_body.h"

namespace compeg {

// One launch: orient_body.h's (its records, tables and grid; dst is [slots][oh][ow]; of scale, bias and pad only element
// 0 is read, bgr is 0) and the weights.
struct LumaPack {
    FilterPack f;
    uint32_t weights[3]; // for R, G, B: each 0 .. 65536, their sum 65536
};

// L of one pixel, R in its low byte.  (Both factors of every product fit 24 bits.)
CG_DEV uint32_t luma_pixel(uint32_t v, uint32_t wr, uint32_t wg, uint32_t wb)
{
    uint32_t acc = (v & 0xffu) * wr + 32768u;
    acc = ((v >> 8) & 0xffu) * wg + acc;
    acc = ((v >> 16) & 0xffu) * wb + acc;
    return acc >> 16;
}

// The sum of L over the K x K pixels whose first one is at p.  Every load is one pixel, 4 bytes at an address that 4
// divides, as in resize_block (the compiler joins the loads of a block row).
template <uint32_t K>
CG_DEV uint32_t luma_block(const uint8_t *p, uint32_t pitch, uint32_t wr, uint32_t wg, uint32_t wb)
{
    uint32_t sum = 0u;
    for (uint32_t r = 0; r < K; r++, p += pitch) {
#pragma unroll
        for (uint32_t i = 0; i < K; i++)
            sum += luma_pixel(*CG_GLOBAL(const uint32_t, reinterpret_cast<const uint32_t *>(p + 4u * i)), wr, wg, wb);
    }
    return sum;
}

// One x tap into h: h = P * w for a row's first tap, h = h + (P * w) after it; antialias_tap's operations for one channel.
template <uint32_t K>
CG_DEV void luma_tap(float &h, uint32_t sum, float w, bool first)
{
    constexpr float kInv = 1.0f / float(K * K);
    const float p = float(sum) * kInv;
    const float q = p * w;
    const float next = h + q;
    h = first ? q : next;
}

// h(j) of one source row for one output column: filter_row with one running sum.
template <uint32_t K>
CG_DEV float luma_row(const uint8_t *p, uint32_t pitch, uint32_t count, const uint32_t *w, uint32_t stride, uint32_t wr, uint32_t wg,
                      uint32_t wb)
{
    float h = 0.0f;
    uint32_t tx = 0;
    for (; K == 1u && tx + 4u <= count; tx += 4u) {
        uint32_t px[4];
        float wt[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            wt[u] = antialias_weight(w + size_t(tx + u) * stride);
            px[u] = *CG_GLOBAL(const uint32_t, reinterpret_cast<const uint32_t *>(p + size_t(tx + u) * 4u));
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++)
            luma_tap<K>(h, luma_pixel(px[u], wr, wg, wb), wt[u], tx + u == 0u);
    }
    for (; tx < count; tx++) {
        const float wt = antialias_weight(w + size_t(tx) * stride);
        luma_tap<K>(h, luma_block<K>(p + size_t(tx) * K * 4u, pitch, wr, wg, wb), wt, tx == 0u);
    }
    return h;
}

// Lane `item` of slot `slot`: band item / tw, column item % tw of T.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void luma_tensor_lane(const LumaPack &n, uint32_t slot, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    const FilterPack &t = n.f;
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

    // ---- orient_body.h's walk with one sum a band row -----------------------------------------------------------------
    float m[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        m[r] = 0.0f;
    if (rows != 0u) {
        // (uniform, and no change to a checked weight: the products below are 24-bit ones)
        const uint32_t wr = n.weights[0] & 0xffffffu, wg = n.weights[1] & 0xffffffu, wb = n.weights[2] & 0xffffffu;
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
            const float h = luma_row<K>(origin + size_t(j) * K * im.pitch, im.pitch, xcount, wx, dw, wr, wg, wb);
#pragma unroll
            for (uint32_t r = 0; r < R; r++) {
                if (j >= from[r] && j < to[r]) {
                    const float w = antialias_weight(wy + size_t(j - from[r]) * dh + r);
                    const float q = h * w;
                    const float sum = m[r] + q;
                    m[r] = j == from[r] ? q : sum;
                }
            }
        }
    }

    // ---- the values, converted ---------------------------------------------------------------------------------------
    const float pad = filter_pad(t, 0u);
    uint32_t bits[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const float scaled = m[r] * t.scale[0];
        const float filtered = scaled + t.bias[0];
        const float val = r < rows ? filtered : pad;
        bits[r] = tensor_bits<DTYPE>(val);
    }

    // ---- the stores, through the orientation ------------------------------------------------------------------------
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
            uint8_t *p = t.dst + (size_t(slot) * plane + size_t(uy) * t.ow + ux) * kElem;
            tensor_store_run(p, TensorVec{{bits[r], 0u, 0u, 0u}}, kElem);
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
    uint32_t run[R];
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        run[r] = descending ? bits[R - 1u - r] : bits[r];
    orient_shift_down<R>(run, skip);
    uint8_t *p = t.dst + (size_t(slot) * plane + size_t(uy) * t.ow + ux) * kElem;
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

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_slot workgroups for every slot, one slot behind the
// other.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void luma_tensor_block_lane(const LumaPack &n, uint32_t block, uint32_t lane)
{
    const uint32_t slot = block / n.f.blocks_per_slot;
    luma_tensor_lane<DTYPE, K, R>(n, slot, (block - slot * n.f.blocks_per_slot) * kTensorThreads + lane);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

// Whether the kernels take these weights: each 0 .. 65536, their sum 65536, the reserved word 0.
inline bool luma_spec_ok(const compeg_luma_spec &luma)
{
    uint64_t sum = 0;
    for (int c = 0; c < 3; c++) {
        if (luma.weights[c] > 65536u)
            return false;
        sum += luma.weights[c];
    }
    return sum == 65536u && luma.reserved == 0u;
}

// The launch of one pack: plan_orient_pack's (the records are plan_orient_slots's, unchanged) with the weights.  pad: one
// value, or null for 0.  The order has no effect: R, G and B are at known places in the source.
inline bool plan_luma_pack(LumaPack &n, uint32_t &grid_blocks, uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter,
                           const compeg_luma_spec &luma, const float *pad, void *dst, uint32_t band, bool upright, bool transposed)
{
    n = LumaPack{};
    const float p = pad ? pad[0] : 0.0f, pads[3] = {p, p, p};
    if (!luma_spec_ok(luma) || !plan_orient_pack(n.f, grid_blocks, slots, spec, filter, pads, dst, band, upright, transposed))
        return false;
    n.f.bgr = 0u;
    for (int c = 0; c < 3; c++)
        n.weights[c] = luma.weights[c];
    return true;
}

} // namespace compeg
