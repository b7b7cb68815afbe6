// Per-lane body of the nhwc_tensor_* kernels (nhwc_kernels.hip): the oriented tensor output of orient_body.h into a
// channels-last destination of 3 or 4 channels (include/compeg_hip.h, "Channels-last tensor output").
//
// Written like orient_body.h, whose records, axis tables, planners, grid, row walk, pad, conversions and stores it uses:
// what one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_nhwc compiles the very
// same code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and there is no LDS.
//
// Contract.  The destination is [slots][oh][ow][C], tight, C = 3 or 4.  Element (s, y, x, c), c < 3, is
// element (s, c, y, x) of what orient_body.h stores for the same launch; for C = 4 element 3 of every pixel, the pad's
// pixels included, is `fill` converted to the element type, with neither scale nor bias.
//
// Shape: orient_body.h's -- a lane owns column x' of T and a band of R rows, the source walk, the R x 3 sums, the
// operations and their order restated from it (as it restates filter_body.h), so the bits are its bits.  Only the stores
// differ: the channel values of a pixel are neighbours in memory.
//   1..4: per band row the lane puts its pixel's C values into one vector in channel order and stores C elements with
//         one tensor_store_run (C = 4 at an aligned address: one store); a wave covers 64 neighbouring pixels of a row
//         of U, 64 * C elements in a piece.
//   5..8: the lane's R pixels are neighbours in one row of U.  It puts the pixels into output order channel by channel
//         (reversed where they descend, the run's first pixel moved to the front with orient_shift_down), interleaves
//         them into R * C elements and stores count * C of them in 16-byte vectors through tensor_store_run; pad rows of
//         the band go out in the same run, the fill with its pixel.
// `channels` is the launch's: a wave-uniform branch around the two interleavings.  Register indices are constants
// throughout.
#pragma once

#include <cmath>

#include "orient_body.h"

namespace compeg {

// One launch: orient_body.h's (its records, tables and grid; there is no plane, dst is [slots][oh][ow][channels]) and
// what the layout adds.
struct NhwcPack {
    FilterPack f;
    uint32_t channels; // 3 or 4
    float fill;        // channels == 4: element 3 of every pixel, converted like any value
};

// The elements first .. first + count * C - 1 of a run of R pixels of C channels, ch[c][i] the bits of channel c of
// pixel i, to p: 16-byte vectors, each cut to what the run still holds.
template <uint32_t DTYPE, uint32_t R, uint32_t C>
CG_DEV void nhwc_store_pixels(uint8_t *p, const uint32_t (&ch)[4][R], uint32_t count)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    constexpr uint32_t kPerVec = 16u / kElem, kVecs = (R * C + kPerVec - 1u) / kPerVec;
    const uint32_t bytes = count * C * kElem;
#pragma unroll
    for (uint32_t v = 0; v < kVecs; v++) {
        TensorVec out{{0u, 0u, 0u, 0u}};
#pragma unroll
        for (uint32_t e = 0; e < kPerVec; e++) {
            const uint32_t at = v * kPerVec + e; // element `at` of the run: channel at % C of pixel at / C
            if (at < R * C)
                out.w[e * kElem / 4u] |= ch[at % C][at / C] << (8u * (e * kElem % 4u));
        }
        const uint32_t done = v * 16u, here = bytes > done ? (bytes - done < 16u ? bytes - done : 16u) : 0u;
        tensor_store_run(p + done, out, here);
    }
}

// Lane `item` of slot `slot`: band item / tw, column item % tw of T.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void nhwc_tensor_lane(const NhwcPack &n, uint32_t slot, uint32_t item)
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

    // ---- orient_body.h's lane (filter_body.h's), word for word -----------------------------------------------------
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

    // ---- the values, converted: bits[c][r] is destination channel c of band row r ----------------------------------
    const float pad[3] = {filter_pad(t, 0u), filter_pad(t, 1u), filter_pad(t, 2u)};
    const uint32_t fill = tensor_bits<DTYPE>(n.fill);
    uint32_t bits[3][R];
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        // (constant indices: the launch's arguments stay in scalar registers)
        const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            const float scaled = m[r][ch] * scale;
            const float filtered = scaled + bias;
            const float val = r < rows ? filtered : pad[ch];
            bits[ch][r] = tensor_bits<DTYPE>(val);
        }
    }
    // (source channel ch goes to destination channel 2 - ch under bgr: a uniform exchange of two registers a row)
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t a = bits[0][r], b = bits[2][r];
        bits[0][r] = t.bgr ? b : a;
        bits[2][r] = t.bgr ? a : b;
    }

    // ---- the stores, through the orientation ------------------------------------------------------------------------
    const size_t pixel = size_t(n.channels) * kElem;
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
            const uint32_t e[4] = {bits[0][r], bits[1][r], bits[2][r], fill};
            TensorVec out{{0u, 0u, 0u, 0u}};
#pragma unroll
            for (uint32_t c = 0; c < 4u; c++)
                out.w[c * kElem / 4u] |= e[c] << (8u * (c * kElem % 4u));
            uint8_t *p = t.dst + ((size_t(slot) * t.oh + uy) * t.ow + ux) * pixel;
            tensor_store_run(p, out, uint32_t(pixel)); // (the first three elements, or all four)
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
    // the run's first column in U, and how many places its first pixel lies from the front once in output order
    const uint32_t ux = descending ? t.ow - (y0 + r1) : y0 + r0;
    const uint32_t skip = descending ? R - r1 : r0;
    uint32_t run[4][R];
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
#pragma unroll
        for (uint32_t r = 0; r < R; r++)
            run[c][r] = descending ? bits[c][R - 1u - r] : bits[c][r];
        orient_shift_down<R>(run[c], skip);
    }
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        run[3][r] = fill;
    uint8_t *p = t.dst + ((size_t(slot) * t.oh + uy) * t.ow + ux) * pixel;
    if (n.channels == 3u)
        nhwc_store_pixels<DTYPE, R, 3>(p, run, count);
    else
        nhwc_store_pixels<DTYPE, R, 4>(p, run, count);
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_slot workgroups for every slot, one slot behind the
// other.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void nhwc_tensor_block_lane(const NhwcPack &n, uint32_t block, uint32_t lane)
{
    const uint32_t slot = block / n.f.blocks_per_slot;
    nhwc_tensor_lane<DTYPE, K, R>(n, slot, (block - slot * n.f.blocks_per_slot) * kTensorThreads + lane);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

// Whether the kernels take this layout: 3 or 4 channels, a finite fill, reserved words of 0.
inline bool nhwc_spec_ok(const compeg_nhwc_spec &nhwc)
{
    return (nhwc.channels == 3u || nhwc.channels == 4u) && std::isfinite(nhwc.fill) && nhwc.reserved[0] == 0u && nhwc.reserved[1] == 0u;
}

// The launch of one pack: plan_orient_pack's (the records are plan_orient_slots's, unchanged) with the layout.
inline bool plan_nhwc_pack(NhwcPack &n, uint32_t &grid_blocks, uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter,
                           const compeg_nhwc_spec &nhwc, const float *pad, void *dst, uint32_t band, bool upright, bool transposed)
{
    n = NhwcPack{};
    if (!nhwc_spec_ok(nhwc) || !plan_orient_pack(n.f, grid_blocks, slots, spec, filter, pad, dst, band, upright, transposed))
        return false;
    n.channels = nhwc.channels;
    n.fill = nhwc.fill;
    return true;
}

} // namespace compeg
