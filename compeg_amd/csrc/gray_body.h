// Lane body of the fused grayscale kernels (decode_fused_gray_kernel, decode_fused_gray_single_kernel).
// No HIP dependency up to the wave functions at the end: tests/emul_gray drives the same steps lane by lane.
//
// A grayscale image (COMPEG_PARSE_GRAYSCALE) is its 4:4:4 twin without the chroma data units: one 8x8 data unit per
// MCU, every pixel R = G = B = the luma sample, A = 255.  The kernel is decode_wave_fused_layout<1, 1, MC>'s sibling --
// a lane per restart interval, coefficients through the lane's LDS slot, samples in registers, the composite through
// the lanes' quads -- with a third of its entropy work and a sixth of its sample registers: the colour step replicates
// a byte instead of converting with constant chroma.  It shares the 8-pixel-MCU layouts' row exchange and limits
// (kernels_body.h: layout_row_from_quad, pair_half_limit, target_limit); what is written anew here is what those
// have as functions of LayoutPixels<HS, VS, MC>, whose blocks count HS VS + 2 data units an MCU.
#pragma once

#include "kernels_body.h"

namespace compeg {

// MC: MCUs a lane holds before it composites them -- 1 (rows of 32 bytes), or 2 (rows of 64; restart intervals of two
// MCUs or more: a pair never straddles two intervals, the last MCU of an odd one is composited alone).
template <int MC>
struct GrayPixels {
    uint32_t px[MC][16]; // held MCU m: row r's eight samples in words 2 r, 2 r + 1
    uint32_t mx, my;     // the first held MCU
    bool active;
};

// Four pixels of four samples: R = G = B = the sample, A = 255.
CG_DEV Vec4u gray_quad(uint32_t yw)
{
    Vec4u o;
#if defined(__HIP_DEVICE_COMPILE__)
    // (selector bytes 0..3 pick from the second source, 0x0d = 0xff)
    o.x = __builtin_amdgcn_perm(0u, yw, 0x0d000000u);
    o.y = __builtin_amdgcn_perm(0u, yw, 0x0d010101u);
    o.z = __builtin_amdgcn_perm(0u, yw, 0x0d020202u);
    o.w = __builtin_amdgcn_perm(0u, yw, 0x0d030303u);
#else
    o.x = (yw & 0xffu) * 0x010101u | 0xff000000u;
    o.y = ((yw >> 8) & 0xffu) * 0x010101u | 0xff000000u;
    o.z = ((yw >> 16) & 0xffu) * 0x010101u | 0xff000000u;
    o.w = (yw >> 24) * 0x010101u | 0xff000000u;
#endif
    return o;
}

// Row `row` of the lane's MCU group into its slot: 2 MC pieces of 16 bytes.
template <int MC>
CG_DEV void gray_row_to_slot(const GrayPixels<MC> &t, int row, uint8_t *slot)
{
    SlotVec *p = reinterpret_cast<SlotVec *>(slot);
#pragma unroll
    for (int g = 0; g < 2 * MC; g++) {
        const Vec4u o = gray_quad(t.px[g >> 1][row * 2 + (g & 1)]);
        p[g] = SlotVec{o.x, o.y, o.z, o.w};
    }
}

// MCUs cut by the right / bottom edge of the output inside a 16-byte piece, or an unaligned pitch (composite_layout_edge's
// counterpart: neither arises with outputs the runtime allocates): the owning lane stores them pixel by pixel, each held
// MCU at its own place.
template <int MC>
CG_DEV void composite_gray_edge(const GrayPixels<MC> &t, const ImageDesc &d, uint32_t held = uint32_t(MC))
{
#pragma unroll 1
    for (uint32_t m = 0; m < held; m++) {
        uint32_t mx = t.mx + m, my = t.my;
        if (mx >= d.width_mcus) {
            mx -= d.width_mcus;
            my++;
        }
        const uint32_t x0 = mx * 8u, y0 = my * 8u;
        uint8_t *base = d.out + size_t(y0) * d.out_pitch + size_t(x0) * 4u;
#pragma unroll 1
        for (uint32_t w = 0; w < 16u; w++) { // (word w: row w / 2, pixels 4 (w & 1) .. + 3)
            const uint32_t row = w >> 1, x = x0 + (w & 1u) * 4u;
            if (y0 + row >= d.out_h)
                break;
            uint32_t yw = 0; // (the word selected without dynamic register indexing)
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
#pragma unroll
                for (uint32_t blk = 0; blk < uint32_t(MC); blk++)
                    yw = (i == w && blk == m) ? t.px[blk][i] : yw;
            }
            const Vec4u o = gray_quad(yw);
            auto *q = CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(base + size_t(row) * d.out_pitch + size_t(w & 1u) * 16u));
            if (x < d.out_w)
                q[0] = o.x;
            if (x + 1u < d.out_w)
                q[1] = o.y;
            if (x + 2u < d.out_w)
                q[2] = o.z;
            if (x + 3u < d.out_w)
                q[3] = o.w;
        }
    }
}

template <int MC>
CG_DEV void gray_init(GrayPixels<MC> &t, const ImageDesc &d, uint32_t interval, bool active)
{
#pragma unroll
    for (int k = 0; k < MC; k++)
#pragma unroll
        for (int w = 0; w < 16; w++)
            t.px[k][w] = 0u;
    mcu_cursor_init(t, d, interval);
    t.active = active;
}

// One data unit: coefficients out of `slot` (cleared for reuse) and IDCT; place: which held MCU it is.  One copy of the
// IDCT in the instruction stream: it leaves its words in the last block, a pair's first MCU is moved (layout_transform).
template <int MC>
CG_DEV void gray_transform(GrayPixels<MC> &t, const ImageDesc &d, uint32_t place, uint8_t *slot, int32_t dc)
{
    uint32_t rec[kRetained / 2];
    take_slot(slot, rec);
    idct_data_unit(rec, dc, d.quant[0], t.px[MC - 1]);
#pragma unroll
    for (int j = 0; j < MC - 1; j++) {
        if (place == uint32_t(j)) {
#pragma unroll
            for (int w = 0; w < 16; w++)
                t.px[j][w] = t.px[MC - 1][w];
            CG_PLACE_MARK("; data unit in place");
        }
    }
}

template <int MC>
CG_DEV McuTarget gray_target(const GrayPixels<MC> &t, const ImageDesc &d)
{
    const uint32_t x0 = t.mx * 8u, y0 = t.my * 8u;
    McuTarget g;
    g.base = d.out + size_t(y0) * d.out_pitch + size_t(x0) * 4u;
    // (all held MCUs in one MCU row, inside what is allocated: layout_target)
    g.whole = t.active && t.mx + uint32_t(MC) <= d.width_mcus && x0 + 8u * MC <= umax(d.out_w, d.out_pitch / 4u) &&
              y0 + 8u <= umax(d.out_h, d.out_alloc_h) && (d.out_pitch & 15u) == 0u && x0 < d.out_w && y0 < d.out_h;
    return g;
}

template <int MC>
CG_DEV uint32_t gray_limit(const GrayPixels<MC> &t, const ImageDesc &d)
{
    return target_limit(d, t.active && t.mx + uint32_t(MC) <= d.width_mcus, t.mx * 8u, t.my * 8u, 8u * MC, 8u);
}

// pair_limits for a pair of grayscale MCUs -- bits 0-7: the limit of the pair's first MCU, 8-15: of its second, or kPairEdge.
CG_DEV uint32_t gray_pair_limits(const GrayPixels<2> &t, const ImageDesc &d, bool whole, bool alone = false)
{
    const uint32_t full = 8u | 2u << 5;
    if (alone)
        return t.active ? pair_half_limit<1>(d, t.mx * 8u, t.my * 8u) : 0u;
    if (whole)
        return full | full << 8;
    if (!t.active)
        return 0u;
    if (t.mx + 2u <= d.width_mcus) {
        const uint32_t lim = gray_limit<2>(t, d);
        if (!lim)
            return kPairEdge;
        const uint32_t rows = lim & 31u, pieces = lim >> 5;
        return (rows | umin(pieces, 2u) << 5) | (pieces > 2u ? (rows | (pieces - 2u) << 5) << 8 : 0u);
    }
    // (the second MCU begins the next MCU row; an image one MCU across: every pair is two MCU rows)
    const uint32_t a = pair_half_limit<1>(d, t.mx * 8u, t.my * 8u), b = pair_half_limit<1>(d, 0u, (t.my + 1u) * 8u);
    return (a | b) & kPairEdge ? kPairEdge : a | b << 8;
}

// How far behind its place in the pair's row the second MCU lies (bytes; 0 in one MCU row with the first)
CG_DEV uint32_t gray_pair_second_offset(const GrayPixels<2> &t, const ImageDesc &d)
{
    return t.active && t.mx + 2u > d.width_mcus ? 8u * d.out_pitch - t.mx * 32u - 32u : 0u;
}

// The lane's group is the edge path's: nothing of it went through the quad.
template <int MC>
CG_DEV bool gray_is_edge(const GrayPixels<MC> &t, const ImageDesc &d, bool whole, bool alone = false)
{
    if (!t.active || (whole && !alone))
        return false;
    if constexpr (MC == 2)
        return gray_pair_limits(t, d, false, alone) == kPairEdge;
    else
        return gray_limit<MC>(t, d) == 0u;
}

template <int MC>
CG_DEV void gray_next_group(GrayPixels<MC> &t, const ImageDesc &d)
{
    t.mx += uint32_t(MC);
#pragma unroll
    for (int m = 0; m < MC; m++) { // (an image one MCU across: a pair is two MCU rows)
        if (t.mx >= d.width_mcus) {
            t.mx -= d.width_mcus;
            t.my++;
        }
    }
}

#if defined(__HIPCC__)
// The composite of the wave's 64 current MCU groups through the lanes' quads (composite_layout_mcus's counterpart).
// alone (wave-uniform; pairs): the groups' first MCUs are all there is -- the last MCU of an odd restart interval.
template <int MC>
CG_DEV void composite_gray_mcus(GrayPixels<MC> &t, const ImageDesc &d, uint8_t *wave_slots, uint32_t lane, bool alone = false)
{
    const McuTarget g = gray_target<MC>(t, d);
    const uint64_t addr = reinterpret_cast<uint64_t>(g.base);
    const uint32_t lo = uint32_t(addr), hi = uint32_t(addr >> 32), wh = g.whole ? 1u : 0u;
    uint8_t *bases[4] = {
        reinterpret_cast<uint8_t *>(uint64_t(quad_lane<0>(hi)) << 32 | quad_lane<0>(lo)),
        reinterpret_cast<uint8_t *>(uint64_t(quad_lane<1>(hi)) << 32 | quad_lane<1>(lo)),
        reinterpret_cast<uint8_t *>(uint64_t(quad_lane<2>(hi)) << 32 | quad_lane<2>(lo)),
        reinterpret_cast<uint8_t *>(uint64_t(quad_lane<3>(hi)) << 32 | quad_lane<3>(lo)),
    };
    const uint32_t whole_mask = quad_lane<0>(wh) | quad_lane<1>(wh) << 1 | quad_lane<2>(wh) << 2 | quad_lane<3>(wh) << 3;
    uint8_t *slot = wave_slots + lane * kDuSlotBytes;
    // (pairs, an odd number of MCUs a row or an interval: some pairs lie across two 64-byte segments -- layout_store)
    const bool across = MC == 2 && ((d.width_mcus | d.restart_interval) & 1u) != 0u;
    if (!alone && __builtin_amdgcn_ballot_w64(whole_mask != 0xfu) == 0u) {
#pragma unroll
        for (int row = 0; row < 8; row++) {
            gray_row_to_slot<MC>(t, row, slot);
            if (across)
                layout_row_from_quad<2 * MC, true>(d, wave_slots, lane, uint32_t(row), bases, 0xfu);
            else
                layout_row_from_quad<2 * MC, 2 * MC != 4>(d, wave_slots, lane, uint32_t(row), bases, 0xfu);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else if constexpr (MC == 2) {
        // (some pair is cut, outside, alone, or has its second MCU at the next MCU row's beginning: each half its own limit,
        // the second its own place; second halves without a limit store nothing)
        const uint32_t lim = gray_pair_limits(t, d, g.whole, alone), off = gray_pair_second_offset(t, d);
        const uint32_t lims[4] = {quad_lane<0>(lim), quad_lane<1>(lim), quad_lane<2>(lim), quad_lane<3>(lim)};
        const uint32_t limits = pair_rows_for_lane(lims, lane & 3u);
        // (the exchange by every lane, then masked: composite_layout_mcus)
        const uint32_t second = 0u - ((lane >> 1) & 1u);
        uint8_t *moved[4] = {bases[0] + (quad_lane<0>(off) & second), bases[1] + (quad_lane<1>(off) & second),
                             bases[2] + (quad_lane<2>(off) & second), bases[3] + (quad_lane<3>(off) & second)};
#pragma unroll
        for (int row = 0; row < 8; row++) {
            gray_row_to_slot<MC>(t, row, slot);
            layout_row_from_quad_cut<2 * MC>(d, wave_slots, lane, uint32_t(row), moved, limits);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // (some MCU of the wave is cut by the output's edge, or outside: what lies inside in whole pieces the same way)
        const uint32_t lim = g.whole ? 8u | uint32_t(2 * MC) << 5 : gray_limit<MC>(t, d);
        const uint32_t limits = cut_rows_for_piece(quad_lane<0>(lim) | quad_lane<1>(lim) << 8 | quad_lane<2>(lim) << 16 | quad_lane<3>(lim) << 24,
                                                   lane & 1u);
#pragma unroll
        for (int row = 0; row < 8; row++) {
            gray_row_to_slot<MC>(t, row, slot);
            layout_row_from_quad_cut<2 * MC>(d, wave_slots, lane, uint32_t(row), bases, limits);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    zero_slot(slot);
    if (gray_is_edge<MC>(t, d, g.whole, alone))
        composite_gray_edge<MC>(t, d, alone ? 1u : uint32_t(MC));
    gray_next_group<MC>(t, d);
}

// The whole path for 64 restart intervals, one per lane (decode_wave_fused_layout's counterpart).  Lanes past the image's
// last interval decode that last interval once more and never store an MCU of their own: they stay for their quad's
// exchange.  MC = 2: pairs by the MCU's place in its interval; the last MCU of an odd interval is composited alone.
template <int MC>
CG_DEV void decode_wave_fused_gray(const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane)
{
    const bool active = interval < d.total_intervals;
    interval = active ? interval : d.total_intervals - 1u;
    uint8_t *slot = s.du_slots + lane * kDuSlotBytes;
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    GrayPixels<MC> t;
    gray_init<MC>(t, d, interval, active);
    __builtin_amdgcn_s_setprio(CG_PRIO_ENTROPY);
    const uint32_t mcus = d.restart_interval;
    uint32_t place = 0; // the MCU's place among the held ones (wave-uniform)
#pragma unroll 1
    for (uint32_t mcu = 0; mcu < mcus; mcu++) {
        const int32_t dc = entropy_data_unit(e, d, s, 0u, slot16);
        __builtin_amdgcn_s_setprio(CG_PRIO_IDCT);
        gray_transform<MC>(t, d, place, slot, dc);
        const bool alone = MC == 2 && mcu + 1u == mcus && place != uint32_t(MC - 1); // (pairs, an odd restart interval: its last MCU alone)
        if (place == uint32_t(MC - 1) || alone) {
            __builtin_amdgcn_s_setprio(CG_PRIO_COMPOSITE);
            composite_gray_mcus<MC>(t, d, s.du_slots, lane, alone);
            place = 0;
        } else {
            place++;
        }
        __builtin_amdgcn_s_setprio(CG_PRIO_ENTROPY);
    }
}
#endif // __HIPCC__

} // namespace compeg
