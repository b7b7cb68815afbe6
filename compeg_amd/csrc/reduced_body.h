// Lane body of the reduced kernels (decode_reduced_*_kernel, reduced_kernels.hip): a decode at 1/8
// scale that writes one RGB pixel per luma data unit into memory of the caller's -- the entropy decode and nothing
// else of the transform.  No HIP dependency up to the wave function at the end: tests/emul_reduced drives the same
// steps lane by lane.
//
// A lane per restart interval, coefficients through the lane's LDS slot with entropy_data_unit as it is (the AC levels
// it leaves there are cleared, not read), one sample per data unit:
//
//     s = sample_u8((float(dc) * 0.125f) + 128.5f)
//
// -- what idct_data_unit leaves in all 64 samples of a data unit whose AC coefficients are zero (only in0 non-zero:
// both AAN passes hand it through, aan_scale(0)^2 * 0.125 = 0.125).  One f32 product, one f32 sum (this file is
// compiled with -ffp-contract=off like the IDCT), a clamp and a truncation; not restated in integers.  Per MCU the lane
// keeps HS * VS + 2 bytes (1 for grayscale); at the MCU's last unit come the colour step (ycbcr_to_rgba, chroma nearest
// neighbour) and the store: the lane's own HS x VS pixels, ordinary stores.
#pragma once

#include "kernels_body.h"
#include "reduced_types.h"

namespace compeg {

struct alignas(4) ReducedPair { // two RGBA pixels; the destination promises multiples of 4, no more
    uint32_t x, y;
};

// HS x VS: the luma sampling; VS = 0: a grayscale image, one data unit an MCU and no chroma.
template <int HS, int VS>
struct ReducedMcu {
    static constexpr int kLuma = VS == 0 ? 1 : HS * VS, kDus = VS == 0 ? 1 : HS * VS + 2, kRows = VS == 0 ? 1 : VS;
    uint32_t y;      // luma data unit k's sample in byte k (raster order)
    uint32_t cb, cr;
    uint32_t mx, my;
    bool active;     // the lane has an interval of its own: it stores
};

CG_DEV uint32_t reduced_sample(int32_t dc)
{
    return sample_u8((float(dc) * 0.125f) + 128.5f);
}

template <int HS, int VS>
CG_DEV void reduced_init(ReducedMcu<HS, VS> &t, const ImageDesc &d, uint32_t interval, bool active)
{
    t.y = 0u;
    t.cb = t.cr = 128u;
    mcu_cursor_init(t, d, interval);
    t.active = active;
}

// One data unit: its slot cleared for reuse (the levels are dropped), its sample kept; k: its place in the MCU
// (wave-uniform).
template <int HS, int VS>
CG_DEV void reduced_unit(ReducedMcu<HS, VS> &t, uint32_t k, uint8_t *slot, int32_t dc)
{
    constexpr uint32_t kLuma = uint32_t(ReducedMcu<HS, VS>::kLuma);
    zero_slot(slot);
    const uint32_t s = reduced_sample(dc);
    if (k < kLuma)
        t.y = (k == 0u ? 0u : t.y) | s << (8u * k);
    else if (k == kLuma)
        t.cb = s;
    else
        t.cr = s;
}

// The lane's MCU: HS x VS pixels at (mx HS, my VS), every one against the extent.  The format is wave-uniform.
template <int HS, int VS>
CG_DEV void reduced_store_mcu(const ReducedMcu<HS, VS> &t, const ReducedTarget &g, uint8_t *img)
{
    constexpr int kRows = ReducedMcu<HS, VS>::kRows;
    if (!t.active)
        return;
    const uint32_t x0 = t.mx * uint32_t(HS), y0 = t.my * uint32_t(kRows);
    uint32_t px[kRows][HS];
#pragma unroll
    for (int v = 0; v < kRows; v++)
#pragma unroll
        for (int h = 0; h < HS; h++) {
            const uint32_t s = (t.y >> (8 * (v * HS + h))) & 0xffu;
            px[v][h] = VS == 0 ? (s * 0x010101u | 0xff000000u) : ycbcr_to_rgba(s, t.cb, t.cr);
        }
    if (g.format == kReducedRgba) {
        const bool whole = x0 + uint32_t(HS) <= g.ow && y0 + uint32_t(kRows) <= g.oh;
#pragma unroll
        for (int v = 0; v < kRows; v++) {
            uint8_t *p = img + uint64_t(y0 + uint32_t(v)) * g.pitch + uint64_t(x0) * 4u;
            if (whole) {
                if constexpr (HS == 2)
                    *CG_GLOBAL(ReducedPair, reinterpret_cast<ReducedPair *>(p)) = ReducedPair{px[v][0], px[v][1]};
                else
                    *CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(p)) = px[v][0];
            } else {
#pragma unroll
                for (int h = 0; h < HS; h++)
                    if (x0 + uint32_t(h) < g.ow && y0 + uint32_t(v) < g.oh)
                        CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(p))[h] = px[v][h];
            }
        }
    } else {
        const uint64_t plane = uint64_t(g.ow) * g.oh;
        auto *q = CG_GLOBAL(uint8_t, img);
#pragma unroll
        for (int v = 0; v < kRows; v++)
#pragma unroll
            for (int h = 0; h < HS; h++) {
                if (x0 + uint32_t(h) >= g.ow || y0 + uint32_t(v) >= g.oh)
                    continue;
                const uint64_t at = uint64_t(y0 + uint32_t(v)) * g.ow + x0 + uint32_t(h);
#pragma unroll
                for (int c = 0; c < 3; c++)
                    q[uint64_t(c) * plane + at] = uint8_t(px[v][h] >> (8 * c));
            }
    }
}

// (the name the wave function and the emulation driver step by)
template <int HS, int VS>
CG_DEV void reduced_next_mcu(ReducedMcu<HS, VS> &t, const ImageDesc &d)
{
    mcu_cursor_next(t, d);
}

#if defined(__HIPCC__)
// The whole path for 64 restart intervals, one per lane.  Lanes past the image's last interval decode that last interval
// once more and store nothing, as in the planes kernels: the wave's control flow stays one.
template <int HS, int VS>
CG_DEV void decode_wave_reduced(const ImageDesc &d, const HuffShared &s, const ReducedTarget &g, uint8_t *img, uint32_t interval, uint32_t lane)
{
    constexpr uint32_t kDus = uint32_t(ReducedMcu<HS, VS>::kDus), kLuma = uint32_t(ReducedMcu<HS, VS>::kLuma);
    const bool active = interval < d.total_intervals;
    interval = active ? interval : d.total_intervals - 1u;
    uint8_t *slot = s.du_slots + lane * kDuSlotBytes;
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    ReducedMcu<HS, VS> t;
    reduced_init<HS, VS>(t, d, interval, active);
    const uint32_t du_total = d.restart_interval * kDus;
    uint32_t k = 0; // the data unit's place inside its MCU (wave-uniform)
#pragma unroll 1
    for (uint32_t du = 0; du < du_total; du++) {
        const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
        const int32_t dc = entropy_data_unit(e, d, s, comp, slot16);
        reduced_unit<HS, VS>(t, k, slot, dc);
        if (k == kDus - 1u) {
            reduced_store_mcu<HS, VS>(t, g, img);
            reduced_next_mcu<HS, VS>(t, d);
            k = 0;
        } else {
            k++;
        }
    }
}
#endif // __HIPCC__

} // namespace compeg
