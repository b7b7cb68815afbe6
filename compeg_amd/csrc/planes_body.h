// Lane body of the planes kernels (decode_planes_*_kernel, planes_kernels.hip): a decode that writes
// every component's 8-bit samples at the component's own resolution into memory of the caller's -- no colour step, no
// chroma upsampling.  No HIP dependency up to the wave function at the end: tests/emul_planes drives the same steps
// lane by lane.
//
// A lane per restart interval, coefficients through the lane's LDS slot, an MCU's samples in registers -- the layouts'
// kernels (kernels_body.h: decode_wave_fused_layout) up to the IDCT, with entropy_data_unit and idct_data_unit as they
// are.  What is written anew is the store stage: a lane stores its own MCU piece by piece, with ordinary stores the L2
// merges -- nothing goes through the quad, so a lane's stores depend on nothing but its own MCU's place.  The pieces
// ("runs") are a data unit row of 8 bytes, a 4:2:2 / 4:2:0 luma row of 16, an interleaved CbCr row of 16, a packed
// YUYV / UYVY row of 32.  An MCU that lies whole inside every plane it touches, in planes whose rows are aligned for
// the runs, is stored with one vector store a run; any other MCU byte by byte, every byte against the plane's extent.
#pragma once

#include "kernels_body.h"
#include "planes_types.h"

namespace compeg {

struct alignas(8) Vec2u {
    uint32_t x, y;
};

// Two words' bytes interleaved: [a0 b0 a1 b1] and [a2 b2 a3 b3].
CG_DEV uint32_t planes_mix_lo(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(b, a, 0x05010400u); // (selector bytes 0..3 pick from the second source, 4..7 from the first)
#else
    return (a & 0xffu) | (b & 0xffu) << 8 | (a & 0xff00u) << 8 | (b & 0xff00u) << 16;
#endif
}
CG_DEV uint32_t planes_mix_hi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(b, a, 0x07030602u);
#else
    return ((a >> 16) & 0xffu) | ((b >> 16) & 0xffu) << 8 | (a >> 24) << 16 | (b >> 24) << 24;
#endif
}
// Four bytes of (a + b + 1) >> 1 each.
CG_DEV uint32_t planes_avg(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_lerp(a, b, 0x01010101u);
#else
    return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu);
#endif
}

// HS x VS: the luma sampling; VS = 0: a grayscale image, one data unit an MCU and no chroma.
template <int HS, int VS>
struct PlanesMcu {
    static constexpr int kLuma = VS == 0 ? 1 : HS * VS, kDus = VS == 0 ? 1 : HS * VS + 2, kLumaRows = VS == 0 ? 1 : VS;
    uint32_t px[kDus][16]; // data unit k: row r's eight samples in words 2 r, 2 r + 1 (luma in raster order, Cb, Cr)
    uint32_t mx, my;
    bool active;  // the lane has an interval of its own: it stores
    bool aligned; // every plane's base and pitch take the vector stores
};

// Word j (0, 1) of row r of a data unit; r unrolled: a register, r a variable: selected without dynamic indexing.
CG_DEV uint32_t planes_row_word(const uint32_t (&px)[16], uint32_t r, int j)
{
    uint32_t w = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++)
        w = uint32_t(i) == r ? px[2 * i + j] : w;
    return w;
}

// One run of N words at byte xb of row y of plane pl.  FAST: the run lies inside the plane, aligned: vector stores.
template <int N, bool FAST>
CG_DEV void planes_store_run(const PlanesTarget &g, uint8_t *img, int pl, uint32_t xb, uint32_t y, const uint32_t (&w)[N])
{
    if (!FAST && (y >= g.rows[pl] || xb >= g.row_bytes[pl]))
        return;
    uint8_t *p = img + g.offset[pl] + uint64_t(y) * g.pitch[pl] + xb;
    if constexpr (FAST) {
        if constexpr (N == 2) {
            *CG_GLOBAL(Vec2u, reinterpret_cast<Vec2u *>(p)) = Vec2u{w[0], w[1]};
        } else {
#pragma unroll
            for (int i = 0; i < N / 4; i++)
                store_pixels<false>(p + 16 * i, Vec4u{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]});
        }
    } else {
        const uint32_t valid = umin(uint32_t(4 * N), g.row_bytes[pl] - xb);
        auto *q = CG_GLOBAL(uint8_t, p);
#pragma unroll
        for (int b = 0; b < 4 * N; b++)
            if (uint32_t(b) < valid)
                q[b] = uint8_t(w[b >> 2] >> (8 * (b & 3)));
    }
}

// Row r (0..7) of the lane's MCU into every plane it belongs to: the luma rows r of each row of luma data units, and
// chroma row r (CHROMA_420: rows 2 r and 2 r + 1 averaged, r below 4).  The format is wave-uniform.
template <int HS, int VS, bool FAST>
CG_DEV void planes_emit_row(const PlanesMcu<HS, VS> &t, const PlanesTarget &g, uint8_t *img, uint32_t r)
{
    using M = PlanesMcu<HS, VS>;
    if constexpr (HS == 2 && VS == 1) {
        if (g.format >= kPlanesYuyv) {
            // 16 pixels: [Y0 Cb Y1 Cr] (YUYV) or [Cb Y0 Cr Y1] (UYVY) per pair
            const uint32_t yw[4] = {planes_row_word(t.px[0], r, 0), planes_row_word(t.px[0], r, 1), planes_row_word(t.px[1], r, 0),
                                    planes_row_word(t.px[1], r, 1)};
            const uint32_t cb0 = planes_row_word(t.px[2], r, 0), cb1 = planes_row_word(t.px[2], r, 1);
            const uint32_t cr0 = planes_row_word(t.px[3], r, 0), cr1 = planes_row_word(t.px[3], r, 1);
            const uint32_t uv[4] = {planes_mix_lo(cb0, cr0), planes_mix_hi(cb0, cr0), planes_mix_lo(cb1, cr1), planes_mix_hi(cb1, cr1)};
            uint32_t w[8];
            const bool y_first = g.format == kPlanesYuyv;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t a = y_first ? yw[i] : uv[i], b = y_first ? uv[i] : yw[i];
                w[2 * i] = planes_mix_lo(a, b);
                w[2 * i + 1] = planes_mix_hi(a, b);
            }
            planes_store_run<8, FAST>(g, img, 0, t.mx * 32u, t.my * 8u + r, w);
            return;
        }
    }
#pragma unroll
    for (int v = 0; v < M::kLumaRows; v++) {
        uint32_t w[2 * HS];
#pragma unroll
        for (int h = 0; h < HS; h++) {
            w[2 * h] = planes_row_word(t.px[v * HS + h], r, 0);
            w[2 * h + 1] = planes_row_word(t.px[v * HS + h], r, 1);
        }
        planes_store_run<2 * HS, FAST>(g, img, 0, t.mx * (8u * HS), (t.my * uint32_t(M::kLumaRows) + uint32_t(v)) * 8u + r, w);
    }
    if constexpr (VS != 0) {
        const bool half = HS == 2 && VS == 1 && g.chroma420 != 0u;
        if (half && r >= 4u)
            return;
        uint32_t cb[2], cr[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (half) {
                cb[j] = planes_avg(planes_row_word(t.px[M::kLuma], 2u * r, j), planes_row_word(t.px[M::kLuma], 2u * r + 1u, j));
                cr[j] = planes_avg(planes_row_word(t.px[M::kLuma + 1], 2u * r, j), planes_row_word(t.px[M::kLuma + 1], 2u * r + 1u, j));
            } else {
                cb[j] = planes_row_word(t.px[M::kLuma], r, j);
                cr[j] = planes_row_word(t.px[M::kLuma + 1], r, j);
            }
        }
        const uint32_t y = t.my * (half ? 4u : 8u) + r;
        if (g.format == kPlanesSemiplanar) {
            const uint32_t w[4] = {planes_mix_lo(cb[0], cr[0]), planes_mix_hi(cb[0], cr[0]), planes_mix_lo(cb[1], cr[1]), planes_mix_hi(cb[1], cr[1])};
            planes_store_run<4, FAST>(g, img, 1, t.mx * 16u, y, w);
        } else {
            planes_store_run<2, FAST>(g, img, 1, t.mx * 8u, y, cb);
            planes_store_run<2, FAST>(g, img, 2, t.mx * 8u, y, cr);
        }
    }
}

// Whether the lane's MCU lies whole inside every plane it touches (its runs then need no cut).
template <int HS, int VS>
CG_DEV bool planes_mcu_whole(const PlanesMcu<HS, VS> &t, const PlanesTarget &g)
{
    using M = PlanesMcu<HS, VS>;
    const bool packed = HS == 2 && VS == 1 && g.format >= kPlanesYuyv;
    const uint32_t run0 = packed ? 32u : 8u * HS, rows0 = 8u * uint32_t(M::kLumaRows);
    bool whole = uint64_t(t.mx + 1u) * run0 <= g.row_bytes[0] && uint64_t(t.my + 1u) * rows0 <= g.rows[0];
    if (VS != 0 && !packed) {
        const bool half = HS == 2 && VS == 1 && g.chroma420 != 0u;
        const uint32_t run1 = g.format == kPlanesSemiplanar ? 16u : 8u, rows1 = half ? 4u : 8u;
        whole = whole && uint64_t(t.mx + 1u) * run1 <= g.row_bytes[1] && uint64_t(t.my + 1u) * rows1 <= g.rows[1];
    }
    return whole;
}

// ... and whether every plane's first byte and pitch are aligned for the vector stores of its runs: 8 bytes for runs of
// 8, 16 for the longer ones.  (img: the image's first byte.)
template <int HS, int VS>
CG_DEV bool planes_aligned(const PlanesTarget &g, const uint8_t *img)
{
    const bool packed = HS == 2 && VS == 1 && g.format >= kPlanesYuyv;
    const uint64_t base = reinterpret_cast<uint64_t>(img);
    const uint64_t a0 = (packed || HS == 2) ? 15u : 7u;
    bool ok = (((base + g.offset[0]) | g.pitch[0]) & a0) == 0u;
    if (VS != 0 && !packed) {
        const bool semi = g.format == kPlanesSemiplanar;
        ok = ok && (((base + g.offset[1]) | g.pitch[1]) & (semi ? 15u : 7u)) == 0u;
        if (!semi)
            ok = ok && (((base + g.offset[2]) | g.pitch[2]) & 7u) == 0u;
    }
    return ok;
}

template <int HS, int VS>
CG_DEV void planes_store_mcu(const PlanesMcu<HS, VS> &t, const PlanesTarget &g, uint8_t *img)
{
    if (!t.active)
        return;
    if (t.aligned && planes_mcu_whole<HS, VS>(t, g)) {
#pragma unroll
        for (int r = 0; r < 8; r++)
            planes_emit_row<HS, VS, true>(t, g, img, uint32_t(r));
    } else {
#pragma unroll 1
        for (uint32_t r = 0; r < 8u; r++)
            planes_emit_row<HS, VS, false>(t, g, img, r);
    }
}

template <int HS, int VS>
CG_DEV void planes_init(PlanesMcu<HS, VS> &t, const ImageDesc &d, const PlanesTarget &g, const uint8_t *img, uint32_t interval, bool active)
{
#pragma unroll
    for (int k = 0; k < PlanesMcu<HS, VS>::kDus; k++)
#pragma unroll
        for (int w = 0; w < 16; w++)
            t.px[k][w] = 0u;
    mcu_cursor_init(t, d, interval);
    t.active = active;
    t.aligned = planes_aligned<HS, VS>(g, img);
}

// One data unit: coefficients out of `slot` (cleared for reuse) and IDCT; k: its place in the MCU.  One copy of the IDCT
// in the instruction stream: it leaves its words in the last data unit, the others are moved (layout_transform).
template <int HS, int VS>
CG_DEV void planes_transform(PlanesMcu<HS, VS> &t, const ImageDesc &d, uint32_t comp, uint32_t k, uint8_t *slot, int32_t dc)
{
    constexpr int kDus = PlanesMcu<HS, VS>::kDus;
    uint32_t rec[kRetained / 2];
    take_slot(slot, rec);
    idct_data_unit(rec, dc, d.quant[comp], t.px[kDus - 1]);
#pragma unroll
    for (int j = 0; j < kDus - 1; j++) {
        if (k == uint32_t(j)) {
#pragma unroll
            for (int w = 0; w < 16; w++)
                t.px[j][w] = t.px[kDus - 1][w];
            CG_PLACE_MARK("; data unit in place");
        }
    }
}

// (the name the wave function and the emulation driver step by)
template <int HS, int VS>
CG_DEV void planes_next_mcu(PlanesMcu<HS, VS> &t, const ImageDesc &d)
{
    mcu_cursor_next(t, d);
}

#if defined(__HIPCC__)
// The whole path for 64 restart intervals, one per lane.  Lanes past the image's last interval decode that last interval
// once more and store nothing, as in the layouts' kernels: the wave's control flow stays one.
template <int HS, int VS>
CG_DEV void decode_wave_planes(const ImageDesc &d, const HuffShared &s, const PlanesTarget &g, uint8_t *img, uint32_t interval, uint32_t lane)
{
    constexpr uint32_t kDus = uint32_t(PlanesMcu<HS, VS>::kDus), kLuma = uint32_t(PlanesMcu<HS, VS>::kLuma);
    const bool active = interval < d.total_intervals;
    interval = active ? interval : d.total_intervals - 1u;
    uint8_t *slot = s.du_slots + lane * kDuSlotBytes;
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    PlanesMcu<HS, VS> t;
    planes_init<HS, VS>(t, d, g, img, interval, active);
    __builtin_amdgcn_s_setprio(CG_PRIO_ENTROPY);
    const uint32_t du_total = d.restart_interval * kDus;
    uint32_t k = 0; // the data unit's place inside its MCU (wave-uniform)
#pragma unroll 1
    for (uint32_t du = 0; du < du_total; du++) {
        const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
        const int32_t dc = entropy_data_unit(e, d, s, comp, slot16);
        __builtin_amdgcn_s_setprio(CG_PRIO_IDCT);
        planes_transform<HS, VS>(t, d, comp, k, slot, dc);
        if (k == kDus - 1u) {
            __builtin_amdgcn_s_setprio(CG_PRIO_COMPOSITE);
            planes_store_mcu<HS, VS>(t, g, img);
            planes_next_mcu<HS, VS>(t, d);
            k = 0;
        } else {
            k++;
        }
        __builtin_amdgcn_s_setprio(CG_PRIO_ENTROPY);
    }
}
#endif // __HIPCC__

} // namespace compeg
