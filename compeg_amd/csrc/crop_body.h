// Lane body of the cropped kernels (decode_cropped_*_kernel, crop_kernels.hip): a decode of one
// rectangle of the image into memory of the caller's -- pixel for pixel what the RGBA decode has there -- in which a
// restart interval that has no MCU inside the rectangle is not read at all.  No HIP dependency, the wave function at the
// end included: tests/emul_crop calls it lane by lane.
//
// A lane per restart interval, coefficients through the lane's LDS slot, an MCU's samples in registers -- the planes
// kernels (planes_body.h) up to the IDCT, with entropy_data_unit and idct_data_unit as they are.  What is new:
//   - the touch test (crop_reach): how far a run of MCUs in raster order reaches into the rectangle's box of MCUs.  A
//     workgroup asks it of all its intervals together, a wave of its 64, a lane of its own; 0 means "not touched".
//   - a touched lane walks its interval from the start, since every MCU's position in the stream comes from the ones
//     before it, up to its last MCU inside the box and no further; an MCU outside the box has its slots cleared and
//     nothing else done to it.
//   - the store stage: row by row of the MCU, the pixels inside the rectangle -- the colour step per pixel
//     (ycbcr_to_rgba, chroma nearest neighbour), four pixels as one 16-byte store where all four are inside and the
//     address allows it, else 4-byte stores (RGBA) or bytes (planar).
#pragma once

#include "crop_types.h"
#include "kernels_body.h"

namespace compeg {

// MCUs a .. b - 1 of an image wm MCUs wide, in raster order, against the box of MCU columns mx0 .. mx1 - 1 and MCU rows
// my0 .. my1 - 1 (non-empty, inside the image): 0 when none of them lies in the box, else the count of MCUs from a up to
// and with the last one that does -- what a walk from a has to cover.  Right for runs that wrap over the end of an MCU
// row, that span several rows, and for the one run of a file without DRI.
CG_DEV uint32_t crop_reach(uint32_t a, uint32_t b, uint32_t wm, uint32_t mx0, uint32_t mx1, uint32_t my0, uint32_t my1)
{
    const uint32_t lo = umax(a, my0 * wm), hi = umin(b, my1 * wm); // the run inside the box's rows
    if (lo >= hi)
        return 0u;
    // the first MCU at or behind lo in the box's columns: in lo's row, or at mx0 of the row below
    const uint32_t c = lo % wm;
    const uint32_t first = c < mx0 ? lo + (mx0 - c) : (c < mx1 ? lo : lo + (wm - c) + mx0);
    if (first >= hi)
        return 0u;
    // the last one before hi: in that row, or at mx1 - 1 of the row above (which `first` says there is)
    const uint32_t m = hi - 1u, e = m % wm;
    const uint32_t last = e >= mx1 ? m - (e - (mx1 - 1u)) : (e >= mx0 ? m : m - e - (wm - mx1) - 1u);
    return last + 1u - a;
}

// `count` restart intervals from `first` on: interval k holds MCUs k DRI .. k DRI + DRI - 1, cut at the image's MCUs.
CG_DEV uint32_t crop_intervals_reach(const ImageDesc &d, const CropTarget &g, uint32_t first, uint32_t count)
{
    const uint64_t end = (uint64_t(first) + count) * d.restart_interval;
    const uint32_t b = end < d.total_mcus ? uint32_t(end) : d.total_mcus;
    return crop_reach(first * d.restart_interval, b, d.width_mcus, g.mx0, g.mx1, g.my0, g.my1);
}

// A wave-uniform value in a vector register of the lane's own (an identity move the compiler takes for a lane-to-lane
// one).  The entropy decode and the IDCT leave these kernels no scalar register to spare, and of vector registers
// there are some: what the store stage needs of the target goes there (CropEdges), and nothing of the kernels' scalar
// state is put aside in vector lanes (no scalar spills: tests/test_crop_code_objects.py).
CG_DEV uint32_t crop_lane_own(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0xe4, 0xf, 0xf, true)); // (quad_perm 0 1 2 3: every lane its own)
#else
    return v;
#endif
}

// What the rectangle's pixels are laid into: bytes from row to row (planar: the rows' width) and, planar, the bytes from
// plane to plane.  A destination that holds the rectangle alone has the rectangle's own (CropOwnSlot: the one-rectangle
// decode); a region of a list lies in a slot that is larger than it (crop_regions_body.h).  The wave function is handed
// the maker, not the values, and asks it where it fills CropEdges: the one-rectangle kernels then compute the plane where
// they always have, behind the entropy decode's set-up, and hold no scalar register for it before.
struct CropSlot {
    uint32_t pitch;
    uint64_t plane;
};
struct CropOwnSlot {};
CG_DEV CropSlot crop_slot(const CropOwnSlot &, const CropTarget &g)
{
    return CropSlot{g.pitch, uint64_t(g.width) * g.height};
}

// The rectangle's edges in pixels of the image, x0 <= X < x1 and y0 <= Y < y1, the destination's pitch and the bytes of
// one of its planes: the lane's copy (crop_lane_own).
struct CropEdges {
    uint32_t x0, x1, y0, y1, pitch;
    uint32_t plane_lo, plane_hi; // (planar: the bytes from plane to plane -- CropSlot's)
    uint8_t *img;                // the rectangle's first byte in the destination
    uint32_t width_mcus;         // (ImageDesc's)
};

// (img: where this image's rectangle begins; slot: what it is laid into)
CG_DEV CropEdges crop_edges(const ImageDesc &d, const CropTarget &g, const CropSlot &slot, uint8_t *img)
{
    const uint64_t plane = slot.plane, at = reinterpret_cast<uintptr_t>(img);
    const uint64_t own = uint64_t(crop_lane_own(uint32_t(at >> 32))) << 32 | crop_lane_own(uint32_t(at));
    return CropEdges{crop_lane_own(g.x), crop_lane_own(g.x + g.width), crop_lane_own(g.y), crop_lane_own(g.y + g.height), crop_lane_own(slot.pitch),
                     crop_lane_own(uint32_t(plane)), crop_lane_own(uint32_t(plane >> 32)), reinterpret_cast<uint8_t *>(uintptr_t(own)), crop_lane_own(d.width_mcus)};
}

// HS x VS: the luma sampling; VS = 0: a grayscale image, one data unit an MCU and no chroma.
// The MCU's place and whether it lies in the box share one word: beside an MCU's samples the IDCT leaves a lane of the
// 4:2:2 kernel no register to spare at three waves a SIMD (an image has at most 8192 MCUs either way: 13 bits).
template <int HS, int VS>
struct CropMcu {
    static constexpr int kLuma = VS == 0 ? 1 : HS * VS, kDus = VS == 0 ? 1 : HS * VS + 2, kLumaRows = VS == 0 ? 1 : VS;
    uint32_t px[kDus][16]; // data unit k: row r's eight samples in words 2 r, 2 r + 1 (luma in raster order, Cb, Cr)
    uint32_t at;           // mx | my << 16 | kCropInside: the MCU lies in the rectangle's box, it is transformed and stored
};
constexpr uint32_t kCropInside = 1u << 31;

// (the box test on the MCU's pixels: the rectangle's corners are what the store stage holds in registers anyway)
template <int HS, int VS>
CG_DEV uint32_t crop_place(const CropEdges &c, uint32_t mx, uint32_t my)
{
    constexpr uint32_t kW = 8u * HS, kH = VS == 0 ? 8u : 8u * VS;
    const bool inside = mx * kW < c.x1 && (mx + 1u) * kW > c.x0 && my * kH < c.y1 && (my + 1u) * kH > c.y0;
    return mx | my << 16 | (inside ? kCropInside : 0u);
}

template <int HS, int VS>
CG_DEV bool crop_mcu_inside(const CropMcu<HS, VS> &t)
{
    return (t.at & kCropInside) != 0u;
}

template <int HS, int VS>
CG_DEV void crop_init(CropMcu<HS, VS> &t, const ImageDesc &d, const CropEdges &c, uint32_t interval)
{
#pragma unroll
    for (int k = 0; k < CropMcu<HS, VS>::kDus; k++)
#pragma unroll
        for (int w = 0; w < 16; w++)
            t.px[k][w] = 0u;
    const uint32_t mcu0 = interval * d.restart_interval;
    t.at = crop_place<HS, VS>(c, mcu0 % d.width_mcus, mcu0 / d.width_mcus);
}

// One data unit of an MCU in the box: coefficients out of `slot` (cleared for reuse) and IDCT; k: its place in the MCU.
// One copy of the IDCT in the instruction stream, as in planes_transform.  Of an MCU outside the box: the slot cleared.
// (The branch is the lane's own; a wave skips the transform when none of its lanes has an MCU in the box.)
template <int HS, int VS>
CG_DEV void crop_unit(CropMcu<HS, VS> &t, const ImageDesc &d, uint32_t comp, uint32_t k, uint8_t *slot, int32_t dc)
{
    constexpr int kDus = CropMcu<HS, VS>::kDus;
    if (!crop_mcu_inside<HS, VS>(t)) {
        zero_slot(slot);
        return;
    }
    uint32_t rec[kRetained / 2];
    take_slot(slot, rec);
    idct_data_unit(rec, dc, d.quant[comp], t.px[kDus - 1]);
#pragma unroll
    for (int j = 0; j < kDus - 1; j++) {
        if (k == uint32_t(j)) {
#pragma unroll
            for (int w = 0; w < 16; w++)
                t.px[j][w] = t.px[kDus - 1][w];
        }
    }
}

// Four pixels of one row, image columns X .. X + 3 (X a multiple of 4) of image row Y, of which columns cx0 .. cx1 - 1
// lie in the rectangle (some do).  All four inside: one 16-byte store where the address allows it (RGBA; planar: twelve
// bytes).  Any other group -- one the rectangle's edge cuts, one at another address -- goes pixel by pixel in a loop of
// its own.  One test per group, not one per pixel: tests that do not depend on the row the compiler keeps as lane masks
// over all the rows, and sixteen of those are more scalar registers than a wave has.  The format is wave-uniform.
CG_DEV void crop_store4(const CropTarget &g, const CropEdges &c, uint32_t X, uint32_t Y, uint32_t cx0, uint32_t cx1,
                        const uint32_t (&p)[4])
{
    const uint32_t lo = umax(cx0, X) - X, hi = umin(cx1, X + 4u) - X; // pixels lo .. hi - 1 of the four
    const uint32_t row = Y - c.y0, col = X + lo - c.x0;
    if (g.format == kCropRgba) {
        uint8_t *at = c.img + uint64_t(row) * c.pitch + 4u * col;
        if (hi - lo == 4u && (reinterpret_cast<uintptr_t>(at) & 15u) == 0u) {
            store_pixels<false>(at, Vec4u{p[0], p[1], p[2], p[3]});
            return;
        }
#pragma unroll 1
        for (uint32_t i = lo; i < hi; i++, at += 4)
            *CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(at)) = i == 0u ? p[0] : (i == 1u ? p[1] : (i == 2u ? p[2] : p[3]));
    } else {
        const uint64_t plane = uint64_t(c.plane_hi) << 32 | c.plane_lo;
        auto *q = CG_GLOBAL(uint8_t, c.img + uint64_t(row) * c.pitch + col); // (planar: the pitch is the width)
        if (hi - lo == 4u) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    q[uint64_t(ch) * plane + uint32_t(i)] = uint8_t(p[i] >> (8 * ch));
            return;
        }
#pragma unroll 1
        for (uint32_t i = lo; i < hi; i++, q++) {
            const uint32_t v = i == 0u ? p[0] : (i == 1u ? p[1] : (i == 2u ? p[2] : p[3]));
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                q[uint64_t(ch) * plane] = uint8_t(v >> (8 * ch));
        }
    }
}

// The lane's MCU, which lies in the box: its rows inside the rectangle, of each the pixels inside it; luma sample (X, Y) of
// the MCU goes with chroma sample (X / HS, Y / VS).  The eight rows of a row of luma data units are unrolled -- every
// word of samples is then a register of its own, where rows picked by a loop's counter cost the 4:2:2 kernel its
// registers -- and of the two rows of data units of a 16-row MCU one copy of that code serves both, its words chosen
// between the two by v (two-way selects): half the code, which for 4:2:0 is still most of the kernel's.
template <int HS, int VS>
CG_DEV void crop_store_mcu(const CropMcu<HS, VS> &t, const CropTarget &g, const CropEdges &c)
{
    using M = CropMcu<HS, VS>;
    constexpr int kRows = M::kLumaRows;
    const uint32_t X0 = (t.at & 0xffffu) * uint32_t(8 * HS), Y0 = ((t.at >> 16) & 0x7fffu) * uint32_t(8 * kRows);
    const uint32_t cx0 = umax(c.x0, X0), cx1 = umin(c.x1, X0 + uint32_t(8 * HS));
    const uint32_t cy0 = umax(c.y0, Y0), cy1 = umin(c.y1, Y0 + uint32_t(8 * kRows));
#pragma unroll 1
    for (uint32_t v = 0; v < uint32_t(kRows); v++) {
        const bool low = kRows == 2 && v != 0u; // the lower row of luma data units
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t Y = Y0 + 8u * v + uint32_t(r);
            // (a row outside the rectangle: its left edge put out of every group's reach -- X + 4 is at most 65536.  One
            // test per group and row, none per group alone that the compiler would hold as a lane mask over all the rows)
            const uint32_t rx0 = cx0 + ((Y < cy0 || Y >= cy1) ? 0x10000u : 0u);
            uint32_t cb[2] = {0u, 0u}, cr[2] = {0u, 0u};
            if constexpr (VS != 0) {
                constexpr int kLow = VS == 2 ? 4 : 0; // (chroma rows 4 .. 7 go with the lower luma rows)
                const int rc = VS == 2 ? r >> 1 : r;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    cb[j] = low ? t.px[M::kLuma][2 * (rc + kLow) + j] : t.px[M::kLuma][2 * rc + j];
                    cr[j] = low ? t.px[M::kLuma + 1][2 * (rc + kLow) + j] : t.px[M::kLuma + 1][2 * rc + j];
                }
            }
#pragma unroll
            for (int h = 0; h < HS; h++) {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint32_t X = X0 + uint32_t(8 * h + 4 * j);
                    if (X + 4u <= rx0 || X >= cx1)
                        continue;
                    const uint32_t yw = low ? t.px[(kRows - 1) * HS + h][2 * r + j] : t.px[h][2 * r + j];
                    uint32_t p[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const uint32_t ys = (yw >> (8 * i)) & 0xffu;
                        if constexpr (VS == 0) {
                            p[i] = ys * 0x010101u | 0xff000000u;
                        } else {
                            const int col = (8 * h + 4 * j + i) / HS; // (the chroma column: a constant once unrolled)
                            p[i] = ycbcr_to_rgba(ys, (cb[col >> 2] >> (8 * (col & 3))) & 0xffu, (cr[col >> 2] >> (8 * (col & 3))) & 0xffu);
                        }
                    }
                    crop_store4(g, c, X, Y, rx0, cx1, p);
                }
            }
        }
    }
}

// To the MCU behind it in raster order.
template <int HS, int VS>
CG_DEV void crop_next_mcu(CropMcu<HS, VS> &t, const CropEdges &c)
{
    const uint32_t mx = (t.at & 0xffffu) + 1u, my = (t.at >> 16) & 0x7fffu;
    const bool wrap = mx >= c.width_mcus;
    t.at = crop_place<HS, VS>(c, wrap ? 0u : mx, wrap ? my + 1u : my);
}

// The whole path for 64 restart intervals, one per lane.  A lane whose interval does not touch the box, or lies past the
// image's last, does nothing; a touched one stops behind its last MCU in the box.  The lanes of a wave thus leave the
// loop at different counts: nothing in it goes from lane to lane (no quad exchange, lane-local stores), and what stays
// wave-uniform is the data unit's place in its MCU, the same in every lane that is still walking.
// g: the rectangle, its box of MCUs and the format (its pitch is not read here: `into`'s is).
template <int HS, int VS, class Into>
CG_DEV void decode_wave_cropped(const ImageDesc &d, const HuffShared &s, const CropTarget &g, const Into &into, uint8_t *img, uint32_t interval,
                                uint32_t lane)
{
    constexpr uint32_t kDus = uint32_t(CropMcu<HS, VS>::kDus), kLuma = uint32_t(CropMcu<HS, VS>::kLuma);
    const uint32_t reach = interval < d.total_intervals ? crop_intervals_reach(d, g, interval, 1u) : 0u;
    if (reach == 0u)
        return;
    uint8_t *slot = s.du_slots + lane * kDuSlotBytes;
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    const CropEdges c = crop_edges(d, g, crop_slot(into, g), img);
    CropMcu<HS, VS> t;
    crop_init<HS, VS>(t, d, c, interval);
    const uint32_t du_total = reach * kDus;
    uint32_t k = 0; // the data unit's place inside its MCU (the same in every lane still in the loop)
#pragma unroll 1
    for (uint32_t du = 0; du < du_total; du++) {
        const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
        const int32_t dc = entropy_data_unit(e, d, s, comp, slot16);
        crop_unit<HS, VS>(t, d, comp, k, slot, dc);
        if (k == kDus - 1u) {
            if (crop_mcu_inside<HS, VS>(t))
                crop_store_mcu<HS, VS>(t, g, c);
            crop_next_mcu<HS, VS>(t, c);
            k = 0;
        } else {
            k++;
        }
    }
}

// ... into a destination that holds the rectangle alone.
template <int HS, int VS>
CG_DEV void decode_wave_cropped(const ImageDesc &d, const HuffShared &s, const CropTarget &g, uint8_t *img, uint32_t interval, uint32_t lane)
{
    decode_wave_cropped<HS, VS>(d, s, g, CropOwnSlot{}, img, interval, lane);
}

} // namespace compeg
