// Lane body of the scaled kernels (decode_scaled_*_kernel, scaled_kernels.hip): a decode at 1/2 or 1/4
// scale that writes N x N pixels per luma data unit (N = 4 or 2) into memory of the caller's -- the entropy decode and an
// N-point inverse DCT of the N x N lowest-frequency corner of each data unit.  No HIP dependency up to the wave function
// at the end: tests/emul_scaled drives the same steps lane by lane.
//
// A lane per restart interval, coefficients through the lane's LDS slot with entropy_data_unit as it is; of the levels
// it leaves there the corner's N * N - 1 are read (by zig-zag position, in take_slot's 16-byte pieces) and the slot is
// cleared.  The transform is IJG libjpeg's scaled IDCT in f32, every step one IEEE operation (this file is compiled with
// -ffp-contract=off like the IDCT):
//
//     in   = float(dc) * 0.125f                       (DC)        (float(level) * quant[z]) * 0.125f    (AC)
//     column pass over v for each u, then row pass over u for each y; the row pass adds 128.5f to its first input
//     N = 4:  e0 = in0 + in2, e1 = in0 - in2, o0 = (in1 * A) + (in3 * B), o1 = (in1 * B) - (in3 * A)
//             out0 = e0 + o0, out1 = e1 + o1, out2 = e1 - o1, out3 = e0 - o0        A = sqrt2 cos(pi/8), B = sqrt2 cos(3pi/8)
//     N = 2:  out0 = in0 + in1, out1 = in0 - in1
//     s    = sample_u8(out)
//
// With every AC term zero each sample is reduced_sample(dc), bit for bit.  Per MCU the lane keeps N * N bytes per data
// unit; at the MCU's last unit come the colour step (ycbcr_to_rgba, chroma nearest neighbour) and the store: the lane's
// own HS N x VS N pixels, ordinary stores.
#pragma once

#include "kernels_body.h"
#include "scaled_types.h"

namespace compeg {

constexpr float kScaledA = float(1.306562965), kScaledB = float(0.541196100);

template <int P>
struct alignas(4) ScaledRow { // P RGBA pixels; the destination promises multiples of 4, no more
    uint32_t p[P];
};

// HS x VS: the luma sampling; VS = 0: a grayscale image, one data unit an MCU and no chroma.  N: 4 or 2.
template <int HS, int VS, int N>
struct ScaledMcu {
    static_assert(N == 4 || N == 2, "the 4-point and the 2-point transform");
    static constexpr int kLuma = VS == 0 ? 1 : HS * VS, kDus = VS == 0 ? 1 : HS * VS + 2, kRows = VS == 0 ? 1 : VS;
    static constexpr int kWords = N * N / 4;
    // data unit k's sample (x, y) in byte (y N + x) % 4 of word (y N + x) / 4; luma units in raster order, then Cb, Cr
    uint32_t s[kDus][kWords];
    uint32_t mx, my;
    bool active; // the lane has an interval of its own: it stores
};

template <int HS, int VS, int N>
CG_DEV void scaled_init(ScaledMcu<HS, VS, N> &t, const ImageDesc &d, uint32_t interval, bool active)
{
#pragma unroll
    for (int k = 0; k < ScaledMcu<HS, VS, N>::kDus; k++)
#pragma unroll
        for (int i = 0; i < ScaledMcu<HS, VS, N>::kWords; i++)
            t.s[k][i] = 0u;
    mcu_cursor_init(t, d, interval);
    t.active = active;
}

// One pass of the transform over N values `stride` apart, in place.
template <int N, int STRIDE, bool ROW_PASS>
CG_DEV void scaled_1d(float *v)
{
    float in0 = v[0];
    if (ROW_PASS)
        in0 = in0 + 128.5f;
    if constexpr (N == 2) {
        const float in1 = v[STRIDE];
        v[0] = in0 + in1;
        v[STRIDE] = in0 - in1;
    } else {
        const float in1 = v[STRIDE], in2 = v[2 * STRIDE], in3 = v[3 * STRIDE];
        const float e0 = in0 + in2, e1 = in0 - in2;
        const float o0 = (in1 * kScaledA) + (in3 * kScaledB);
        const float o1 = (in1 * kScaledB) - (in3 * kScaledA);
        v[0] = e0 + o0;
        v[STRIDE] = e1 + o1;
        v[2 * STRIDE] = e1 - o1;
        v[3 * STRIDE] = e0 - o0;
    }
}

// The pieces of a slot that hold the corner's levels: zig-zag positions up to 4 (N = 2) or 24 (N = 4).
template <int N>
constexpr int kScaledPieces = N == 2 ? 1 : kRetained / 8;

// rec: the slot's first kScaledPieces<N> pieces (levels by zig-zag position, two a word); quant: this component's
// quantiser values as floats (zig-zag order).  w: the N * N samples, (x, y) in byte (y N + x) % 4 of word (y N + x) / 4.
template <int N>
CG_DEV void scaled_samples(const uint32_t (&rec)[4 * kScaledPieces<N>], int32_t dc, const float *quant, uint32_t (&w)[N * N / 4])
{
    float f[N * N]; // f[v * N + u], v the vertical frequency
#pragma unroll
    for (int v = 0; v < N; v++)
#pragma unroll
        for (int u = 0; u < N; u++) {
            const int z = zigzag_of(v * 8 + u);
            if (z == 0) {
                f[0] = static_cast<float>(dc) * 0.125f; // already dequantised with i32 wrap by the decoder
            } else {
                const int32_t lv = int32_t(int16_t(uint16_t(rec[z >> 1] >> ((z & 1) * 16))));
                f[v * N + u] = (static_cast<float>(lv) * quant[z]) * 0.125f;
            }
        }
#pragma unroll
    for (int u = 0; u < N; u++)
        scaled_1d<N, N, false>(f + u);
#pragma unroll
    for (int y = 0; y < N; y++)
        scaled_1d<N, 1, true>(f + y * N);
#pragma unroll
    for (int i = 0; i < N * N / 4; i++)
        w[i] = sample_u8(f[4 * i]) | sample_u8(f[4 * i + 1]) << 8 | sample_u8(f[4 * i + 2]) << 16 | sample_u8(f[4 * i + 3]) << 24;
}

// One data unit: the corner's levels out of its slot, the slot cleared for reuse, its samples kept; k: its place in the
// MCU (wave-uniform).
template <int HS, int VS, int N>
CG_DEV void scaled_unit(ScaledMcu<HS, VS, N> &t, uint32_t k, uint8_t *slot, int32_t dc, const float *quant)
{
    constexpr int kPieces = kScaledPieces<N>, kWords = ScaledMcu<HS, VS, N>::kWords;
    uint32_t rec[4 * kPieces];
    const SlotVec *p = reinterpret_cast<const SlotVec *>(slot);
#pragma unroll
    for (int i = 0; i < kPieces; i++) {
        const SlotVec v = p[i];
        rec[4 * i + 0] = v.x;
        rec[4 * i + 1] = v.y;
        rec[4 * i + 2] = v.z;
        rec[4 * i + 3] = v.w;
    }
    zero_slot(slot);
    uint32_t w[kWords];
    scaled_samples<N>(rec, dc, quant, w);
    // (selects, not stores under a condition: a store behind `k == j` becomes one store at a variable index, and the
    // samples then live in private memory, not in registers)
#pragma unroll
    for (int j = 0; j < ScaledMcu<HS, VS, N>::kDus; j++)
#pragma unroll
        for (int i = 0; i < kWords; i++)
            t.s[j][i] = k == uint32_t(j) ? w[i] : t.s[j][i];
}

// Pixel (px, py) of the lane's MCU, both known when compiled: its luma sample, the chroma sample at (px / HS, py / VS).
template <int HS, int VS, int N>
CG_DEV uint32_t scaled_pixel(const ScaledMcu<HS, VS, N> &t, int px, int py)
{
    constexpr int kLuma = ScaledMcu<HS, VS, N>::kLuma;
    const int at = (py % N) * N + px % N;
    const uint32_t s = (t.s[(py / N) * HS + px / N][at / 4] >> (8 * (at % 4))) & 0xffu;
    if constexpr (VS == 0) {
        return s * 0x010101u | 0xff000000u;
    } else {
        const int cat = (py / VS) * N + px / HS;
        const uint32_t cb = (t.s[kLuma][cat / 4] >> (8 * (cat % 4))) & 0xffu;
        const uint32_t cr = (t.s[kLuma + 1][cat / 4] >> (8 * (cat % 4))) & 0xffu;
        return ycbcr_to_rgba(s, cb, cr);
    }
}

// The lane's MCU: HS N x VS N pixels at (mx HS N, my VS N), whole rows where the extent holds the whole MCU, pixel by
// pixel against the extent where it cuts it.  The format is wave-uniform.
template <int HS, int VS, int N>
CG_DEV void scaled_store_mcu(const ScaledMcu<HS, VS, N> &t, const ScaledTarget &g, uint8_t *img)
{
    constexpr int kW = HS * N, kH = ScaledMcu<HS, VS, N>::kRows * N;
    if (!t.active)
        return;
    const uint32_t x0 = t.mx * uint32_t(kW), y0 = t.my * uint32_t(kH);
    const bool whole = x0 + uint32_t(kW) <= g.ow && y0 + uint32_t(kH) <= g.oh;
    const uint64_t plane = uint64_t(g.ow) * g.oh;
#pragma unroll
    for (int py = 0; py < kH; py++) {
        ScaledRow<kW> row;
#pragma unroll
        for (int px = 0; px < kW; px++)
            row.p[px] = scaled_pixel<HS, VS, N>(t, px, py);
        const uint32_t y = y0 + uint32_t(py);
        if (g.format == kScaledRgba) {
            uint8_t *p = img + uint64_t(y) * g.pitch + uint64_t(x0) * 4u;
            if (whole) {
                *CG_GLOBAL(ScaledRow<kW>, reinterpret_cast<ScaledRow<kW> *>(p)) = row;
            } else {
#pragma unroll
                for (int px = 0; px < kW; px++)
                    if (x0 + uint32_t(px) < g.ow && y < g.oh)
                        CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(p))[px] = row.p[px];
            }
        } else {
            auto *q = CG_GLOBAL(uint8_t, img);
#pragma unroll
            for (int px = 0; px < kW; px++) {
                if (x0 + uint32_t(px) >= g.ow || y >= g.oh)
                    continue;
                const uint64_t at = uint64_t(y) * g.ow + x0 + uint32_t(px);
#pragma unroll
                for (int c = 0; c < 3; c++)
                    q[uint64_t(c) * plane + at] = uint8_t(row.p[px] >> (8 * c));
            }
        }
    }
}

// (the name the wave function and the emulation driver step by)
template <int HS, int VS, int N>
CG_DEV void scaled_next_mcu(ScaledMcu<HS, VS, N> &t, const ImageDesc &d)
{
    mcu_cursor_next(t, d);
}

#if defined(__HIPCC__)
// The whole path for 64 restart intervals, one per lane: decode_wave_reduced's loop.  Lanes past the image's last
// interval decode that last interval once more and store nothing: the wave's control flow stays one.
template <int HS, int VS, int N>
CG_DEV void decode_wave_scaled(const ImageDesc &d, const HuffShared &s, const ScaledTarget &g, uint8_t *img, uint32_t interval, uint32_t lane)
{
    constexpr uint32_t kDus = uint32_t(ScaledMcu<HS, VS, N>::kDus), kLuma = uint32_t(ScaledMcu<HS, VS, N>::kLuma);
    const bool active = interval < d.total_intervals;
    interval = active ? interval : d.total_intervals - 1u;
    uint8_t *slot = s.du_slots + lane * kDuSlotBytes;
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    ScaledMcu<HS, VS, N> t;
    scaled_init<HS, VS, N>(t, d, interval, active);
    const uint32_t du_total = d.restart_interval * kDus;
    uint32_t k = 0; // the data unit's place inside its MCU (wave-uniform)
#pragma unroll 1
    for (uint32_t du = 0; du < du_total; du++) {
        const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
        const int32_t dc = entropy_data_unit(e, d, s, comp, slot16);
        scaled_unit<HS, VS, N>(t, k, slot, dc, d.quant[comp]);
        if (k == kDus - 1u) {
            scaled_store_mcu<HS, VS, N>(t, g, img);
            scaled_next_mcu<HS, VS, N>(t, d);
            k = 0;
        } else {
            k++;
        }
    }
}
#endif // __HIPCC__

} // namespace compeg
