// Lane body of the levels kernels (decode_levels_*_kernel, levels_kernels.hip): a decode that stops
// behind the entropy stage and writes every data unit's quantised levels, all 64 zig-zag positions, as one block of 64
// int16 into memory of the caller's.  No HIP dependency up to the wave function at the end: tests/emul_levels drives the
// same steps lane by lane.
//
// A lane per restart interval, coefficients through the lane's LDS slot with the shared reader in its 64-position form
// (entropy_data_unit<false, kLevelsKept>: quirk Q3 does not act, a position beyond 63 lands in the dummy position).  No
// quantiser, no IDCT, no colour step.  Per data unit:
//
//   1. position 0 of the slot becomes the low 16 bits of the component's DC predictor behind this unit's difference
//      (the predictor itself, selected by value out of the reader's state, not the dequantised term the reader returns);
//   2. the lane leaves the block's place in the destination (a byte offset into the image, or kLevelsNoPlace: a lane
//      without an interval of its own, a block outside the rasters) in the slot's last eight bytes;
//   3. the wave stores its 64 blocks transposed: in round j = 0..7 lane L writes the 16-byte piece L % 8 of the block of
//      lane 8 j + L / 8, read out of that lane's slot -- eight lanes a whole 128-byte line, a store instruction eight
//      lines.  Natural order permutes while reading: piece p is row p of the 8 x 8, eight int16 gathers by the row's
//      zig-zag positions (the lane's own for the whole kernel: LevelsRow), packed in pairs;
//   4. the slot is cleared.
#pragma once

#include "kernels_body.h"
#include "levels_types.h"

namespace compeg {

static_assert(kLevelsSlotBytes == slot_bytes(kLevelsKept), "the reader's slot");

constexpr uint64_t kLevelsNoPlace = ~uint64_t(0);

// HS x VS: the luma sampling; VS = 0: a grayscale image, one data unit an MCU and no chroma.
template <int HS, int VS>
struct LevelsMcu {
    static constexpr int kLuma = VS == 0 ? 1 : HS * VS, kDus = VS == 0 ? 1 : HS * VS + 2, kRows = VS == 0 ? 1 : VS;
    uint32_t mx, my;
    bool active; // the lane has an interval of its own: its blocks have places
};

template <int HS, int VS>
CG_DEV void levels_init(LevelsMcu<HS, VS> &t, const ImageDesc &d, uint32_t interval, bool active)
{
    mcu_cursor_init(t, d, interval);
    t.active = active;
}

// The byte offsets inside a slot of the eight zig-zag positions of row `piece` of the 8 x 8 (natural index 8 piece + i
// in byte i of the two words): what a lane gathers by in natural order, every round the same.
struct LevelsRow {
    uint32_t at[2];
};

CG_DEV void levels_row_init(LevelsRow &r, uint32_t piece)
{
    r.at[0] = r.at[1] = 0u;
#pragma unroll
    for (int i = 0; i < 8; i++)
        r.at[i / 4] |= uint32_t(zigzag_of(int(piece) * 8 + i) * 2) << (8 * (i % 4));
}

// Where data unit k of the lane's MCU goes (k is wave-uniform): a byte offset into the image, always inside it.
template <int HS, int VS>
CG_DEV uint64_t levels_place(const LevelsMcu<HS, VS> &t, const LevelsTarget &g, uint32_t k)
{
    constexpr uint32_t kLuma = uint32_t(LevelsMcu<HS, VS>::kLuma), kRows = uint32_t(LevelsMcu<HS, VS>::kRows);
    const uint32_t c = k < kLuma ? 0u : k - kLuma + 1u;
    const uint32_t bx = k < kLuma ? t.mx * uint32_t(HS) + k % uint32_t(HS) : t.mx;
    const uint32_t by = k < kLuma ? t.my * kRows + k / uint32_t(HS) : t.my;
    if (!t.active || bx >= g.blocks_w[c] || by >= g.blocks_h[c])
        return kLevelsNoPlace;
    return g.offset[c] + (uint64_t(by) * g.blocks_w[c] + bx) * uint64_t(kLevelsKept * 2);
}

// Steps 1 and 2: the finished data unit's slot made ready for the wave's store.  pred: the component's predictor.
CG_DEV void levels_unit(uint8_t *slot, int32_t pred, uint64_t place)
{
    reinterpret_cast<int16_t *>(slot)[0] = int16_t(uint16_t(uint32_t(pred) & 0xffffu));
    slot_word_t *p = reinterpret_cast<slot_word_t *>(slot + kLevelsPlaceAt);
    p[0] = uint32_t(place);
    p[1] = uint32_t(place >> 32);
}

// Step 3, one lane's share: eight 16-byte pieces, one of each of eight lanes' blocks.
CG_DEV void levels_store(const uint8_t *wave_slots, uint32_t lane, const LevelsRow &row, uint32_t order, uint8_t *img)
{
    const uint32_t piece = lane & 7u, sub = lane >> 3;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint8_t *other = wave_slots + (8u * j + sub) * uint32_t(kLevelsSlotBytes);
        const slot_word_t *p = reinterpret_cast<const slot_word_t *>(other + kLevelsPlaceAt);
        const uint64_t place = uint64_t(p[0]) | uint64_t(p[1]) << 32;
        if (place == kLevelsNoPlace)
            continue;
        uint32_t w[4];
        if (order == kLevelsNatural) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t lo = (row.at[i / 2] >> (16 * (i % 2))) & 0xffu, hi = (row.at[i / 2] >> (16 * (i % 2) + 8)) & 0xffu;
                const uint32_t a = *reinterpret_cast<const uint16_t *>(other + lo), b = *reinterpret_cast<const uint16_t *>(other + hi);
                w[i] = a | b << 16;
            }
        } else {
            const SlotVec v = reinterpret_cast<const SlotVec *>(other)[piece];
            w[0] = v.x;
            w[1] = v.y;
            w[2] = v.z;
            w[3] = v.w;
        }
        *CG_GLOBAL(Vec4u, reinterpret_cast<Vec4u *>(img + place + piece * 16u)) = Vec4u{w[0], w[1], w[2], w[3]};
    }
}

// (the name the wave function and the emulation driver step by)
template <int HS, int VS>
CG_DEV void levels_next_mcu(LevelsMcu<HS, VS> &t, const ImageDesc &d)
{
    mcu_cursor_next(t, d);
}

#if defined(__HIPCC__)
// The whole path for 64 restart intervals, one per lane.  Lanes past the image's last interval decode that last interval
// once more and their blocks have no place, as in the planes kernels: the wave's control flow stays one, and every one
// of the 64 slots a round of the store reads has been written in this step.
template <int HS, int VS>
CG_DEV void decode_wave_levels(const ImageDesc &d, const HuffShared &s, const LevelsTarget &g, uint8_t *img, uint32_t interval, uint32_t lane)
{
    constexpr uint32_t kDus = uint32_t(LevelsMcu<HS, VS>::kDus), kLuma = uint32_t(LevelsMcu<HS, VS>::kLuma);
    const bool active = interval < d.total_intervals;
    interval = active ? interval : d.total_intervals - 1u;
    uint8_t *slot = s.du_slots + lane * uint32_t(kLevelsSlotBytes);
    int16_t *slot16 = reinterpret_cast<int16_t *>(slot);
    zero_slot<kLevelsKept>(slot);
    EntropyState e;
    entropy_init(e, d, s, interval);
    LevelsMcu<HS, VS> t;
    levels_init<HS, VS>(t, d, interval, active);
    LevelsRow row;
    levels_row_init(row, lane & 7u);
    const uint32_t du_total = d.restart_interval * kDus;
    uint32_t k = 0; // the data unit's place inside its MCU (wave-uniform)
#pragma unroll 1
    for (uint32_t du = 0; du < du_total; du++) {
        const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
        entropy_data_unit<false, kLevelsKept>(e, d, s, comp, slot16);
        // (a value, not an address, is selected: the state has to stay in registers)
        const int32_t p0 = e.pred0, p1 = e.pred1, p2 = e.pred2;
        levels_unit(slot, comp == 0u ? p0 : (comp == 1u ? p1 : p2), levels_place<HS, VS>(t, g, k));
        levels_store(s.du_slots, lane, row, g.order, img);
        zero_slot<kLevelsKept>(slot);
        if (k == kDus - 1u) {
            levels_next_mcu<HS, VS>(t, d);
            k = 0;
        } else {
            k++;
        }
    }
}
#endif // __HIPCC__

} // namespace compeg
