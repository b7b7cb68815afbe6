// Plain data shared by the host runtime and the levels kernels (levels_kernels.hip, levels_body.h).
#pragma once

#include <cstdint>

namespace compeg {

// Where one launch of a levels decode writes: per component c a raster of blocks_w[c] x blocks_h[c] blocks of 64 int16
// (128 bytes, the data unit's quantised levels), whole MCUs, tight, component after component from offset[c] on.  dst is
// a multiple of 16 and so is every offset: a block is a 128-byte line.  All images of the launch have one size and one
// sampling: image i lies at dst + i * image_stride.  The values are compeg_levels_shape's (capi.cpp: levels_layout),
// checked there.
struct LevelsTarget {
    uint8_t *dst;
    uint64_t image_stride;
    uint64_t offset[3];
    uint32_t blocks_w[3], blocks_h[3];
    uint32_t order; // COMPEG_LEVELS_ZIGZAG / _NATURAL
};

constexpr uint32_t kLevelsZigzag = 0, kLevelsNatural = 1;

// Zig-zag positions a levels kernel's reader keeps, and its lane's LDS slot: the positions, then 16 bytes whose first
// two are the dummy position (what lies beyond 63 is dropped there) and whose last eight carry the block's place in
// the destination from the lane to the lanes that store it.
constexpr int kLevelsKept = 64;
constexpr int kLevelsSlotBytes = kLevelsKept * 2 + 16;
constexpr int kLevelsPlaceAt = kLevelsKept * 2 + 8; // (byte offset inside the slot)

} // namespace compeg
