// Plain data shared by the host runtime and the reduced kernels (reduced_kernels.hip, reduced_body.h).
#pragma once

#include <cstdint>

namespace compeg {

// Where one launch of a reduced (1/8-scale) decode writes: the destination is the caller's, so the extent is exact --
// ow x oh = ceil(W / 8) x ceil(H / 8) pixels, one per luma data unit, and nothing outside them is ever written.  All
// images of the launch have one size and one sampling: image i lies at dst + i * image_stride.
// The values are compeg_reduced_shape's (capi.cpp: reduced_layout), checked there.
struct ReducedTarget {
    uint8_t *dst;
    uint64_t image_stride;
    uint32_t ow, oh;
    uint32_t pitch;  // RGBA: bytes from row to row (a multiple of 4, like dst); planar: ow
    uint32_t format; // COMPEG_REDUCED_RGBA / _RGB_PLANAR
};

constexpr uint32_t kReducedRgba = 0, kReducedRgbPlanar = 1;

} // namespace compeg
