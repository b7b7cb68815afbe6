// Plain data shared by the host runtime and the scaled kernels (scaled_kernels.hip, scaled_body.h).
#pragma once

#include <cstdint>

namespace compeg {

// Where one launch of a scaled (1/2- or 1/4-scale) decode writes: the destination is the caller's, so the extent is
// exact -- ow x oh = ceil(W / den) x ceil(H / den) pixels, n x n = (8 / den)^2 per data unit, and nothing outside them
// is ever written.  All images of the launch have one size and one sampling: image i lies at dst + i * image_stride.
// The values are compeg_scaled_shape's (capi.cpp: scaled_layout), checked there.
struct ScaledTarget {
    uint8_t *dst;
    uint64_t image_stride;
    uint32_t ow, oh;
    uint32_t pitch;  // RGBA: bytes from row to row (a multiple of 4, like dst); planar: ow
    uint32_t format; // COMPEG_SCALED_RGBA / _RGB_PLANAR
    uint32_t n;      // samples a data unit gives along an axis: 4 (1/2 scale) or 2 (1/4 scale)
};

constexpr uint32_t kScaledRgba = 0, kScaledRgbPlanar = 1;

} // namespace compeg
