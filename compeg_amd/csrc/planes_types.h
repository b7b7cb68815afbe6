// Plain data shared by the host runtime and the planes kernels (planes_kernels.hip, planes_body.h).
#pragma once

#include <cstdint>

namespace compeg {

// Where one launch of a planes decode writes: the destination is the caller's, so every extent here is exact -- nothing
// is rounded up to whole MCUs, and what lies outside a plane's row_bytes x rows is never written.  All images of the
// launch have one size and one sampling: image i's planes lie at dst + i * image_stride + offset[p].
// The values are compeg_planes_shape's (capi.cpp: planes_layout), checked there.
struct PlanesTarget {
    uint8_t *dst;
    uint64_t image_stride;
    uint64_t offset[3];    // plane p's first byte inside an image
    uint32_t pitch[3];     // bytes from row to row
    uint32_t row_bytes[3]; // bytes of a row that belong to the plane
    uint32_t rows[3];
    uint32_t format;       // COMPEG_PLANES_PLANAR / _SEMIPLANAR / _YUYV / _UYVY
    uint32_t chroma420;    // 4:2:2 files only: chroma rows 2r and 2r + 1 averaged into row r
};

constexpr uint32_t kPlanesPlanar = 0, kPlanesSemiplanar = 1, kPlanesYuyv = 2, kPlanesUyvy = 3;

} // namespace compeg
