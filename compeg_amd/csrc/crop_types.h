// Plain data shared by the host runtime and the cropped kernels (crop_kernels.hip, crop_body.h).
#pragma once

#include <cstdint>

namespace compeg {

// Where one launch of a cropped decode writes: the destination is the caller's and holds the rectangle alone -- pixel
// (i, j) of it is pixel (x + i, y + j) of the image, and nothing outside width x height pixels is ever written.  All
// images of the launch have one size and one sampling: image i lies at dst + i * image_stride.
// The values are compeg_crop_shape's (capi.cpp: crop_layout), checked there; the rectangle in MCUs is computed there
// once: MCU columns mx0 .. mx1 - 1 and MCU rows my0 .. my1 - 1 are the ones with a pixel inside the rectangle.
struct CropTarget {
    uint8_t *dst;
    uint64_t image_stride;
    uint32_t x, y, width, height; // pixels of the image; non-empty, inside it
    uint32_t pitch;               // RGBA: bytes from row to row (a multiple of 4, like dst); planar: width
    uint32_t format;              // COMPEG_CROP_RGBA / _RGB_PLANAR
    uint32_t mx0, mx1, my0, my1;
};

constexpr uint32_t kCropRgba = 0; // (anything else: the planar format -- the host has refused what is neither)

} // namespace compeg
