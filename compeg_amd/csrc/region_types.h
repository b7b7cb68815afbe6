// What one slot of a region pack reads and where it puts it (region_body.h plans with it; kernels.h hands it to the
// library's host code, which does not see the lane bodies).
#pragma once

#include <cstdint>

#include "compeg_hip.h"

namespace compeg {

struct RegionSource {
    const void *src; // the image's first pixel, rows pitch bytes apart
    uint32_t pitch;
    compeg_rect crop; // inside the image
    compeg_rect dst;  // inside the ow x oh slot, no side of 0
};

} // namespace compeg
