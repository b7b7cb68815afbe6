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

// One slot of an oriented pack (orient_body.h): `region.dst` is dst', inside the slot T whose extent is the upright ow x oh
// for the orientations 1..4 and oh x ow for 5..8.
struct OrientSource {
    RegionSource region;
    uint32_t orientation; // 1..8
};

// The rectangle of T that holds what `r`, a rectangle inside the upright w x h, holds: the contract's dst -> dst'.
// False: no such orientation, or the rectangle leaves w x h.  64-bit integers.
inline bool orient_rect(uint32_t w, uint32_t h, uint32_t orientation, const compeg_rect &r, compeg_rect &out)
{
    if (orientation < 1u || orientation > 8u || uint64_t(r.x) + r.width > w || uint64_t(r.y) + r.height > h)
        return false;
    const uint32_t fx = uint32_t(uint64_t(w) - r.x - r.width), fy = uint32_t(uint64_t(h) - r.y - r.height);
    switch (orientation) {
    case 1: out = compeg_rect{r.x, r.y, r.width, r.height}; break;
    case 2: out = compeg_rect{fx, r.y, r.width, r.height}; break;
    case 3: out = compeg_rect{fx, fy, r.width, r.height}; break;
    case 4: out = compeg_rect{r.x, fy, r.width, r.height}; break;
    case 5: out = compeg_rect{r.y, r.x, r.height, r.width}; break;
    case 6: out = compeg_rect{r.y, fx, r.height, r.width}; break;
    case 7: out = compeg_rect{fy, fx, r.height, r.width}; break;
    default: out = compeg_rect{fy, r.x, r.height, r.width}; break;
    }
    return true;
}

} // namespace compeg
