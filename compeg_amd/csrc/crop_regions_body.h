// A region of a list through the cropped kernels' lane body (crop_body.h, which does the work): what a
// region's record and the call's target are to decode_wave_cropped.  No HIP dependency: tests/emul_crop_regions calls it
// lane by lane.
#pragma once

#include "crop_body.h"
#include "crop_regions_types.h"

namespace compeg {

// The record's rectangle, as the one-rectangle decode's target has one: the touch test and the store stage read x, y,
// width, height, the box of MCUs and the format from it; dst is where the region's first pixel lies.
CG_DEV CropTarget crop_region_rect(const CropRegionRecord &r, const CropRegionsTarget &t)
{
    CropTarget g{};
    g.dst = t.dst + r.offset;
    g.image_stride = 0;
    g.x = r.x;
    g.y = r.y;
    g.width = r.width;
    g.height = r.height;
    g.pitch = t.pitch;
    g.format = t.format;
    g.mx0 = r.mx0;
    g.mx1 = r.mx1;
    g.my0 = r.my0;
    g.my1 = r.my1;
    return g;
}

// ... and what it is laid into: the slot's rows and planes, not the rectangle's.
struct CropRegionSlot {
    const CropRegionsTarget &t;
};
CG_DEV CropSlot crop_slot(const CropRegionSlot &s, const CropTarget &)
{
    return CropSlot{s.t.pitch, s.t.plane};
}

// 64 restart intervals of the region's image, one per lane (g: crop_region_rect's).
template <int HS, int VS>
CG_DEV void decode_wave_cropped_region(const ImageDesc &d, const HuffShared &s, const CropTarget &g, const CropRegionsTarget &t, uint32_t interval,
                                       uint32_t lane)
{
    decode_wave_cropped<HS, VS>(d, s, g, CropRegionSlot{t}, g.dst, interval, lane);
}

} // namespace compeg
