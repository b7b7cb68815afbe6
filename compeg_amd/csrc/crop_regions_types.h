// Plain data shared by the host and the kernels of the cropped decode of a region list (crop_regions_kernels.hip;
// DESIGN.md 5.21): a rectangle per region, each out of an image of its own, each into a slot of its own.
#pragma once

#include <cstdint>
#include <vector>

namespace compeg {

// One region as a workgroup reads it from device memory (blockIdx.y picks it): which image, the rectangle in pixels of
// that image and in its MCUs (columns mx0 .. mx1 - 1, rows my0 .. my1 - 1: computed once on the host, as for CropTarget),
// and where the rectangle's first pixel lies, in bytes from the destination's first.  The offset carries the slot and
// the place inside it, so a record's position in the array says nothing about where it writes.
struct CropRegionRecord {
    uint32_t image;
    uint32_t x, y, width, height;
    uint32_t mx0, mx1, my0, my1;
    uint32_t reserved;
    uint64_t offset;
};
static_assert(sizeof(CropRegionRecord) == 48, "the kernels read records 48 bytes apart");

// What is the same for every region of a call: the destination, the slots' pitch (RGBA: bytes from row to row; planar:
// the slot's width), the bytes of one of a slot's planes (slot width x slot height) and the format (COMPEG_CROP_*).
struct CropRegionsTarget {
    uint8_t *dst;
    uint64_t plane;
    uint32_t pitch;
    uint32_t format;
};

// The launches of one call: one per luma sampling present among the images the regions name, in this order.
constexpr uint32_t kCropRegionGroups = 5;
// (hs x vs: the luma sampling, 1 x 0 for a grayscale image; kCropRegionGroups: no kernel for it)
constexpr uint32_t crop_region_group(uint32_t hs, uint32_t vs)
{
    return hs == 2 && vs == 1 ? 0u : hs == 1 && vs == 1 ? 1u : hs == 1 && vs == 2 ? 2u : hs == 2 && vs == 2 ? 3u : hs == 1 && vs == 0 ? 4u : kCropRegionGroups;
}
constexpr uint32_t kCropRegionGroupHs[kCropRegionGroups] = {2, 1, 1, 2, 1}, kCropRegionGroupVs[kCropRegionGroups] = {1, 1, 2, 2, 0};

// A validated call (capi.cpp: crop_regions_call): the records grouped by their image's sampling -- a stable grouping,
// group g's records behind group g - 1's -- with each group's count and the largest interval count among its images.
struct CropRegionsCall {
    CropRegionsTarget target{};
    std::vector<CropRegionRecord> records;
    uint32_t count[kCropRegionGroups] = {0, 0, 0, 0, 0};
    uint32_t intervals[kCropRegionGroups] = {0, 0, 0, 0, 0};
};

// One region's record: the rectangle (inside its image: checked by the caller) against MCUs of mcu_w x mcu_h pixels.
inline CropRegionRecord crop_region_record(uint32_t image, uint32_t x, uint32_t y, uint32_t width, uint32_t height, uint32_t mcu_w, uint32_t mcu_h,
                                           uint64_t offset)
{
    return CropRegionRecord{image, x, y, width, height, x / mcu_w, (x + width - 1u) / mcu_w + 1u, y / mcu_h, (y + height - 1u) / mcu_h + 1u, 0u, offset};
}

// A checked region with what the grouping needs of its image: the luma sampling (1 x 0: grayscale; one of the five)
// and the image's restart intervals.
struct CropRegionPlace {
    uint32_t image, x, y, width, height, dst_x, dst_y;
    uint32_t hs, vs, intervals;
};

// The call for `count` checked regions, region k into slot k: slots of slot_bytes, rows target.pitch apart, pixel_bytes a
// pixel in a row (RGBA: 4; planar: 1).  The grouping is stable and every record carries its own place.
inline CropRegionsCall make_crop_regions_call(const CropRegionsTarget &target, uint64_t slot_bytes, uint32_t pixel_bytes, const CropRegionPlace *places,
                                              size_t count)
{
    CropRegionsCall call;
    call.target = target;
    call.records.reserve(count);
    for (uint32_t g = 0; g < kCropRegionGroups; g++)
        for (size_t k = 0; k < count; k++) {
            const CropRegionPlace &p = places[k];
            if (crop_region_group(p.hs, p.vs) != g)
                continue;
            const uint64_t offset = uint64_t(k) * slot_bytes + uint64_t(p.dst_y) * target.pitch + uint64_t(p.dst_x) * pixel_bytes;
            call.records.push_back(crop_region_record(p.image, p.x, p.y, p.width, p.height, 8u * p.hs, 8u * (p.vs ? p.vs : 1u), offset));
            call.count[g]++;
            call.intervals[g] = call.intervals[g] > p.intervals ? call.intervals[g] : p.intervals;
        }
    return call;
}

} // namespace compeg
