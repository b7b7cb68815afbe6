// gfx950 kernels of the cropped decode of a region list: the cropped kernels' prologue (crop_window.h) and
// lane body (crop_body.h) with the rectangle read from a record in device memory instead of the kernel's arguments --
// grid (workgroups per image, regions of one sampling), blockIdx.y picks the record, the record picks the image.  What
// is the same for every region (destination, pitch, plane stride, format) stays an argument.
#include <hip/hip_runtime.h>

#include "crop_regions_body.h"
#include "crop_window.h"

namespace compeg {

static_assert(kCropRegionGroups == kSamplings, "one group of regions per row of a family's kernel table");
static_assert(crop_region_group(2, 1) == kSampling422 && crop_region_group(1, 1) == kSampling444 && crop_region_group(1, 2) == kSampling440 &&
                  crop_region_group(2, 2) == kSampling420 && crop_region_group(1, 0) == kSamplingGray, "... in the table's order");

// The record's words are the same for the whole workgroup: blockIdx.y is, and the records are read-only for the
// launch, so they are loaded once, as scalars, like the image's descriptor.
template <int HS, int VS>
__device__ __forceinline__ void cropped_regions_kernel_body(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records,
                                                            const CropRegionsTarget &t, uint32_t l2_in_lds, uint32_t window_words)
{
    const CropRegionRecord &r = records[blockIdx.y];
    const CropTarget g = crop_region_rect(r, t);
    crop_window_kernel(descs, r.image, g, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
        decode_wave_cropped_region<HS, VS>(d, s, g, t, interval, lane);
    });
}

// The launch bounds are the one-rectangle kernels' (crop_kernels.hip): the lane holds the same samples.
__global__ void __launch_bounds__(768)
decode_cropped_regions_422_kernel(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records, CropRegionsTarget t,
                                  uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_regions_kernel_body<2, 1>(descs, records, t, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_regions_444_kernel(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records, CropRegionsTarget t,
                                  uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_regions_kernel_body<1, 1>(descs, records, t, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_regions_440_kernel(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records, CropRegionsTarget t,
                                  uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_regions_kernel_body<1, 2>(descs, records, t, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(512)
decode_cropped_regions_420_kernel(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records, CropRegionsTarget t,
                                  uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_regions_kernel_body<2, 2>(descs, records, t, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_regions_gray_kernel(const ImageDesc *__restrict__ descs, const CropRegionRecord *__restrict__ records, CropRegionsTarget t,
                                   uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_regions_kernel_body<1, 0>(descs, records, t, l2_in_lds, window_words);
}

// Waves per workgroup the planner may choose: the one-rectangle kernels' caps, which these launch bounds hold.
uint32_t crop_regions_wave_cap(uint32_t hs, uint32_t vs) { return crop_wave_cap(hs, vs); }

hipError_t launch_cropped_regions(const ImageDesc *descs, const CropRegionRecord *records, uint32_t regions, uint32_t max_intervals,
                                  const HuffLdsPlan &plan, uint32_t group, const CropRegionsTarget &target, hipStream_t stream)
{
    static constexpr void (*kKernels[kSamplings])(const ImageDesc *, const CropRegionRecord *, CropRegionsTarget, uint32_t, uint32_t) = {
        decode_cropped_regions_422_kernel, decode_cropped_regions_444_kernel, decode_cropped_regions_440_kernel, decode_cropped_regions_420_kernel,
        decode_cropped_regions_gray_kernel};
    if (group >= kSamplings || regions > 65535u || plan.waves_per_block > crop_regions_wave_cap(kCropRegionGroupHs[group], kCropRegionGroupVs[group]))
        return hipErrorInvalidValue;
    return launch_interval_grid(kKernels[group], descs, regions, max_intervals, plan, stream, records, target);
}

} // namespace compeg
