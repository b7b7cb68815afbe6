// The region_tensor_* kernels (region_body.h): one kernel per filter (nearest, bilinear, antialiased bilinear), element
// type and downscale factor; a lane per 16-byte run of an output row of a slot, antialiased a lane per output element.
// No LDS, no lane exchange; compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "region_body.h"

namespace compeg {

// Grid: flat over (slot, item) -- blocks_per_slot workgroups for every slot, one behind the other in x.
#define CG_REGION_KERNEL(fname, FILTER, name, DTYPE, K)                                                               \
    __global__ void __launch_bounds__(kTensorThreads) region_tensor_##fname##_##name##_k##K##_kernel(RegionPack t)    \
    {                                                                                                                 \
        region_tensor_block_lane<DTYPE, K, FILTER>(t, blockIdx.x, threadIdx.x);                                       \
    }
#define CG_REGION_KERNELS(fname, FILTER, name, DTYPE) \
    CG_REGION_KERNEL(fname, FILTER, name, DTYPE, 1)   \
    CG_REGION_KERNEL(fname, FILTER, name, DTYPE, 2)   \
    CG_REGION_KERNEL(fname, FILTER, name, DTYPE, 4)   \
    CG_REGION_KERNEL(fname, FILTER, name, DTYPE, 8)
#define CG_REGION_FILTER(fname, FILTER)                      \
    CG_REGION_KERNELS(fname, FILTER, u8, COMPEG_TENSOR_U8)   \
    CG_REGION_KERNELS(fname, FILTER, f16, COMPEG_TENSOR_F16) \
    CG_REGION_KERNELS(fname, FILTER, bf16, COMPEG_TENSOR_BF16) \
    CG_REGION_KERNELS(fname, FILTER, f32, COMPEG_TENSOR_F32)

CG_REGION_FILTER(nearest, COMPEG_RESIZE_NEAREST)
CG_REGION_FILTER(bilinear, COMPEG_RESIZE_BILINEAR)
CG_REGION_FILTER(antialias, (COMPEG_RESIZE_BILINEAR | COMPEG_RESIZE_ANTIALIAS))

using RegionKernel = void (*)(RegionPack);

static_assert(sizeof(RegionSlot) == kRegionRecordBytes, "kernels.h states the record's size");
bool make_region_blob(std::vector<uint32_t> &blob, size_t &tables_at, const RegionSource *sources, uint32_t slots, uint32_t k, uint32_t filter)
{
    size_t axes = 0;
    return plan_region_slots(blob, tables_at, axes, sources, slots, k, filter);
}

bool region_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_resize_spec &resize)
{
    RegionPack t;
    uint32_t blocks = 0;
    return plan_region_pack(t, blocks, slots, spec, resize, nullptr, nullptr);
}

hipError_t launch_region_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_resize_spec &resize, const float *pad, void *dst, hipStream_t stream)
{
    static const RegionKernel kernels[3][4][4] = {
#define CG_REGION_ROW(fname, name)                                                                        \
    {region_tensor_##fname##_##name##_k1_kernel, region_tensor_##fname##_##name##_k2_kernel,              \
     region_tensor_##fname##_##name##_k4_kernel, region_tensor_##fname##_##name##_k8_kernel}
        {CG_REGION_ROW(nearest, u8), CG_REGION_ROW(nearest, f16), CG_REGION_ROW(nearest, bf16), CG_REGION_ROW(nearest, f32)},
        {CG_REGION_ROW(bilinear, u8), CG_REGION_ROW(bilinear, f16), CG_REGION_ROW(bilinear, bf16), CG_REGION_ROW(bilinear, f32)},
        {CG_REGION_ROW(antialias, u8), CG_REGION_ROW(antialias, f16), CG_REGION_ROW(antialias, bf16), CG_REGION_ROW(antialias, f32)}};
    RegionPack t;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(slots) * sizeof(RegionSlot) || !plan_region_pack(t, blocks, slots, spec, resize, pad, dst))
        return hipErrorInvalidValue;
    t.slots = device_blob;
    t.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    const uint32_t fi = (resize.filter & COMPEG_RESIZE_ANTIALIAS) ? 2u : resize.filter;
    hipLaunchKernelGGL(kernels[fi][spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

} // namespace compeg
