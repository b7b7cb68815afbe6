// The filter_tensor_* kernels (filter_body.h): one kernel per element type and downscale factor -- box, triangle, bicubic
// and Lanczos differ in their tables only; a lane per output column of a band of kFilterBand rows of a slot.  No LDS, no
// lane exchange; compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "filter_body.h"

namespace compeg {

// Grid: flat over (slot, item) -- blocks_per_slot workgroups for every slot, one behind the other in x.
#define CG_FILTER_KERNEL(name, DTYPE, K)                                                                \
    __global__ void __launch_bounds__(kTensorThreads) filter_tensor_##name##_k##K##_kernel(FilterPack t) \
    {                                                                                                   \
        filter_tensor_block_lane<DTYPE, K, kFilterBand>(t, blockIdx.x, threadIdx.x);                    \
    }
#define CG_FILTER_KERNELS(name, DTYPE) \
    CG_FILTER_KERNEL(name, DTYPE, 1)   \
    CG_FILTER_KERNEL(name, DTYPE, 2)   \
    CG_FILTER_KERNEL(name, DTYPE, 4)   \
    CG_FILTER_KERNEL(name, DTYPE, 8)

CG_FILTER_KERNELS(u8, COMPEG_TENSOR_U8)
CG_FILTER_KERNELS(f16, COMPEG_TENSOR_F16)
CG_FILTER_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_FILTER_KERNELS(f32, COMPEG_TENSOR_F32)

using FilterKernel = void (*)(FilterPack);

static_assert(sizeof(RegionAntialiasSlot) == kRegionRecordBytes, "kernels.h states the record's size");
bool make_filter_blob(std::vector<uint32_t> &blob, size_t &tables_at, const RegionSource *sources, uint32_t slots, uint32_t k, uint32_t kernel)
{
    size_t axes = 0;
    return plan_filter_slots(blob, tables_at, axes, sources, slots, k, kernel);
}

bool filter_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter)
{
    FilterPack t;
    uint32_t blocks = 0;
    return plan_filter_pack(t, blocks, slots, spec, filter, nullptr, nullptr, kFilterBand);
}

hipError_t launch_filter_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_filter_spec &filter, const float *pad, void *dst, hipStream_t stream)
{
    static const FilterKernel kernels[4][4] = {
#define CG_FILTER_ROW(name) \
    {filter_tensor_##name##_k1_kernel, filter_tensor_##name##_k2_kernel, filter_tensor_##name##_k4_kernel, filter_tensor_##name##_k8_kernel}
        CG_FILTER_ROW(u8), CG_FILTER_ROW(f16), CG_FILTER_ROW(bf16), CG_FILTER_ROW(f32)};
    FilterPack t;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(slots) * sizeof(RegionAntialiasSlot) ||
        !plan_filter_pack(t, blocks, slots, spec, filter, pad, dst, kFilterBand))
        return hipErrorInvalidValue;
    t.slots = device_blob;
    t.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

} // namespace compeg
