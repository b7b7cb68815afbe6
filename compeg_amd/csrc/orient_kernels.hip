// The orient_tensor_* kernels (orient_body.h): one kernel per element type and downscale factor, like the filter_tensor_*
// ones, whose lane they run in the coordinates of the stored raster; the stores go through the slot's orientation.  No LDS,
// no lane exchange; compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "orient_body.h"

namespace compeg {

// Grid: flat over (slot, item) -- blocks_per_slot workgroups for every slot, one behind the other in x.
#define CG_ORIENT_KERNEL(name, DTYPE, K)                                                                \
    __global__ void __launch_bounds__(kTensorThreads) orient_tensor_##name##_k##K##_kernel(FilterPack t) \
    {                                                                                                   \
        orient_tensor_block_lane<DTYPE, K, kFilterBand>(t, blockIdx.x, threadIdx.x);                    \
    }
#define CG_ORIENT_KERNELS(name, DTYPE) \
    CG_ORIENT_KERNEL(name, DTYPE, 1)   \
    CG_ORIENT_KERNEL(name, DTYPE, 2)   \
    CG_ORIENT_KERNEL(name, DTYPE, 4)   \
    CG_ORIENT_KERNEL(name, DTYPE, 8)

CG_ORIENT_KERNELS(u8, COMPEG_TENSOR_U8)
CG_ORIENT_KERNELS(f16, COMPEG_TENSOR_F16)
CG_ORIENT_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_ORIENT_KERNELS(f32, COMPEG_TENSOR_F32)

using OrientKernel = void (*)(FilterPack);

static_assert(sizeof(OrientSlot) == kOrientRecordBytes, "kernels.h states the record's size");
bool make_orient_blob(std::vector<uint32_t> &blob, size_t &tables_at, const OrientSource *sources, uint32_t slots, uint32_t k,
                      uint32_t kernel, uint32_t ow, uint32_t oh)
{
    size_t axes = 0;
    return plan_orient_slots(blob, tables_at, axes, sources, slots, k, kernel, ow, oh);
}

bool orient_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter, bool upright, bool transposed)
{
    FilterPack t;
    uint32_t blocks = 0;
    return plan_orient_pack(t, blocks, slots, spec, filter, nullptr, nullptr, kFilterBand, upright, transposed);
}

hipError_t launch_orient_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_filter_spec &filter, bool upright, bool transposed, const float *pad, void *dst,
                                hipStream_t stream)
{
    static const OrientKernel kernels[4][4] = {
#define CG_ORIENT_ROW(name) \
    {orient_tensor_##name##_k1_kernel, orient_tensor_##name##_k2_kernel, orient_tensor_##name##_k4_kernel, orient_tensor_##name##_k8_kernel}
        CG_ORIENT_ROW(u8), CG_ORIENT_ROW(f16), CG_ORIENT_ROW(bf16), CG_ORIENT_ROW(f32)};
    FilterPack t;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(slots) * sizeof(OrientSlot) ||
        !plan_orient_pack(t, blocks, slots, spec, filter, pad, dst, kFilterBand, upright, transposed))
        return hipErrorInvalidValue;
    t.slots = device_blob;
    t.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

} // namespace compeg
