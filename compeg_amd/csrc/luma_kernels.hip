// The luma_tensor_* kernels (luma_body.h): one kernel per element type and downscale factor, like the orient_tensor_*
// ones, whose grid and records they use; a slot is one plane, the weighted sum of R, G and B.  No LDS, no lane exchange;
// compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "luma_body.h"

namespace compeg {

// Grid: flat over (slot, item) -- blocks_per_slot workgroups for every slot, one behind the other in x.
#define CG_LUMA_KERNEL(name, DTYPE, K)                                                               \
    __global__ void __launch_bounds__(kTensorThreads) luma_tensor_##name##_k##K##_kernel(LumaPack n) \
    {                                                                                                \
        luma_tensor_block_lane<DTYPE, K, kFilterBand>(n, blockIdx.x, threadIdx.x);                   \
    }
#define CG_LUMA_KERNELS(name, DTYPE) \
    CG_LUMA_KERNEL(name, DTYPE, 1)   \
    CG_LUMA_KERNEL(name, DTYPE, 2)   \
    CG_LUMA_KERNEL(name, DTYPE, 4)   \
    CG_LUMA_KERNEL(name, DTYPE, 8)

CG_LUMA_KERNELS(u8, COMPEG_TENSOR_U8)
CG_LUMA_KERNELS(f16, COMPEG_TENSOR_F16)
CG_LUMA_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_LUMA_KERNELS(f32, COMPEG_TENSOR_F32)

using LumaKernel = void (*)(LumaPack);

hipError_t launch_luma_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                              const compeg_filter_spec &filter, const compeg_luma_spec &luma, bool upright, bool transposed, const float *pad,
                              void *dst, hipStream_t stream)
{
    static const LumaKernel kernels[4][4] = {
#define CG_LUMA_ROW(name) \
    {luma_tensor_##name##_k1_kernel, luma_tensor_##name##_k2_kernel, luma_tensor_##name##_k4_kernel, luma_tensor_##name##_k8_kernel}
        CG_LUMA_ROW(u8), CG_LUMA_ROW(f16), CG_LUMA_ROW(bf16), CG_LUMA_ROW(f32)};
    LumaPack n;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(slots) * sizeof(OrientSlot) ||
        !plan_luma_pack(n, blocks, slots, spec, filter, luma, pad, dst, kFilterBand, upright, transposed))
        return hipErrorInvalidValue;
    n.f.slots = device_blob;
    n.f.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, n);
    return hipGetLastError();
}

} // namespace compeg
