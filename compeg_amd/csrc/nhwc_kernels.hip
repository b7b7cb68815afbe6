// The nhwc_tensor_* kernels (nhwc_body.h): one kernel per element type and downscale factor, like the orient_tensor_*
// ones, whose lane they run; the stores put a pixel's 3 or 4 channel values next to each other.  No LDS, no lane
// exchange; compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nhwc_body.h"

namespace compeg {

// Grid: flat over (slot, item) -- blocks_per_slot workgroups for every slot, one behind the other in x.
#define CG_NHWC_KERNEL(name, DTYPE, K)                                                               \
    __global__ void __launch_bounds__(kTensorThreads) nhwc_tensor_##name##_k##K##_kernel(NhwcPack n) \
    {                                                                                                \
        nhwc_tensor_block_lane<DTYPE, K, kFilterBand>(n, blockIdx.x, threadIdx.x);                   \
    }
#define CG_NHWC_KERNELS(name, DTYPE) \
    CG_NHWC_KERNEL(name, DTYPE, 1)   \
    CG_NHWC_KERNEL(name, DTYPE, 2)   \
    CG_NHWC_KERNEL(name, DTYPE, 4)   \
    CG_NHWC_KERNEL(name, DTYPE, 8)

CG_NHWC_KERNELS(u8, COMPEG_TENSOR_U8)
CG_NHWC_KERNELS(f16, COMPEG_TENSOR_F16)
CG_NHWC_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_NHWC_KERNELS(f32, COMPEG_TENSOR_F32)

using NhwcKernel = void (*)(NhwcPack);

hipError_t launch_nhwc_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                              const compeg_filter_spec &filter, const compeg_nhwc_spec &nhwc, bool upright, bool transposed, const float *pad,
                              void *dst, hipStream_t stream)
{
    static const NhwcKernel kernels[4][4] = {
#define CG_NHWC_ROW(name) \
    {nhwc_tensor_##name##_k1_kernel, nhwc_tensor_##name##_k2_kernel, nhwc_tensor_##name##_k4_kernel, nhwc_tensor_##name##_k8_kernel}
        CG_NHWC_ROW(u8), CG_NHWC_ROW(f16), CG_NHWC_ROW(bf16), CG_NHWC_ROW(f32)};
    NhwcPack n;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(slots) * sizeof(OrientSlot) ||
        !plan_nhwc_pack(n, blocks, slots, spec, filter, nhwc, pad, dst, kFilterBand, upright, transposed))
        return hipErrorInvalidValue;
    n.f.slots = device_blob;
    n.f.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, n);
    return hipGetLastError();
}

} // namespace compeg
