// The pack_tensor_* kernels (tensor_body.h): one streaming kernel per element type and downscale factor, a lane
// per 16-byte run of an output row.  No LDS, no lane exchange; compiled with the library's flags (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "tensor_body.h"

namespace compeg {

// Grid: flat over (image, run) -- blocks_per_image workgroups for every image, one behind the other in x.
#define CG_PACK_KERNEL(name, DTYPE, K)                                                                   \
    __global__ void __launch_bounds__(kTensorThreads) pack_tensor_##name##_k##K##_kernel(TensorPack t)  \
    {                                                                                                    \
        pack_tensor_block_lane<DTYPE, K>(t, blockIdx.x, threadIdx.x);                                   \
    }
#define CG_PACK_KERNELS(name, DTYPE) \
    CG_PACK_KERNEL(name, DTYPE, 1)   \
    CG_PACK_KERNEL(name, DTYPE, 2)   \
    CG_PACK_KERNEL(name, DTYPE, 4)   \
    CG_PACK_KERNEL(name, DTYPE, 8)

CG_PACK_KERNELS(u8, COMPEG_TENSOR_U8)
CG_PACK_KERNELS(f16, COMPEG_TENSOR_F16)
CG_PACK_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_PACK_KERNELS(f32, COMPEG_TENSOR_F32)

using PackKernel = void (*)(TensorPack);

hipError_t launch_pack_tensor(const void *src, size_t src_image_stride, uint32_t src_pitch, uint32_t width, uint32_t height,
                              uint32_t images, const compeg_tensor_spec &spec, void *dst, hipStream_t stream)
{
    static const PackKernel kernels[4][4] = {
#define CG_PACK_ROW(name) \
    {pack_tensor_##name##_k1_kernel, pack_tensor_##name##_k2_kernel, pack_tensor_##name##_k4_kernel, pack_tensor_##name##_k8_kernel}
        CG_PACK_ROW(u8), CG_PACK_ROW(f16), CG_PACK_ROW(bf16), CG_PACK_ROW(f32)};
    TensorPack t;
    uint32_t blocks = 0;
    if (!plan_tensor_pack(t, blocks, src, src_image_stride, src_pitch, width, height, images, spec, dst))
        return hipErrorInvalidValue;
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

} // namespace compeg
