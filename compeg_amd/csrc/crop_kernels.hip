// gfx950 kernels of the cropped decode (lane body in crop_body.h, design in DESIGN.md 5.18): one kernel per sampling the
// front end accepts, each a whole-window prologue in front of decode_wave_cropped -- grid (workgroups per image, images)
// as launch_interval_grid lays it, a lane per restart interval, global reads beyond the window cap: any interval length,
// a file without DRI is one lane.  The format is a kernel argument, not a template axis.
#include <hip/hip_runtime.h>

#include "crop_window.h"

namespace compeg {

template <int HS, int VS>
__device__ __forceinline__ void cropped_kernel_body(const ImageDesc *__restrict__ descs, const CropTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    crop_window_kernel(descs, blockIdx.y, g, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
        decode_wave_cropped<HS, VS>(d, s, g, g.dst + uint64_t(blockIdx.y) * g.image_stride, interval, lane);
    });
}

// A lane holds an MCU's samples as the planes kernels' lanes do (four data units for 4:2:2, six for 4:2:0): their bounds.
__global__ void __launch_bounds__(768)
decode_cropped_422_kernel(const ImageDesc *__restrict__ descs, CropTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_kernel_body<2, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_444_kernel(const ImageDesc *__restrict__ descs, CropTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_kernel_body<1, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_440_kernel(const ImageDesc *__restrict__ descs, CropTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_kernel_body<1, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(512)
decode_cropped_420_kernel(const ImageDesc *__restrict__ descs, CropTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_kernel_body<2, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_cropped_gray_kernel(const ImageDesc *__restrict__ descs, CropTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    cropped_kernel_body<1, 0>(descs, g, l2_in_lds, window_words);
}

// Waves per workgroup the planner may choose (plan_huffman's wave_cap): what the launch bounds above hold on a CU in
// one workgroup.  A first choice, not tuned.
uint32_t crop_wave_cap(uint32_t hs, uint32_t vs) { return hs == 2 && vs == 2 ? 8u : 12u; }

hipError_t launch_cropped(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                          const CropTarget &target, hipStream_t stream)
{
    static constexpr void (*kKernels[kSamplings])(const ImageDesc *, CropTarget, uint32_t, uint32_t) = {
        decode_cropped_422_kernel, decode_cropped_444_kernel, decode_cropped_440_kernel, decode_cropped_420_kernel, decode_cropped_gray_kernel};
    const uint32_t sampling = sampling_index(hs, vs);
    if (sampling == kSamplings || plan.waves_per_block > crop_wave_cap(hs, vs))
        return hipErrorInvalidValue;
    return launch_interval_grid(kKernels[sampling], descs, images, max_intervals, plan, stream, target);
}

} // namespace compeg
