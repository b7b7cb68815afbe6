// gfx950 kernels of the planes decode (lane body in planes_body.h, design in DESIGN.md 5.16): one kernel per sampling
// the front end accepts, each the whole-window prologue (whole_window.h) in front of decode_wave_planes -- grid
// (workgroups per image, images), a lane per restart interval, global reads beyond the window cap: any interval length,
// a file without DRI is one lane.  The format is a kernel argument, not a template axis.
#include <hip/hip_runtime.h>

#include "planes_body.h"
#include "whole_window.h"

namespace compeg {

template <int HS, int VS>
__device__ __forceinline__ void planes_kernel_body(const ImageDesc *__restrict__ descs, const PlanesTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    whole_window_kernel(descs, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
        decode_wave_planes<HS, VS>(d, s, g, g.dst + uint64_t(blockIdx.y) * g.image_stride, interval, lane);
    });
}

// 4:2:2 and 4:2:0 hold four and six data units of samples a lane: the bounds of their RGBA kernels (three and two waves
// to a SIMD); the 8-pixel-MCU samplings and grayscale three.
__global__ void __launch_bounds__(768)
decode_planes_422_kernel(const ImageDesc *__restrict__ descs, PlanesTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    planes_kernel_body<2, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_planes_444_kernel(const ImageDesc *__restrict__ descs, PlanesTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    planes_kernel_body<1, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_planes_440_kernel(const ImageDesc *__restrict__ descs, PlanesTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    planes_kernel_body<1, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(512)
decode_planes_420_kernel(const ImageDesc *__restrict__ descs, PlanesTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    planes_kernel_body<2, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(768)
decode_planes_gray_kernel(const ImageDesc *__restrict__ descs, PlanesTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    planes_kernel_body<1, 0>(descs, g, l2_in_lds, window_words);
}

// Waves per workgroup the planner may choose (plan_huffman's wave_cap): what the launch bounds above hold on a CU in
// one workgroup.  A first choice, not tuned.
uint32_t planes_wave_cap(uint32_t hs, uint32_t vs) { return hs == 2 && vs == 2 ? 8u : 12u; }

hipError_t launch_planes(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const PlanesTarget &target, hipStream_t stream)
{
    static constexpr void (*kKernels[kSamplings])(const ImageDesc *, PlanesTarget, uint32_t, uint32_t) = {
        decode_planes_422_kernel, decode_planes_444_kernel, decode_planes_440_kernel, decode_planes_420_kernel, decode_planes_gray_kernel};
    const uint32_t sampling = sampling_index(hs, vs);
    if (sampling == kSamplings || plan.waves_per_block > planes_wave_cap(hs, vs))
        return hipErrorInvalidValue;
    return launch_interval_grid(kKernels[sampling], descs, images, max_intervals, plan, stream, target);
}

} // namespace compeg
