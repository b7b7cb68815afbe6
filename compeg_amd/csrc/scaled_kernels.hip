// gfx950 kernels of the scaled (1/2- and 1/4-scale) decode (lane body in scaled_body.h, design in DESIGN.md 5.19): one
// kernel per sampling the front end accepts and per transform size N (4: 1/2 scale, 2: 1/4 scale), each the whole-window
// prologue (whole_window.h) in front of decode_wave_scaled -- grid (workgroups per image, images), a lane per restart
// interval, global reads beyond the window cap: any interval length, a file without DRI is one lane.  N is a template
// axis, not a kernel argument: the samples a lane keeps per MCU are N * N bytes a data unit in registers, whose count
// and indices must be known when compiled, and each N gets the register allocation -- and so the launch bounds -- its
// own samples need (as compiled, the same for both: see below).  The format is a kernel argument.
#include <hip/hip_runtime.h>

#include "scaled_body.h"
#include "whole_window.h"

namespace compeg {

template <int HS, int VS, int N>
__device__ __forceinline__ void scaled_kernel_body(const ImageDesc *__restrict__ descs, const ScaledTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    whole_window_kernel(descs, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
        decode_wave_scaled<HS, VS, N>(d, s, g, g.dst + uint64_t(blockIdx.y) * g.image_stride, interval, lane);
    });
}

// Waves per workgroup the planner may choose (plan_huffman's wave_cap), and the kernels' launch bounds.  Beside the
// entropy walk's registers a lane holds N * N bytes per data unit of its MCU -- up to 6 registers at N = 2, up to 24 at
// N = 4 (4:2:0) -- and, in the transform and the store, sixteen values or a row of up to eight pixels for a moment.
// The walk's peak lies inside entropy_data_unit, where neither the transform's values nor the row are alive, and it
// leaves room: under the reduced kernels' bounds of sixteen waves (128 registers, four waves a SIMD) all ten kernels
// come out at 112 registers, no private memory, no spills (tests/test_scaled_code_objects.py prints the counts).  So
// both sizes take the sixteen waves; were N = 4 ever to outgrow 128 registers, eight waves are this function's to say.
// What a CU really holds is the LDS's to say.  A first choice, not tuned.
constexpr uint32_t scaled_waves(int) { return 16u; }
uint32_t scaled_wave_cap(uint32_t, uint32_t, uint32_t n) { return scaled_waves(int(n)); }

template <int N>
__global__ void __launch_bounds__(scaled_waves(N) * kWave)
decode_scaled_422_kernel(const ImageDesc *__restrict__ descs, ScaledTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    scaled_kernel_body<2, 1, N>(descs, g, l2_in_lds, window_words);
}
template <int N>
__global__ void __launch_bounds__(scaled_waves(N) * kWave)
decode_scaled_444_kernel(const ImageDesc *__restrict__ descs, ScaledTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    scaled_kernel_body<1, 1, N>(descs, g, l2_in_lds, window_words);
}
template <int N>
__global__ void __launch_bounds__(scaled_waves(N) * kWave)
decode_scaled_440_kernel(const ImageDesc *__restrict__ descs, ScaledTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    scaled_kernel_body<1, 2, N>(descs, g, l2_in_lds, window_words);
}
template <int N>
__global__ void __launch_bounds__(scaled_waves(N) * kWave)
decode_scaled_420_kernel(const ImageDesc *__restrict__ descs, ScaledTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    scaled_kernel_body<2, 2, N>(descs, g, l2_in_lds, window_words);
}
template <int N>
__global__ void __launch_bounds__(scaled_waves(N) * kWave)
decode_scaled_gray_kernel(const ImageDesc *__restrict__ descs, ScaledTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    scaled_kernel_body<1, 0, N>(descs, g, l2_in_lds, window_words);
}

hipError_t launch_scaled(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const ScaledTarget &target, hipStream_t stream)
{
    using Kernel = void (*)(const ImageDesc *, ScaledTarget, uint32_t, uint32_t);
    static constexpr Kernel kKernels[2][kSamplings] = {
        {decode_scaled_422_kernel<4>, decode_scaled_444_kernel<4>, decode_scaled_440_kernel<4>, decode_scaled_420_kernel<4>, decode_scaled_gray_kernel<4>},
        {decode_scaled_422_kernel<2>, decode_scaled_444_kernel<2>, decode_scaled_440_kernel<2>, decode_scaled_420_kernel<2>, decode_scaled_gray_kernel<2>}};
    const uint32_t sampling = sampling_index(hs, vs);
    if (sampling == kSamplings || (target.n != 4u && target.n != 2u) || plan.waves_per_block > scaled_wave_cap(hs, vs, target.n))
        return hipErrorInvalidValue;
    return launch_interval_grid(kKernels[target.n == 4u ? 0 : 1][sampling], descs, images, max_intervals, plan, stream, target);
}

} // namespace compeg
