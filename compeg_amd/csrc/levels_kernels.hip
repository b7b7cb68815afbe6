// gfx950 kernels of the levels decode (lane body in levels_body.h, design in DESIGN.md 5.20): one kernel per sampling
// the front end accepts, each the whole-window prologue (whole_window.h) with slots of kLevelsSlotBytes in front of
// decode_wave_levels -- grid (workgroups per image, images), a lane per restart interval, global reads beyond the
// window cap: any interval length, a file without DRI is one lane.  The order is a kernel argument, not a template axis.
#include <hip/hip_runtime.h>

#include "levels_body.h"
#include "whole_window.h"

namespace compeg {

template <int HS, int VS>
__device__ __forceinline__ void levels_kernel_body(const ImageDesc *__restrict__ descs, const LevelsTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    whole_window_kernel<kLevelsSlotBytes>(descs, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
        decode_wave_levels<HS, VS>(d, s, g, g.dst + uint64_t(blockIdx.y) * g.image_stride, interval, lane);
    });
}

// A lane holds nothing of a data unit outside its slot: the entropy walk's registers and a block's place -- the bounds
// of sixteen waves (128 registers), as for the reduced kernels.  What a CU really holds is the LDS's to say
// (levels_wave_cap).
__global__ void __launch_bounds__(1024)
decode_levels_422_kernel(const ImageDesc *__restrict__ descs, LevelsTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    levels_kernel_body<2, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_levels_444_kernel(const ImageDesc *__restrict__ descs, LevelsTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    levels_kernel_body<1, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_levels_440_kernel(const ImageDesc *__restrict__ descs, LevelsTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    levels_kernel_body<1, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_levels_420_kernel(const ImageDesc *__restrict__ descs, LevelsTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    levels_kernel_body<2, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_levels_gray_kernel(const ImageDesc *__restrict__ descs, LevelsTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    levels_kernel_body<1, 0>(descs, g, l2_in_lds, window_words);
}

// Waves per workgroup the planner may choose (plan_huffman's wave_cap): the reduced kernels' choice.  With 17 KB of
// tables and 16 KB a wave (7 KB of window at 4K DRI 4, 9 KB of slots) the 160 KB of LDS hold eight; short windows let
// the planner go higher.  A first choice, not tuned.
uint32_t levels_wave_cap() { return 16u; }

hipError_t launch_levels(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const LevelsTarget &target, hipStream_t stream)
{
    static constexpr void (*kKernels[kSamplings])(const ImageDesc *, LevelsTarget, uint32_t, uint32_t) = {
        decode_levels_422_kernel, decode_levels_444_kernel, decode_levels_440_kernel, decode_levels_420_kernel, decode_levels_gray_kernel};
    const uint32_t sampling = sampling_index(hs, vs);
    if (sampling == kSamplings || plan.waves_per_block > levels_wave_cap())
        return hipErrorInvalidValue;
    return launch_interval_grid(kKernels[sampling], descs, images, max_intervals, plan, stream, target);
}

} // namespace compeg
