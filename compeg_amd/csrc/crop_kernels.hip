// gfx950 kernels of the cropped decode (lane body in crop_body.h, design in DESIGN.md 5.18): one kernel per sampling the
// front end accepts, each a whole-window prologue in front of decode_wave_cropped -- grid (workgroups per image, images)
// as launch_interval_grid lays it, a lane per restart interval, global reads beyond the window cap: any interval length,
// a file without DRI is one lane.  The format is a kernel argument, not a template axis.
#include <hip/hip_runtime.h>

#include "crop_body.h"
#include "whole_window.h"

namespace compeg {

// whole_window_kernel (whole_window.h: the LDS layout, the order of loads) with the touch test in front of everything
// that costs: a workgroup none of whose intervals touch the rectangle's box returns before it stages anything; a wave
// none of whose 64 do issues no window loads, helps with the LUT copy and leaves behind the barrier, as a wave past the
// image's last interval does.  DRI is the image's own (ImageDesc::restart_interval), so the test is made here and not
// where the grid is laid.  A sibling, not a predicate of the shared prologue's: the other families' code stays what it was.
template <class Body>
__device__ __forceinline__ void crop_window_kernel(const ImageDesc *__restrict__ descs, const CropTarget &g, uint32_t l2_in_lds, uint32_t window_words,
                                                   Body body)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ImageDesc &d = descs[blockIdx.y];
    const uint32_t first_interval = blockIdx.x * blockDim.x;
    if (first_interval >= d.total_intervals)
        return;
    if (crop_intervals_reach(d, g, first_interval, blockDim.x) == 0u)
        return; // the whole workgroup
    uint16_t *l1 = reinterpret_cast<uint16_t *>(smem);
    uint16_t *l2 = l1 + kL1Entries;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    uint8_t *wave_base = smem + align16((kL1Entries + l2_in_lds) * 2u);
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x / kWave))), lane = threadIdx.x % kWave;
    uint32_t *win = reinterpret_cast<uint32_t *>(wave_base + wave * wave_area);
    const uint32_t wave_first = first_interval + wave * kWave;
    const bool touched = wave_first < d.total_intervals && crop_intervals_reach(d, g, wave_first, kWave) != 0u;
    uint32_t win_base = 0, win_len = 0;
    if (touched)
        wave_window(d, wave_first, window_words, win_base, win_len);
    stage_luts_and_window(d, l1, l2, l2_in_lds, threadIdx.x, blockDim.x, win, win_base, win_len, lane);
    __syncthreads();
    if (!touched)
        return; // the whole wave
    HuffShared s;
    s.l1 = l1;
    s.l2 = l2;
    s.l2_staged = umin(l2_in_lds, d.fast_off + 2u * kFastEntries);
    s.win = win;
    s.win_base = win_base;
    s.win_len = win_len;
    s.du_slots = reinterpret_cast<uint8_t *>(win) + align16(window_words * 4u);
    body(d, s, wave_first + lane, lane);
}

template <int HS, int VS>
__device__ __forceinline__ void cropped_kernel_body(const ImageDesc *__restrict__ descs, const CropTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    crop_window_kernel(descs, g, l2_in_lds, window_words, [&](const ImageDesc &d, const HuffShared &s, uint32_t interval, uint32_t lane) {
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
