// gfx950 kernels of the reduced (1/8-scale) decode (lane body in reduced_body.h, design in DESIGN.md 5.17): one kernel
// per sampling the front end accepts, each the planes kernels' whole-window prologue (planes_kernels.hip:
// planes_kernel_body) in front of decode_wave_reduced -- grid (workgroups per image, images), a lane per restart
// interval, global reads beyond the window cap: any interval length, a file without DRI is one lane.  The format is a
// kernel argument, not a template axis.
#include <hip/hip_runtime.h>

#include "reduced_body.h"
#include "kernels.h"

namespace compeg {

template <int HS, int VS>
__device__ __forceinline__ void reduced_kernel_body(const ImageDesc *__restrict__ descs, const ReducedTarget &g, uint32_t l2_in_lds, uint32_t window_words)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ImageDesc &d = descs[blockIdx.y];
    const uint32_t first_interval = blockIdx.x * blockDim.x;
    if (first_interval >= d.total_intervals)
        return;
    uint16_t *l1 = reinterpret_cast<uint16_t *>(smem);
    uint16_t *l2 = l1 + kL1Entries;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    uint8_t *wave_base = smem + align16((kL1Entries + l2_in_lds) * 2u);
    const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(threadIdx.x / kWave))), lane = threadIdx.x % kWave;
    uint32_t *win = reinterpret_cast<uint32_t *>(wave_base + wave * wave_area);
    const uint32_t wave_first = first_interval + wave * kWave;
    uint32_t win_base = 0, win_len = 0;
    if (wave_first < d.total_intervals)
        wave_window(d, wave_first, window_words, win_base, win_len);
    stage_luts_and_window(d, l1, l2, l2_in_lds, threadIdx.x, blockDim.x, win, win_base, win_len, lane);
    __syncthreads();
    if (wave_first >= d.total_intervals)
        return; // the whole wave
    HuffShared s;
    s.l1 = l1;
    s.l2 = l2;
    s.l2_staged = umin(l2_in_lds, d.fast_off + 2u * kFastEntries);
    s.win = win;
    s.win_base = win_base;
    s.win_len = win_len;
    s.du_slots = reinterpret_cast<uint8_t *>(win) + align16(window_words * 4u);
    decode_wave_reduced<HS, VS>(d, s, g, g.dst + uint64_t(blockIdx.y) * g.image_stride, wave_first + lane, lane);
}

// A lane holds no samples beyond an MCU's few bytes: the entropy walk's registers alone, which entropy_kernel runs at
// four waves to a SIMD -- the bounds of sixteen waves (128 registers).  What a CU really holds is the LDS's to say
// (reduced_wave_cap).
__global__ void __launch_bounds__(1024)
decode_reduced_422_kernel(const ImageDesc *__restrict__ descs, ReducedTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    reduced_kernel_body<2, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_reduced_444_kernel(const ImageDesc *__restrict__ descs, ReducedTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    reduced_kernel_body<1, 1>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_reduced_440_kernel(const ImageDesc *__restrict__ descs, ReducedTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    reduced_kernel_body<1, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_reduced_420_kernel(const ImageDesc *__restrict__ descs, ReducedTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    reduced_kernel_body<2, 2>(descs, g, l2_in_lds, window_words);
}
__global__ void __launch_bounds__(1024)
decode_reduced_gray_kernel(const ImageDesc *__restrict__ descs, ReducedTarget g, uint32_t l2_in_lds, uint32_t window_words)
{
    reduced_kernel_body<1, 0>(descs, g, l2_in_lds, window_words);
}

// Waves per workgroup the planner may choose (plan_huffman's wave_cap): what the launch bounds above hold on a CU in
// one workgroup.  With 17 KB of tables and 12 KB a wave (7 KB of window at 4K DRI 4, 5 KB of slots) the 160 KB of LDS
// hold eleven; short windows let the planner go up to the sixteen.  A first choice, not tuned.
uint32_t reduced_wave_cap() { return 16u; }

hipError_t launch_reduced(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                          const ReducedTarget &target, hipStream_t stream)
{
    if (images == 0 || max_intervals == 0)
        return hipSuccess;
    using Kernel = void (*)(const ImageDesc *, ReducedTarget, uint32_t, uint32_t);
    const Kernel kernel = hs == 2 && vs == 1   ? decode_reduced_422_kernel
                          : hs == 1 && vs == 1 ? decode_reduced_444_kernel
                          : hs == 1 && vs == 2 ? decode_reduced_440_kernel
                          : hs == 2 && vs == 2 ? decode_reduced_420_kernel
                          : hs == 1 && vs == 0 ? decode_reduced_gray_kernel
                                               : nullptr;
    if (!kernel || plan.waves_per_block > reduced_wave_cap())
        return hipErrorInvalidValue;
    int dev = 0, lds = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess ||
        lds < 64 * 1024)
        lds = 160 * 1024;
    const uint32_t threads = plan.waves_per_block * kWave;
    dim3 grid((max_intervals + threads - 1) / threads, images, 1);
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (attr != hipSuccess)
        return attr;
    hipLaunchKernelGGL(kernel, grid, dim3(threads), plan.total_bytes, stream, descs, target, plan.l2_entries_in_lds, plan.window_words);
    return hipGetLastError();
}

} // namespace compeg
