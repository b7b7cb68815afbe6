// What the lane-per-interval kernels share (kernels.hip, planes_kernels.hip, reduced_kernels.hip): the prologue of the
// ones that stage a wave's whole window, the launch over the grid (workgroups per image, images), and the map from a
// luma sampling to a row of a family's kernel table.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_body.h"
#include "kernels.h"

namespace compeg {

// LDS layout (dynamic, 16-byte aligned carve-outs):
//   [L1: 5*256 u16][L2: l2_in_lds u16][per wave: window_words u32 | 64 DU slots]
// The wave's window loads are issued first and the LUT copy runs under their latency; a wave past the image's last
// interval leaves behind the barrier, lanes past it in a partly used wave stay (quad exchange, quad stores).
// body(d, s, interval, lane): what a lane then does with its restart interval.
// SLOT: bytes of a lane's data-unit slot (the plan's: plan_huffman's slot_bytes).
template <int SLOT = kDuSlotBytes, class Body>
__device__ __forceinline__ void whole_window_kernel(const ImageDesc *__restrict__ descs, uint32_t l2_in_lds, uint32_t window_words, Body body)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ImageDesc &d = descs[blockIdx.y];
    const uint32_t first_interval = blockIdx.x * blockDim.x;
    if (first_interval >= d.total_intervals)
        return;
    uint16_t *l1 = reinterpret_cast<uint16_t *>(smem);
    uint16_t *l2 = l1 + kL1Entries;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * uint32_t(SLOT);
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
    body(d, s, wave_first + lane, lane);
}

// The launch of a lane-per-interval kernel: workgroups of the plan's waves over (the largest image's intervals, images)
// with the plan's LDS; args: what the kernel takes between descs and (l2_in_lds, window_words).
template <class Kernel, class... Args>
hipError_t launch_interval_grid(Kernel kernel, const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan,
                                hipStream_t stream, const Args &...args)
{
    if (images == 0 || max_intervals == 0)
        return hipSuccess;
    const uint32_t threads = plan.waves_per_block * kWave;
    dim3 grid((max_intervals + threads - 1) / threads, images, 1);
    const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                int(device_limits().lds_bytes));
    if (attr != hipSuccess)
        return attr;
    hipLaunchKernelGGL(kernel, grid, dim3(threads), plan.total_bytes, stream, descs, args..., plan.l2_entries_in_lds, plan.window_words);
    return hipGetLastError();
}

// Row of a family's kernel table for the luma sampling hs x vs (1 x 0: grayscale images), or kSamplings: no kernel.
enum : uint32_t { kSampling422, kSampling444, kSampling440, kSampling420, kSamplingGray, kSamplings };
inline uint32_t sampling_index(uint32_t hs, uint32_t vs)
{
    return hs == 2 && vs == 1 ? kSampling422 : hs == 1 && vs == 1 ? kSampling444 : hs == 1 && vs == 2 ? kSampling440
           : hs == 2 && vs == 2 ? kSampling420 : hs == 1 && vs == 0 ? kSamplingGray : kSamplings;
}

} // namespace compeg
