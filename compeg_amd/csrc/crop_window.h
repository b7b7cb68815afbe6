// The prologue of the cropped kernels (crop_kernels.hip, crop_regions_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "crop_body.h"
#include "whole_window.h"

namespace compeg {

// whole_window_kernel (whole_window.h: the LDS layout, the order of loads) with the touch test in front of everything
// that costs: a workgroup none of whose intervals touch the rectangle's box returns before it stages anything; a wave
// none of whose 64 do issues no window loads, helps with the LUT copy and leaves behind the barrier, as a wave past the
// image's last interval does.  DRI is the image's own (ImageDesc::restart_interval), so the test is made here and not
// where the grid is laid.  A sibling, not a predicate of the shared prologue's: the other families' code stays what it was.
// image: the image of this row of the grid (the one-rectangle kernels: blockIdx.y; a region list: its record's).
template <class Body>
__device__ __forceinline__ void crop_window_kernel(const ImageDesc *__restrict__ descs, uint32_t image, const CropTarget &g, uint32_t l2_in_lds,
                                                   uint32_t window_words, Body body)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const ImageDesc &d = descs[image];
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

} // namespace compeg
