// How many LUT entries the stand-alone drivers of the lane-per-interval bodies stage in their "LDS" behind L1 (TEST ONLY):
// tests/emul_reduced, _planes, _gray, _crop, _crop_regions, _scaled, _levels.
//
// Two optional arguments behind a driver's own:
//
//   budget   "plan" (the default): what the planner is given and makes of it -- runtime.cpp: staged_lut_entries, the L2
//            LUT padded to a dword PLUS the two direct AC tables; kernels.hip: plan_huffman, at most 12288 entries.  With
//            ordinary tables s.l2_staged then reaches d.fast_off + 2 * kFastEntries and the fast entropy mode is on, as
//            it is on the card.  A number: that many entries.
//   control  "beyond": the body is told s.l2_staged = UINT32_MAX while the budget's entries are staged, as a kernel would
//            that forgot `idx >= s.l2_staged` -- every L2 lookup goes to "LDS", and beyond the staged entries finds what
//            lies there (wave windows, slots, 0xA5).  A frame that decodes to its expectation all the same never looks
//            up beyond the boundary.  The allocation is made large enough for any 15-bit index, so that the sanitizer has
//            nothing to say about the control itself, and the direct tables are taken from the body (fast_table = 2, as
//            for an image whose components use no direct table): with tables that outgrow the share they are not
//            staged, and the control is about L2.
//
// The driver reports what it computed on stderr: "luts in_lds=N l2_staged=N fast=0|1" (fast: fast_tables_usable).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../compeg_amd/csrc/device_types.h"
#include "../../compeg_amd/csrc/front.h"
#include "../../compeg_amd/csrc/kernels_body.h"

namespace compeg {

struct LutBudget {
    const char *budget = nullptr;
    bool beyond = false;

    LutBudget(int argc, char **argv, int at)
    {
        budget = argc > at && strcmp(argv[at], "plan") != 0 ? argv[at] : nullptr;
        beyond = argc > at + 1 && strcmp(argv[at + 1], "beyond") == 0;
    }

    // entries staged behind L1 for this image (a batch: the largest of its images')
    uint32_t in_lds(const ImageData &img) const
    {
        if (budget)
            return uint32_t(atoi(budget)) & ~1u;
        const uint32_t staged = uint32_t((img.l2.size() * 2 + 3) / 4 * 2 + img.ac_fast.size()); // runtime.cpp: staged_lut_entries
        return staged < kLutLdsShare ? (staged + 1u) & ~1u : kLutLdsShare;                        // kernels.hip: plan_huffman
    }

    // the control's change to the descriptor
    void apply(ImageDesc &d) const
    {
        if (beyond)
            d.fast_table[0] = d.fast_table[1] = d.fast_table[2] = 2u;
    }

    // what the body is told is staged (kernels.hip: s.l2_staged)
    uint32_t l2_staged(const ImageDesc &d, uint32_t l2_in_lds) const
    {
        return beyond ? UINT32_MAX : umin(l2_in_lds, d.fast_off + 2u * kFastEntries);
    }

    // bytes to allocate for an "LDS" of lds_bytes
    uint32_t alloc_bytes(uint32_t lds_bytes) const
    {
        const uint32_t any_index = (kL1Entries + 0x8000u + 256u) * 2u;
        return beyond && lds_bytes < any_index ? any_index : lds_bytes;
    }

    void report(const ImageDesc &d, uint32_t l2_in_lds) const
    {
        HuffShared probe{};
        probe.l2_staged = l2_staged(d, l2_in_lds);
        fprintf(stderr, "luts in_lds=%u l2_staged=%u fast=%d\n", l2_in_lds, probe.l2_staged, int(fast_tables_usable(d, probe)));
    }
};

} // namespace compeg
