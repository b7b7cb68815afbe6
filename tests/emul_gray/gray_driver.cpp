// Host-side run of the fused grayscale kernels' lane body (compeg_amd/csrc/gray_body.h) for sanitizer runs (TEST ONLY).
//
// A stand-alone program: g++ -fsanitize=address,undefined compiles the body the GPU lanes execute together with the host
// front end, and main() drives decode_fused_gray_kernel / decode_fused_gray_single_kernel the way tests/emul/emul.cpp
// drives the layouts' kernels: workgroup by workgroup, the 64 lanes of a wave data unit by data unit and through the
// quad exchange of the composite phase by phase, with a heap block filled with 0xA5 standing in for LDS and exact-size
// heap copies of the words, the start positions and the LUTs.  The output lies between two runs of sentinel bytes inside
// one block; the whole block is written out for the test to look at.
//
//   gray_driver in.jpg out.bin flags waves_per_block window_words single tex_w tex_h pitch alloc_h [luts [control]]
//
// flags: COMPEG_PARSE_*; single: 1 = the single-MCU form whatever the restart interval (0: pairs from two MCUs an
// interval on, as the runtime dispatches); pitch x alloc_h: what lies behind the output pointer (bytes x rows).
// luts, control: how many LUT entries are staged behind L1 and the control that ignores it (tests/emul/lut_budget.h);
// default: what the planner stages, the direct AC tables counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../compeg_amd/csrc/device_types.h"
#include "../../compeg_amd/csrc/front.h"
#include "../../compeg_amd/csrc/gray_body.h"
#include "../../compeg_amd/csrc/scan.h"
#include "../emul/lut_budget.h"

namespace compeg {
void fill_desc(const ImageData &img, ImageDesc &d);
}
using namespace compeg;

constexpr size_t kSentinelBytes = 256;
constexpr uint8_t kSentinel = 0x5c, kPrefill = 0x3c;

template <int MC>
static void run_wave(const ImageDesc &d, const HuffShared &sh, uint32_t wave_first)
{
    uint8_t *slots = sh.du_slots;
    std::vector<EntropyState> es(kWave);
    std::vector<GrayPixels<MC>> ps(kWave);
    std::vector<McuTarget> tg(kWave);
    std::vector<int32_t> dcs(kWave);
    for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
        zero_slot(slots + lane * kDuSlotBytes);
        const bool active = wave_first + lane < d.total_intervals;
        const uint32_t iv = active ? wave_first + lane : d.total_intervals - 1u;
        entropy_init(es[lane], d, sh, iv);
        gray_init<MC>(ps[lane], d, iv, active);
    }
    const uint32_t mcus = d.restart_interval;
    for (uint32_t mcu = 0, place = 0; mcu < mcus; mcu++) {
        for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
            dcs[lane] = entropy_data_unit(es[lane], d, sh, 0u, reinterpret_cast<int16_t *>(slots + lane * kDuSlotBytes));
        for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
            gray_transform<MC>(ps[lane], d, place, slots + lane * kDuSlotBytes, dcs[lane]);
        const bool alone = MC == 2 && mcu + 1u == mcus && place != uint32_t(MC - 1); // (decode_wave_fused_gray)
        if (place != uint32_t(MC - 1) && !alone) {
            place++;
            continue;
        }
        place = 0;
        // composite_gray_mcus, phase by phase
        bool all_whole = !alone; // (the kernel's ballot: every group of the wave whole)
        for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
            tg[lane] = gray_target<MC>(ps[lane], d);
            all_whole = all_whole && tg[lane].whole;
        }
        const bool across = MC == 2 && ((d.width_mcus | d.restart_interval) & 1u) != 0u;
        for (int row = 0; row < 8; row++) {
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
                gray_row_to_slot<MC>(ps[lane], row, slots + lane * kDuSlotBytes);
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
                const uint32_t quad = lane & ~3u;
                uint8_t *bases[4];
                uint32_t limits = 0, pair_lims[4] = {0, 0, 0, 0};
                for (uint32_t j = 0; j < 4; j++) {
                    bases[j] = tg[quad + j].base;
                    if constexpr (MC == 2)
                        pair_lims[j] = gray_pair_limits(ps[quad + j], d, tg[quad + j].whole, alone);
                    else
                        limits |= (tg[quad + j].whole ? 8u | uint32_t(2 * MC) << 5 : gray_limit<MC>(ps[quad + j], d)) << (8u * j);
                }
                if (all_whole) {
                    if (across)
                        layout_row_from_quad<2 * MC, true>(d, slots, lane, uint32_t(row), bases, 0xfu);
                    else
                        layout_row_from_quad<2 * MC, 2 * MC != 4>(d, slots, lane, uint32_t(row), bases, 0xfu);
                } else if constexpr (MC == 2) {
                    for (uint32_t j = 0; j < 4 && (lane & 2u); j++)
                        bases[j] += gray_pair_second_offset(ps[quad + j], d);
                    layout_row_from_quad_cut<2 * MC>(d, slots, lane, uint32_t(row), bases, pair_rows_for_lane(pair_lims, lane & 3u));
                } else {
                    layout_row_from_quad_cut<2 * MC>(d, slots, lane, uint32_t(row), bases, cut_rows_for_piece(limits, lane & 1u));
                }
            }
        }
        for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
            zero_slot(slots + lane * kDuSlotBytes);
            if (gray_is_edge<MC>(ps[lane], d, tg[lane].whole, alone))
                composite_gray_edge<MC>(ps[lane], d, alone ? 1u : uint32_t(MC));
            gray_next_group<MC>(ps[lane], d);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 11 || argc > 11 + 2) {
        fprintf(stderr, "usage: %s in.jpg out.bin flags waves window_words single tex_w tex_h pitch alloc_h [luts [control]]\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        file.insert(file.end(), buf, buf + n);
    fclose(f);
    // exact-size copy: reads past the end of the file are the sanitizer's to report
    uint8_t *jpeg = static_cast<uint8_t *>(malloc(file.size() ? file.size() : 1));
    memcpy(jpeg, file.data(), file.size());
    const unsigned flags = unsigned(atoi(argv[3]));
    const uint32_t waves_per_block = uint32_t(atoi(argv[4]));
    uint32_t window_words = (uint32_t(atoi(argv[5])) + 3u) & ~3u;
    const bool single = atoi(argv[6]) != 0;
    const uint32_t tex_w = uint32_t(atoi(argv[7])), tex_h = uint32_t(atoi(argv[8])), pitch = uint32_t(atoi(argv[9])), alloc_h = uint32_t(atoi(argv[10]));

    ImageData *img = nullptr;
    Status s = ImageData::parse(jpeg, file.size(), false, &img, flags);
    if (!s.ok()) {
        printf("error: %s\n", s.message.c_str());
        free(jpeg);
        return 1;
    }
    if (img->components != 1) {
        printf("error: not a grayscale image\n");
        delete img;
        free(jpeg);
        return 1;
    }
    ScanBuffer scan;
    Status pre = scan.process(img->scan_data(), img->scan_len, img->metadata.total_restart_intervals);
    if (!pre.ok() && pre.code != COMPEG_E_COUNT_MISMATCH) {
        printf("error: %s\n", pre.message.c_str());
        delete img;
        free(jpeg);
        return 1;
    }
    ImageDesc d;
    fill_desc(*img, d);
    if (d.dus_per_mcu != 1u || d.mcu_w != 8u || d.mcu_h != 8u || d.coop_ok || d.mcu_ok) {
        printf("error: inconsistent descriptor\n");
        return 1;
    }
    std::vector<uint32_t> words(scan.words(), scan.words() + scan.nwords());
    std::vector<uint32_t> starts(scan.starts(), scan.starts() + scan.nstarts());
    std::vector<uint16_t> l1(img->l1, img->l1 + 1024), l2(img->l2);
    // the global LUT blob as the runtime lays it out: L2, padded to a dword, then the direct tables
    if (l2.size() & 1)
        l2.push_back(0);
    l2.insert(l2.end(), img->ac_fast.begin(), img->ac_fast.end());
    l2.insert(l2.end(), img->dc_fast.begin(), img->dc_fast.end());
    const size_t out_bytes = size_t(pitch) * alloc_h;
    std::vector<uint8_t> block(kSentinelBytes + out_bytes + kSentinelBytes, kSentinel);
    memset(block.data() + kSentinelBytes, kPrefill, out_bytes);
    d.words = words.data();
    d.starts = starts.data();
    d.nwords = uint32_t(words.size());
    d.nstarts = uint32_t(starts.size());
    d.l1 = l1.data();
    d.l2 = l2.data();
    d.out = block.data() + kSentinelBytes;
    d.out_w = tex_w;
    d.out_h = tex_h;
    d.out_alloc_h = alloc_h;
    d.out_pitch = pitch;

    const LutBudget luts(argc, argv, 11);
    luts.apply(d);
    const uint32_t l2_in_lds = luts.in_lds(*img);
    luts.report(d, l2_in_lds);
    const uint32_t threads = waves_per_block * kWave;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    const uint32_t lds_bytes = align16((kL1Entries + l2_in_lds) * 2u) + waves_per_block * wave_area;
    const bool pairs = !single && d.restart_interval >= 2u;
    for (uint32_t first = 0; first < d.total_intervals; first += threads) {
        uint8_t *smem = static_cast<uint8_t *>(aligned_alloc(16, align16(luts.alloc_bytes(lds_bytes))));
        memset(smem, 0xa5, luts.alloc_bytes(lds_bytes)); // LDS is not zero-initialised
        uint16_t *sl1 = reinterpret_cast<uint16_t *>(smem);
        uint16_t *sl2 = sl1 + kL1Entries;
        uint8_t *wave_base = smem + align16((kL1Entries + l2_in_lds) * 2u);
        for (uint32_t tid = 0; tid < threads; tid++)
            stage_luts(d, sl1, sl2, l2_in_lds, tid, threads);
        for (uint32_t wave = 0; wave < waves_per_block; wave++) {
            uint32_t *win = reinterpret_cast<uint32_t *>(wave_base + wave * wave_area);
            uint8_t *slots = reinterpret_cast<uint8_t *>(win) + align16(window_words * 4u);
            const uint32_t wave_first = first + wave * kWave;
            if (wave_first >= d.total_intervals)
                continue;
            uint32_t wb = 0, wl = 0;
            wave_window(d, wave_first, window_words, wb, wl);
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
                stage_window(d, win, wb, wl, lane);
            HuffShared sh{sl1, sl2, luts.l2_staged(d, l2_in_lds), win, wb, wl, slots};
            if (pairs)
                run_wave<2>(d, sh, wave_first);
            else
                run_wave<1>(d, sh, wave_first);
        }
        free(smem);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    fwrite(block.data(), 1, block.size(), o);
    fclose(o);
    printf("ok %u %u %u %u\n", img->width, img->height, d.total_intervals, d.restart_interval);
    delete img;
    free(jpeg);
    return 0;
}
