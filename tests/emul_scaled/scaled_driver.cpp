// Host-side run of the scaled kernels' lane body (compeg_amd/csrc/scaled_body.h) for sanitizer runs (TEST ONLY).
//
// A stand-alone program: g++ -fsanitize=address,undefined compiles the body the GPU lanes execute together with the host
// front end, and main() drives decode_scaled_*_kernel the way tests/emul_reduced/reduced_driver.cpp drives the reduced
// kernels: workgroup by workgroup over a heap block filled with 0xA5 standing in for LDS and exact-size heap copies of
// the words, the start positions and the LUTs.  The store stage is lane-local, so a wave is its 64 lanes one after the
// other, each through the steps of decode_wave_scaled.  The destination lies between two runs of sentinel bytes inside
// one block, pre-filled with 0xA5; the whole block is written out for the test to look at.
//
//   scaled_driver in.jpg out.bin flags waves_per_block window_words format shift ow oh pitch total n [luts [control]]
//
// flags: COMPEG_PARSE_*; format: COMPEG_SCALED_*; shift: bytes the destination begins behind a 16-byte boundary;
// ow, oh, pitch, total: compeg_scaled_shape's answer for the one image; n: 8 / denominator, 4 or 2.
// luts, control: how many LUT entries are staged behind L1 and the control that ignores it (tests/emul/lut_budget.h);
// default: what the planner stages, the direct AC tables counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../compeg_amd/csrc/device_types.h"
#include "../../compeg_amd/csrc/front.h"
#include "../../compeg_amd/csrc/scaled_body.h"
#include "../../compeg_amd/csrc/scan.h"
#include "../emul/lut_budget.h"

namespace compeg {
void fill_desc(const ImageData &img, ImageDesc &d);
}
using namespace compeg;

constexpr size_t kSentinelBytes = 256;
constexpr uint8_t kSentinel = 0x5c, kPrefill = 0xa5;

template <int HS, int VS, int N>
static void run_wave(const ImageDesc &d, const HuffShared &sh, const ScaledTarget &g, uint32_t wave_first)
{
    constexpr uint32_t kDus = uint32_t(ScaledMcu<HS, VS, N>::kDus), kLuma = uint32_t(ScaledMcu<HS, VS, N>::kLuma);
    for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
        uint8_t *slot = sh.du_slots + lane * kDuSlotBytes;
        zero_slot(slot);
        const bool active = wave_first + lane < d.total_intervals;
        const uint32_t iv = active ? wave_first + lane : d.total_intervals - 1u;
        EntropyState e;
        entropy_init(e, d, sh, iv);
        ScaledMcu<HS, VS, N> t;
        scaled_init<HS, VS, N>(t, d, iv, active);
        const uint32_t du_total = d.restart_interval * kDus;
        for (uint32_t du = 0, k = 0; du < du_total; du++) {
            const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
            const int32_t dc = entropy_data_unit(e, d, sh, comp, reinterpret_cast<int16_t *>(slot));
            scaled_unit<HS, VS, N>(t, k, slot, dc, d.quant[comp]);
            if (k == kDus - 1u) {
                scaled_store_mcu<HS, VS, N>(t, g, g.dst);
                scaled_next_mcu<HS, VS, N>(t, d);
                k = 0;
            } else {
                k++;
            }
        }
    }
}

template <int N>
static bool run_wave_of(uint32_t hs, uint32_t vs, const ImageDesc &d, const HuffShared &sh, const ScaledTarget &g, uint32_t wave_first)
{
    if (hs == 2 && vs == 1)
        run_wave<2, 1, N>(d, sh, g, wave_first);
    else if (hs == 1 && vs == 1)
        run_wave<1, 1, N>(d, sh, g, wave_first);
    else if (hs == 1 && vs == 2)
        run_wave<1, 2, N>(d, sh, g, wave_first);
    else if (hs == 2 && vs == 2)
        run_wave<2, 2, N>(d, sh, g, wave_first);
    else if (hs == 1 && vs == 0)
        run_wave<1, 0, N>(d, sh, g, wave_first);
    else
        return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 13 || argc > 13 + 2) {
        fprintf(stderr, "usage: %s in.jpg out.bin flags waves window_words format shift ow oh pitch total n [luts [control]]\n", argv[0]);
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
    const uint32_t window_words = (uint32_t(atoi(argv[5])) + 3u) & ~3u;
    ScaledTarget g{};
    g.format = uint32_t(atoi(argv[6]));
    const size_t shift = size_t(atoi(argv[7]));
    g.ow = uint32_t(atoi(argv[8]));
    g.oh = uint32_t(atoi(argv[9]));
    g.pitch = uint32_t(atoi(argv[10]));
    const size_t total = size_t(atoll(argv[11]));
    g.image_stride = total;
    g.n = uint32_t(atoi(argv[12]));
    if (g.n != 4u && g.n != 2u) {
        free(jpeg);
        return 2;
    }

    ImageData *img = nullptr;
    Status s = ImageData::parse(jpeg, file.size(), false, &img, flags);
    if (!s.ok()) {
        printf("error: %s\n", s.message.c_str());
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
    std::vector<uint32_t> words(scan.words(), scan.words() + scan.nwords());
    std::vector<uint32_t> starts(scan.starts(), scan.starts() + scan.nstarts());
    std::vector<uint16_t> l1(img->l1, img->l1 + 1024), l2(img->l2);
    // the global LUT blob as the runtime lays it out: L2, padded to a dword, then the direct tables
    if (l2.size() & 1)
        l2.push_back(0);
    l2.insert(l2.end(), img->ac_fast.begin(), img->ac_fast.end());
    l2.insert(l2.end(), img->dc_fast.begin(), img->dc_fast.end());
    // sentinels | shift | the destination, exactly `total` bytes | sentinels
    uint8_t *block = static_cast<uint8_t *>(aligned_alloc(16, (kSentinelBytes + shift + total + kSentinelBytes + 15) & ~size_t(15)));
    memset(block, kSentinel, kSentinelBytes + shift + total + kSentinelBytes);
    memset(block + kSentinelBytes + shift, kPrefill, total);
    g.dst = block + kSentinelBytes + shift;
    d.words = words.data();
    d.starts = starts.data();
    d.nwords = uint32_t(words.size());
    d.nstarts = uint32_t(starts.size());
    d.l1 = l1.data();
    d.l2 = l2.data();
    d.out = nullptr; // (a scaled decode has no texture)

    const uint32_t hs = d.hsample[0], vs = img->components == 1 ? 0u : d.vsample[0];
    const LutBudget luts(argc, argv, 13);
    luts.apply(d);
    const uint32_t l2_in_lds = luts.in_lds(*img);
    luts.report(d, l2_in_lds);
    const uint32_t threads = waves_per_block * kWave;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    const uint32_t lds_bytes = align16((kL1Entries + l2_in_lds) * 2u) + waves_per_block * wave_area;
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
            if (!(g.n == 4u ? run_wave_of<4>(hs, vs, d, sh, g, wave_first) : run_wave_of<2>(hs, vs, d, sh, g, wave_first)))
                return 3;
        }
        free(smem);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    fwrite(block, 1, kSentinelBytes + shift + total + kSentinelBytes, o);
    fclose(o);
    printf("ok %u %u %u %u\n", img->width, img->height, d.total_intervals, d.restart_interval);
    free(block);
    delete img;
    free(jpeg);
    return 0;
}
