// Host-side run of the planes kernels' lane body (compeg_amd/csrc/planes_body.h) for sanitizer runs (TEST ONLY).
//
// A stand-alone program: g++ -fsanitize=address,undefined compiles the body the GPU lanes execute together with the host
// front end, and main() drives decode_planes_*_kernel the way tests/emul_gray/gray_driver.cpp drives the grayscale
// kernels: workgroup by workgroup over a heap block filled with 0xA5 standing in for LDS and exact-size heap copies of
// the words, the start positions and the LUTs.  The store stage is lane-local, so a wave is its 64 lanes one after the
// other, each through the steps of decode_wave_planes.  The destination lies between two runs of sentinel bytes inside
// one block, pre-filled; the whole block is written out for the test to look at.
//
//   planes_driver in.jpg out.bin flags waves_per_block window_words format chroma420 shift total planes {offset pitch row_bytes rows}... [luts [control]]
//
// flags: COMPEG_PARSE_*; format: COMPEG_PLANES_*; shift: bytes the destination begins behind a 16-byte boundary;
// total and the planes: compeg_planes_shape's layout of the one image.
// luts, control: how many LUT entries are staged behind L1 and the control that ignores it (tests/emul/lut_budget.h);
// default: what the planner stages, the direct AC tables counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../compeg_amd/csrc/device_types.h"
#include "../../compeg_amd/csrc/front.h"
#include "../../compeg_amd/csrc/planes_body.h"
#include "../../compeg_amd/csrc/scan.h"
#include "../emul/lut_budget.h"

namespace compeg {
void fill_desc(const ImageData &img, ImageDesc &d);
}
using namespace compeg;

constexpr size_t kSentinelBytes = 256;
constexpr uint8_t kSentinel = 0x5c, kPrefill = 0x3c;

template <int HS, int VS>
static void run_wave(const ImageDesc &d, const HuffShared &sh, const PlanesTarget &g, uint32_t wave_first)
{
    constexpr uint32_t kDus = uint32_t(PlanesMcu<HS, VS>::kDus), kLuma = uint32_t(PlanesMcu<HS, VS>::kLuma);
    for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
        uint8_t *slot = sh.du_slots + lane * kDuSlotBytes;
        zero_slot(slot);
        const bool active = wave_first + lane < d.total_intervals;
        const uint32_t iv = active ? wave_first + lane : d.total_intervals - 1u;
        EntropyState e;
        entropy_init(e, d, sh, iv);
        PlanesMcu<HS, VS> t;
        planes_init<HS, VS>(t, d, g, g.dst, iv, active);
        const uint32_t du_total = d.restart_interval * kDus;
        for (uint32_t du = 0, k = 0; du < du_total; du++) {
            const uint32_t comp = k < kLuma ? 0u : k - kLuma + 1u;
            const int32_t dc = entropy_data_unit(e, d, sh, comp, reinterpret_cast<int16_t *>(slot));
            planes_transform<HS, VS>(t, d, comp, k, slot, dc);
            if (k == kDus - 1u) {
                planes_store_mcu<HS, VS>(t, g, g.dst);
                planes_next_mcu<HS, VS>(t, d);
                k = 0;
            } else {
                k++;
            }
        }
    }
}

int main(int argc, char **argv)
{
    if (argc < 11) {
        fprintf(stderr, "usage: %s in.jpg out.bin flags waves window_words format chroma420 shift total planes {offset pitch row_bytes rows}... [luts [control]]\n", argv[0]);
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
    PlanesTarget g{};
    g.format = uint32_t(atoi(argv[6]));
    g.chroma420 = uint32_t(atoi(argv[7]));
    const size_t shift = size_t(atoi(argv[8])), total = size_t(atoll(argv[9]));
    const int planes = atoi(argv[10]);
    if (planes < 1 || planes > 3 || argc < 11 + 4 * planes || argc > 11 + 4 * planes + 2)
        return 2;
    for (int p = 0; p < planes; p++) {
        g.offset[p] = uint64_t(atoll(argv[11 + 4 * p]));
        g.pitch[p] = uint32_t(atoi(argv[12 + 4 * p]));
        g.row_bytes[p] = uint32_t(atoi(argv[13 + 4 * p]));
        g.rows[p] = uint32_t(atoi(argv[14 + 4 * p]));
    }
    g.image_stride = total;

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
    d.out = nullptr; // (a planes decode has no texture)

    const uint32_t hs = d.hsample[0], vs = img->components == 1 ? 0u : d.vsample[0];
    const LutBudget luts(argc, argv, 11 + 4 * planes);
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
            if (hs == 2 && vs == 1)
                run_wave<2, 1>(d, sh, g, wave_first);
            else if (hs == 1 && vs == 1)
                run_wave<1, 1>(d, sh, g, wave_first);
            else if (hs == 1 && vs == 2)
                run_wave<1, 2>(d, sh, g, wave_first);
            else if (hs == 2 && vs == 2)
                run_wave<2, 2>(d, sh, g, wave_first);
            else if (hs == 1 && vs == 0)
                run_wave<1, 0>(d, sh, g, wave_first);
            else
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
