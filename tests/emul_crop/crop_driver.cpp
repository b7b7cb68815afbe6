// Host-side run of the cropped kernels' lane body and touch test (compeg_amd/csrc/crop_body.h) for sanitizer runs (TEST ONLY).
//
// A stand-alone program: g++ -fsanitize=address,undefined compiles the body the GPU lanes execute together with the host
// front end, and main() drives decode_cropped_*_kernel the way tests/emul_reduced/reduced_driver.cpp drives the reduced
// kernels: workgroup by workgroup over a heap block filled with 0xA5 standing in for LDS and exact-size heap copies of
// the words, the start positions and the LUTs.  The prologue's three tests are made where the kernel makes them: a
// workgroup none of whose intervals touch the box is not set up at all, a wave none of whose 64 do has no window staged
// (its LDS stays 0xA5), a lane that does not touch runs nothing.  The store stage is lane-local, so a wave is its 64 lanes
// one after the other, each through decode_wave_cropped itself.  The destination lies between two runs of sentinel
// bytes inside one block, pre-filled with 0xA5; the whole block is written out for the test to look at.
//
//   crop_driver decode in.jpg out.bin flags waves_per_block window_words format shift x y width height pitch total [luts [control]]
//   crop_driver touch cases.txt
//
// flags: COMPEG_PARSE_*; format: COMPEG_CROP_*; shift: bytes the destination begins behind a 16-byte boundary; pitch,
// total: compeg_crop_shape's answer for the one image.
// touch: every line of cases.txt is "wm total_mcus dri mx0 mx1 my0 my1 interval reach" -- reach as tests/crop_stream.py
// found it by going through the interval's MCUs one by one -- and crop_reach must give that; then every rectangle of a
// 5 x 4-MCU image at DRI 1 .. 21 and without DRI against the same search made here; and two mutants of crop_reach, which
// must each disagree with the search somewhere.
// luts, control: how many LUT entries are staged behind L1 and the control that ignores it (tests/emul/lut_budget.h);
// default: what the planner stages, the direct AC tables counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../compeg_amd/csrc/crop_body.h"
#include "../../compeg_amd/csrc/device_types.h"
#include "../../compeg_amd/csrc/front.h"
#include "../../compeg_amd/csrc/scan.h"
#include "../emul/lut_budget.h"

namespace compeg {
void fill_desc(const ImageData &img, ImageDesc &d);
}
using namespace compeg;

constexpr size_t kSentinelBytes = 256;
constexpr uint8_t kSentinel = 0x5c, kPrefill = 0xa5;

struct Skipped {
    uint32_t workgroups = 0, waves = 0, lanes = 0, walked = 0, mcus = 0, stored = 0;
};

// A wave: its 64 lanes one after the other through decode_wave_cropped itself (the store stage is lane-local).  What is
// counted beside it -- the lanes that do not touch, the MCUs walked, the MCUs in the box -- comes from the touch test and
// a search through each interval's MCUs, not from the wave function: that its walk and its stores are those is what the
// comparison of every destination byte says.
template <int HS, int VS>
static void run_wave(const ImageDesc &d, const HuffShared &sh, const CropTarget &g, uint32_t wave_first, Skipped &n)
{
    for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
        const uint32_t iv = wave_first + lane;
        decode_wave_cropped<HS, VS>(d, sh, g, g.dst, iv, lane);
        if (iv >= d.total_intervals)
            continue;
        const uint32_t reach = crop_intervals_reach(d, g, iv, 1u);
        n.lanes += reach == 0u ? 1u : 0u;
        n.walked += reach != 0u ? 1u : 0u;
        n.mcus += reach;
        for (uint32_t m = iv * d.restart_interval; m < iv * d.restart_interval + reach; m++) {
            const uint32_t mx = m % d.width_mcus, my = m / d.width_mcus;
            n.stored += mx >= g.mx0 && mx < g.mx1 && my >= g.my0 && my < g.my1 ? 1u : 0u;
        }
    }
}

static int decode(int argc, char **argv)
{
    if (argc < 15 || argc > 15 + 2) {
        fprintf(stderr, "usage: %s decode in.jpg out.bin flags waves window_words format shift x y width height pitch total [luts [control]]\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[2], "rb");
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
    const unsigned flags = unsigned(atoi(argv[4]));
    const uint32_t waves_per_block = uint32_t(atoi(argv[5]));
    const uint32_t window_words = (uint32_t(atoi(argv[6])) + 3u) & ~3u;
    CropTarget g{};
    g.format = uint32_t(atoi(argv[7]));
    const size_t shift = size_t(atoi(argv[8]));
    g.x = uint32_t(atoi(argv[9]));
    g.y = uint32_t(atoi(argv[10]));
    g.width = uint32_t(atoi(argv[11]));
    g.height = uint32_t(atoi(argv[12]));
    g.pitch = uint32_t(atoi(argv[13]));
    const size_t total = size_t(atoll(argv[14]));
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
    // the rectangle in MCUs, as the library's host side computes it once (capi.cpp: crop_target)
    g.mx0 = g.x / d.mcu_w;
    g.mx1 = (g.x + g.width - 1u) / d.mcu_w + 1u;
    g.my0 = g.y / d.mcu_h;
    g.my1 = (g.y + g.height - 1u) / d.mcu_h + 1u;
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
    d.out = nullptr; // (a cropped decode has no texture)

    const uint32_t hs = d.hsample[0], vs = img->components == 1 ? 0u : d.vsample[0];
    const LutBudget luts(argc, argv, 15);
    luts.apply(d);
    const uint32_t l2_in_lds = luts.in_lds(*img);
    luts.report(d, l2_in_lds);
    const uint32_t threads = waves_per_block * kWave;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    const uint32_t lds_bytes = align16((kL1Entries + l2_in_lds) * 2u) + waves_per_block * wave_area;
    Skipped skipped;
    for (uint32_t first = 0; first < d.total_intervals; first += threads) {
        if (crop_intervals_reach(d, g, first, threads) == 0u) {
            skipped.workgroups++; // (before it stages anything)
            continue;
        }
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
            if (crop_intervals_reach(d, g, wave_first, kWave) == 0u) {
                skipped.waves++; // (no window loads)
                continue;
            }
            uint32_t wb = 0, wl = 0;
            wave_window(d, wave_first, window_words, wb, wl);
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
                stage_window(d, win, wb, wl, lane);
            HuffShared sh{sl1, sl2, luts.l2_staged(d, l2_in_lds), win, wb, wl, slots};
            if (hs == 2 && vs == 1)
                run_wave<2, 1>(d, sh, g, wave_first, skipped);
            else if (hs == 1 && vs == 1)
                run_wave<1, 1>(d, sh, g, wave_first, skipped);
            else if (hs == 1 && vs == 2)
                run_wave<1, 2>(d, sh, g, wave_first, skipped);
            else if (hs == 2 && vs == 2)
                run_wave<2, 2>(d, sh, g, wave_first, skipped);
            else if (hs == 1 && vs == 0)
                run_wave<1, 0>(d, sh, g, wave_first, skipped);
            else
                return 3;
        }
        free(smem);
    }
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(block, 1, kSentinelBytes + shift + total + kSentinelBytes, o);
    fclose(o);
    printf("ok %u %u %u %u\n", img->width, img->height, d.total_intervals, d.restart_interval);
    printf("skipped %u workgroups %u waves %u lanes; walked %u lanes %u mcus, stored %u\n", skipped.workgroups, skipped.waves, skipped.lanes,
           skipped.walked, skipped.mcus, skipped.stored);
    free(block);
    delete img;
    free(jpeg);
    return 0;
}

// ---- the touch test --------------------------------------------------------------------------------------------------

struct Box {
    uint32_t mx0, mx1, my0, my1;
};

// MCUs a .. b - 1 one by one: the count from a up to and with the last one in the box, 0 if there is none.
static uint32_t search_reach(uint32_t a, uint32_t b, uint32_t wm, const Box &x)
{
    uint32_t reach = 0;
    for (uint32_t m = a; m < b; m++) {
        const uint32_t mx = m % wm, my = m / wm;
        if (mx >= x.mx0 && mx < x.mx1 && my >= x.my0 && my < x.my1)
            reach = m - a + 1u;
    }
    return reach;
}

// Mutant 1: off by one where a run wraps over the end of an MCU row -- the first MCU of the row below is taken for column 1.
static uint32_t mutant_wrap(uint32_t a, uint32_t b, uint32_t wm, const Box &x)
{
    const uint32_t lo = umax(a, x.my0 * wm), hi = umin(b, x.my1 * wm);
    if (lo >= hi)
        return 0u;
    const uint32_t c = lo % wm;
    const uint32_t first = c < x.mx0 ? lo + (x.mx0 - c) : (c < x.mx1 ? lo : lo + (wm - c) + x.mx0 + 1u);
    if (first >= hi)
        return 0u;
    const uint32_t m = hi - 1u, e = m % wm;
    const uint32_t last = e >= x.mx1 ? m - (e - (x.mx1 - 1u)) : (e >= x.mx0 ? m : m - e - (wm - x.mx1) - 1u);
    return last + 1u - a;
}

// Mutant 2: the last MCU of a run is not looked at.
static uint32_t mutant_last(uint32_t a, uint32_t b, uint32_t wm, const Box &x)
{
    return b > a ? crop_reach(a, b - 1u, wm, x.mx0, x.mx1, x.my0, x.my1) : 0u;
}

struct Tally {
    unsigned long cases = 0, wrong = 0, touch_wrong = 0, wrap = 0, last = 0;
    void one(uint32_t a, uint32_t b, uint32_t wm, const Box &x, uint32_t want)
    {
        cases++;
        const uint32_t got = crop_reach(a, b, wm, x.mx0, x.mx1, x.my0, x.my1);
        if (got != want) {
            if (wrong++ < 5)
                printf("wrong: MCUs %u..%u of rows of %u, box [%u, %u) x [%u, %u): reach %u, the search says %u\n", a, b, wm, x.mx0, x.mx1, x.my0,
                       x.my1, got, want);
            touch_wrong += (got != 0u) != (want != 0u);
        }
        wrap += (mutant_wrap(a, b, wm, x) != 0u) != (want != 0u); // (the mutants are judged on "touches or not" alone)
        last += (mutant_last(a, b, wm, x) != 0u) != (want != 0u);
    }
};

static int touch(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f)
        return 2;
    Tally listed, all;
    unsigned wm, total, dri, mx0, mx1, my0, my1, k, want;
    while (fscanf(f, "%u %u %u %u %u %u %u %u %u", &wm, &total, &dri, &mx0, &mx1, &my0, &my1, &k, &want) == 9) {
        const uint32_t a = k * dri;
        const uint64_t end = uint64_t(k + 1u) * dri;
        const Box x{mx0, mx1, my0, my1};
        const uint32_t b = end < total ? uint32_t(end) : total;
        if (search_reach(a, b, wm, x) != want) {
            printf("the two searches disagree on a case\n");
            return 1;
        }
        listed.one(a, b, wm, x, want);
    }
    fclose(f);
    // every rectangle of a 5 x 4-MCU image at DRI 1 .. 21 and without DRI (one interval of 20)
    const uint32_t w5 = 5, h4 = 4, mcus = w5 * h4;
    for (uint32_t dri = 0; dri <= 21; dri++) {
        const uint32_t per = dri ? dri : mcus;
        for (uint32_t x0 = 0; x0 < w5; x0++)
            for (uint32_t x1 = x0 + 1; x1 <= w5; x1++)
                for (uint32_t y0 = 0; y0 < h4; y0++)
                    for (uint32_t y1 = y0 + 1; y1 <= h4; y1++)
                        for (uint32_t k = 0; k * per < mcus; k++) {
                            const Box x{x0, x1, y0, y1};
                            const uint32_t a = k * per, b = umin(a + per, mcus);
                            all.one(a, b, w5, x, search_reach(a, b, w5, x));
                        }
    }
    printf("touch listed %lu wrong %lu touch_wrong %lu mutant_wrap %lu mutant_last %lu\n", listed.cases, listed.wrong, listed.touch_wrong, listed.wrap,
           listed.last);
    printf("touch exhaustive %lu wrong %lu touch_wrong %lu mutant_wrap %lu mutant_last %lu\n", all.cases, all.wrong, all.touch_wrong, all.wrap, all.last);
    return listed.wrong || all.wrong ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && strcmp(argv[1], "decode") == 0)
        return decode(argc, argv);
    if (argc == 3 && strcmp(argv[1], "touch") == 0)
        return touch(argv[2]);
    fprintf(stderr, "usage: %s decode ... | touch cases.txt\n", argv[0]);
    return 2;
}
