// Host-side run of the region-list cropped kernels (compeg_amd/csrc/crop_regions_body.h over crop_body.h) for sanitizer
// runs (TEST ONLY).
//
// A stand-alone program: g++ -fsanitize=address,undefined compiles the body the GPU lanes execute together with the host
// front end and the library's own grouping (crop_regions_types.h: make_crop_regions_call), and main() drives
// decode_cropped_regions_*_kernel the way tests/emul_crop/crop_driver.cpp drives the one-rectangle kernels: per sampling
// group, per record (a row of the grid), workgroup by workgroup over a heap block filled with 0xA5 standing in for LDS
// and exact-size heap copies of every image's words, start positions and LUTs and of the record array.  The prologue's
// tests are made where the kernel makes them.  The destination lies between two runs of sentinel bytes inside one
// block, pre-filled with 0xA5; the whole block is written out for the test to look at.
//
//   crop_regions_driver manifest.txt out.bin [luts [control]]
//
// manifest.txt: "format pitch slot_w slot_h slot_bytes shift window_words waves mutant images regions", then per image
// "path flags", then per region "image x y width height dst_x dst_y".  pitch, slot_bytes: compeg_crop_regions_shape's.
// shift: bytes the destination begins behind a 16-byte boundary.  mutant 1: every region decodes the first record's
// rectangle; mutant 2: a region's slot is its rank inside its sampling group, not its index -- the test must catch both.
// luts, control: how many LUT entries are staged behind L1 and the control that ignores it (tests/emul/lut_budget.h);
// default: what the planner stages for the batch -- its largest image's, the direct AC tables counted -- while each image
// stages its own.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../compeg_amd/csrc/crop_regions_body.h"
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

// One image with exact-size copies of what its descriptor points at: reads past an end are the sanitizer's to report.
struct Image {
    std::unique_ptr<ImageData> data;
    std::vector<uint32_t> words, starts;
    std::vector<uint16_t> l1, l2;
    uint32_t l2_in_lds = 0, hs = 0, vs = 0;
    uint8_t *jpeg = nullptr; // (the file, exact size; the parsed image may point into it)
    Image() = default;
    Image(const Image &) = delete;
    ~Image()
    {
        data.reset();
        free(jpeg);
    }
};

static bool load(const char *path, unsigned flags, const LutBudget &luts, Image &out, ImageDesc &d)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return false;
    std::vector<uint8_t> file;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0)
        file.insert(file.end(), buf, buf + n);
    fclose(f);
    uint8_t *jpeg = static_cast<uint8_t *>(malloc(file.size() ? file.size() : 1));
    memcpy(jpeg, file.data(), file.size());
    ImageData *img = nullptr;
    Status s = ImageData::parse(jpeg, file.size(), false, &img, flags);
    out.jpeg = jpeg;
    if (!s.ok()) {
        printf("error: %s: %s\n", path, s.message.c_str());
        return false;
    }
    out.data.reset(img);
    ScanBuffer scan;
    Status pre = scan.process(img->scan_data(), img->scan_len, img->metadata.total_restart_intervals);
    if (!pre.ok() && pre.code != COMPEG_E_COUNT_MISMATCH) {
        printf("error: %s: %s\n", path, pre.message.c_str());
        return false;
    }
    fill_desc(*img, d);
    luts.apply(d);
    out.words.assign(scan.words(), scan.words() + scan.nwords());
    out.starts.assign(scan.starts(), scan.starts() + scan.nstarts());
    out.l1.assign(img->l1, img->l1 + 1024);
    out.l2 = img->l2;
    // the global LUT blob as the runtime lays it out: L2, padded to a dword, then the direct tables
    if (out.l2.size() & 1)
        out.l2.push_back(0);
    out.l2.insert(out.l2.end(), img->ac_fast.begin(), img->ac_fast.end());
    out.l2.insert(out.l2.end(), img->dc_fast.begin(), img->dc_fast.end());
    out.l2_in_lds = luts.in_lds(*img);
    out.hs = d.hsample[0];
    out.vs = img->components == 1 ? 0u : d.vsample[0];
    d.words = out.words.data();
    d.starts = out.starts.data();
    d.nwords = uint32_t(out.words.size());
    d.nstarts = uint32_t(out.starts.size());
    d.l1 = out.l1.data();
    d.l2 = out.l2.data();
    d.out = nullptr; // (a cropped decode has no texture)
    return true;
}

struct Counts {
    uint32_t launches = 0, workgroups_skipped = 0, waves_skipped = 0, lanes_walked = 0;
};

// A row of the grid: the kernel's body for record `y` of the launch, every workgroup of the x extent.
template <int HS, int VS>
static void run_row(const ImageDesc *descs, const CropRegionRecord *records, uint32_t y, const CropRegionsTarget &t, uint32_t max_intervals,
                    uint32_t l2_in_lds, uint32_t window_words, uint32_t waves_per_block, Counts &n, const LutBudget &luts)
{
    const CropRegionRecord &r = records[y];
    const CropTarget g = crop_region_rect(r, t);
    const ImageDesc &d = descs[r.image];
    const uint32_t threads = waves_per_block * kWave;
    const uint32_t wave_area = align16(window_words * 4u) + kWave * kDuSlotBytes;
    const uint32_t lds_bytes = align16((kL1Entries + l2_in_lds) * 2u) + waves_per_block * wave_area;
    for (uint32_t first = 0; first < max_intervals; first += threads) { // (the grid's x extent is the group's largest image's)
        if (first >= d.total_intervals)
            continue;
        if (crop_intervals_reach(d, g, first, threads) == 0u) {
            n.workgroups_skipped++; // (before it stages anything)
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
                n.waves_skipped++; // (no window loads)
                continue;
            }
            uint32_t wb = 0, wl = 0;
            wave_window(d, wave_first, window_words, wb, wl);
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++)
                stage_window(d, win, wb, wl, lane);
            HuffShared sh{sl1, sl2, luts.l2_staged(d, l2_in_lds), win, wb, wl, slots};
            for (uint32_t lane = 0; lane < uint32_t(kWave); lane++) {
                decode_wave_cropped_region<HS, VS>(d, sh, g, t, wave_first + lane, lane);
                n.lanes_walked += wave_first + lane < d.total_intervals && crop_intervals_reach(d, g, wave_first + lane, 1u) != 0u ? 1u : 0u;
            }
        }
        free(smem);
    }
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc > 3 + 2) {
        fprintf(stderr, "usage: %s manifest.txt out.bin [luts [control]]\n", argv[0]);
        return 2;
    }
    const LutBudget luts(argc, argv, 3);
    FILE *m = fopen(argv[1], "r");
    if (!m)
        return 2;
    unsigned format, pitch, slot_w, slot_h, shift, window, waves, mutant, nimages, nregions;
    unsigned long long slot_bytes;
    if (fscanf(m, "%u %u %u %u %llu %u %u %u %u %u %u", &format, &pitch, &slot_w, &slot_h, &slot_bytes, &shift, &window, &waves, &mutant, &nimages,
               &nregions) != 11)
        return 2;
    const uint32_t window_words = (window + 3u) & ~3u;
    std::vector<Image> images(nimages);
    // exact-size heap copy of the descriptors, as the device's array is
    ImageDesc *descs = static_cast<ImageDesc *>(malloc(sizeof(ImageDesc) * (nimages ? nimages : 1)));
    uint32_t max_l2 = 0;
    for (unsigned i = 0; i < nimages; i++) {
        char path[4096];
        unsigned flags;
        if (fscanf(m, "%4095s %u", path, &flags) != 2 || !load(path, flags, luts, images[i], descs[i]))
            return 1;
        max_l2 = std::max(max_l2, images[i].l2_in_lds); // (plan_huffman: the batch's own maximum)
    }
    for (unsigned i = 0; i < nimages; i++)
        luts.report(descs[i], max_l2);
    std::vector<CropRegionPlace> places(nregions);
    for (unsigned k = 0; k < nregions; k++) {
        CropRegionPlace &p = places[k];
        if (fscanf(m, "%u %u %u %u %u %u %u", &p.image, &p.x, &p.y, &p.width, &p.height, &p.dst_x, &p.dst_y) != 7 || p.image >= nimages)
            return 2;
        p.hs = images[p.image].hs;
        p.vs = images[p.image].vs;
        p.intervals = descs[p.image].total_intervals;
    }
    fclose(m);

    // sentinels | shift | the destination, exactly count slots | sentinels
    const size_t total = size_t(slot_bytes) * nregions;
    uint8_t *block = static_cast<uint8_t *>(aligned_alloc(16, (kSentinelBytes + shift + total + kSentinelBytes + 15) & ~size_t(15)));
    memset(block, kSentinel, kSentinelBytes + shift + total + kSentinelBytes);
    memset(block + kSentinelBytes + shift, kPrefill, total);
    const CropRegionsTarget target{block + kSentinelBytes + shift, uint64_t(slot_w) * slot_h, pitch, format};
    const uint32_t pixel = format == kCropRgba ? 4u : 1u;
    CropRegionsCall call = make_crop_regions_call(target, slot_bytes, pixel, places.data(), nregions);
    if (call.records.size() != nregions)
        return 3;
    // (the mutants go through the records in the library's order again: record `at` is region k, the rank-th of its group)
    size_t at = 0, first = 0;
    for (uint32_t g = 0; g < kCropRegionGroups && mutant != 0; g++) {
        uint32_t rank = 0;
        for (unsigned k = 0; k < nregions; k++) {
            if (crop_region_group(places[k].hs, places[k].vs) != g)
                continue;
            CropRegionRecord &r = call.records[at];
            if (at == 0)
                first = k;
            if (mutant == 1) {
                // the first record's rectangle, at the first record's place in this region's own slot (so it stays inside it)
                const CropRegionRecord &f = call.records[0];
                r.x = f.x, r.y = f.y, r.width = f.width, r.height = f.height;
                r.mx0 = f.mx0, r.mx1 = f.mx1, r.my0 = f.my0, r.my1 = f.my1;
                r.offset = uint64_t(k) * slot_bytes + uint64_t(places[first].dst_y) * pitch + uint64_t(places[first].dst_x) * pixel;
            } else {
                r.offset = uint64_t(rank) * slot_bytes + uint64_t(places[k].dst_y) * pitch + uint64_t(places[k].dst_x) * pixel;
            }
            at++, rank++;
        }
    }
    CropRegionRecord *records = static_cast<CropRegionRecord *>(malloc(sizeof(CropRegionRecord) * (nregions ? nregions : 1)));
    memcpy(records, call.records.data(), sizeof(CropRegionRecord) * nregions);

    Counts counts;
    const CropRegionRecord *group_records = records;
    for (uint32_t g = 0; g < kCropRegionGroups; g++) {
        const uint32_t n = call.count[g];
        counts.launches += n ? 1u : 0u;
        for (uint32_t y = 0; y < n; y++) {
            switch (g) {
            case 0: run_row<2, 1>(descs, group_records, y, call.target, call.intervals[g], max_l2, window_words, waves, counts, luts); break;
            case 1: run_row<1, 1>(descs, group_records, y, call.target, call.intervals[g], max_l2, window_words, waves, counts, luts); break;
            case 2: run_row<1, 2>(descs, group_records, y, call.target, call.intervals[g], max_l2, window_words, waves, counts, luts); break;
            case 3: run_row<2, 2>(descs, group_records, y, call.target, call.intervals[g], max_l2, window_words, waves, counts, luts); break;
            default: run_row<1, 0>(descs, group_records, y, call.target, call.intervals[g], max_l2, window_words, waves, counts, luts); break;
            }
        }
        group_records += n;
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    fwrite(block, 1, kSentinelBytes + shift + total + kSentinelBytes, o);
    fclose(o);
    printf("ok %u launches; skipped %u workgroups %u waves; walked %u lanes\n", counts.launches, counts.workgroups_skipped, counts.waves_skipped,
           counts.lanes_walked);
    printf("groups %u %u %u %u %u\n", call.count[0], call.count[1], call.count[2], call.count[3], call.count[4]);
    free(records);
    free(block);
    free(descs);
    return 0;
}
