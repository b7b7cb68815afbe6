// Stand-alone driver of the scan kernels (compeg_amd/csrc/scan_kernels.hip) for tests/test_gpu_scan_edges.py.
//
//     scan_harness CASES OUTDIR
//
// Linked with the library's own scan_kernels.o: the kernels under test are the shipped ones.  Of the runtime it
// calls launch_scan, launch_pull, launch_pull3 and scan_tiles (scan_kernels.h), nothing else.
//
// Every output lies in one device allocation (the arena) at exactly the size scan_kernels.h documents, at the
// alignment the runtime gives it (256 bytes; results at a 32-byte stride), with kGuard bytes in front of and behind
// it, so that an overrun lands in a guard and is read back.  Before a launch the whole arena is filled with kPrefill
// (never zeros; result[3] alone is cleared, which is the caller's part of the contract) -- or, for a group that
// says `keep`, left as the previous group's launch left it, the way a batch's second upload finds its arenas.
// After the launch the whole arena goes to OUTDIR/gNNNN.bin behind a table of where everything lies.
//
// File formats (little-endian u32 unless said otherwise): tests/scan_edges.py writes and reads them.
//   CASES:  magic, ngroups, then per group: kind (0 scan, 1 pull, 2 pull3) and
//     scan:  nimages, skip, with_span, keep; per image: len, expected, slots, mis, fill, patch, the segment padded
//            to a multiple of 4 bytes.  The first `skip` images only fill descs[0 .. skip): the launch gets
//            descs + skip, and their outputs must keep the prefill.
//     pull:  nseg (1: launch_pull, 3: launch_pull3); per segment: bytes, the source padded to a multiple of 16
//            (the padding is what the pinned source holds up to the next multiple of 16).
//   gNNNN.bin: magic, kind, arena bytes, rows, then per row 10 words -- offset and size of tile_state, starts,
//            words, result, patch targets (pull: offset and size of dst, 8 zeros) -- then the arena.
// Every HIP call is checked; the first error ends the process with a non-zero status and nothing more is launched.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "scan_kernels.h"

namespace {

constexpr uint32_t kMagic = 0x484e4353u; // "SCNH"
constexpr size_t kGuard = 256;
constexpr uint8_t kPrefill = 0xa5;

#define HIP_OK(call)                                                                                                   \
    do {                                                                                                               \
        const hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "scan_harness: %s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));        \
            exit(3);                                                                                                   \
        }                                                                                                              \
    } while (0)

[[noreturn]] void die(const char *what)
{
    fprintf(stderr, "scan_harness: %s\n", what);
    exit(2);
}

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    uint32_t u32()
    {
        if (at + 4 > buf.size())
            die("case file ends early");
        uint32_t v;
        memcpy(&v, buf.data() + at, 4);
        at += 4;
        return v;
    }
    const uint8_t *bytes(size_t n)
    {
        if (at + n > buf.size())
            die("case file ends early");
        const uint8_t *p = buf.data() + at;
        at += n;
        return p;
    }
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One device allocation that grows when a group needs more and otherwise stays where it is.
struct DeviceBuf {
    uint8_t *ptr = nullptr;
    size_t cap = 0;
    void reserve(size_t bytes)
    {
        if (bytes <= cap)
            return;
        if (ptr)
            HIP_OK(hipFree(ptr));
        ptr = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void **>(&ptr), bytes));
        cap = bytes;
    }
};

struct Image {
    uint32_t len, expected, slots, mis, fill, patch;
    const uint8_t *seg;
    size_t o_in;                                     // in the input allocation: start of the image's region
    size_t o_tile, o_starts, o_words, o_result, o_patch; // in the arena
    size_t n_tile, n_starts, n_words;
};

struct Arena {
    size_t total = kGuard;
    // `bytes` at `align` (+ `skew`), kGuard untouched bytes in front of it and behind it
    size_t take(size_t bytes, size_t skew = 0)
    {
        const size_t at = align_up(total, 256) + skew;
        total = at + bytes + kGuard;
        return at;
    }
};

void write_result(const std::string &dir, uint32_t group, uint32_t kind, const std::vector<uint32_t> &table,
                  const std::vector<uint8_t> &arena)
{
    char name[32];
    snprintf(name, sizeof name, "/g%04u.bin", group);
    const std::string tmp = dir + name + ".part", path = dir + name;
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f)
        die("cannot write the result file");
    const uint32_t head[4] = {kMagic, kind, uint32_t(arena.size()), uint32_t(table.size() / 10)};
    bool ok = fwrite(head, 4, 4, f) == 4 && fwrite(table.data(), 4, table.size(), f) == table.size() &&
              fwrite(arena.data(), 1, arena.size(), f) == arena.size();
    ok = fclose(f) == 0 && ok;
    if (!ok || rename(tmp.c_str(), path.c_str()) != 0)
        die("cannot write the result file");
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 3)
        die("usage: scan_harness CASES OUTDIR");
    Reader in;
    {
        FILE *f = fopen(argv[1], "rb");
        if (!f)
            die("cannot read the case file");
        fseek(f, 0, SEEK_END);
        const long n = ftell(f);
        fseek(f, 0, SEEK_SET);
        in.buf.resize(size_t(n));
        if (fread(in.buf.data(), 1, size_t(n), f) != size_t(n))
            die("cannot read the case file");
        fclose(f);
    }
    const std::string outdir = argv[2];
    if (in.u32() != kMagic)
        die("not a case file");
    const uint32_t ngroups = in.u32();

    HIP_OK(hipSetDevice(0));
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));
    DeviceBuf arena, inputs, descs;
    size_t last_total = 0;
    std::vector<uint8_t> host;

    for (uint32_t g = 0; g < ngroups; g++) {
        const uint32_t kind = in.u32();
        std::vector<uint32_t> table;
        if (kind == 0) {
            const uint32_t n = in.u32(), skip = in.u32(), with_span = in.u32(), keep = in.u32();
            if (skip >= n)
                die("a scan group launches no image");
            std::vector<Image> im(n);
            Arena lay;
            size_t in_total = 0;
            uint32_t max_tiles = 0;
            for (uint32_t i = 0; i < n; i++) {
                Image &m = im[i];
                m.len = in.u32(), m.expected = in.u32(), m.slots = in.u32(), m.mis = in.u32(), m.fill = in.u32();
                m.patch = in.u32();
                m.seg = in.bytes(align_up(m.len, 4));
                if (m.slots == 0 || (m.slots & (m.slots - 1)) || m.mis >= 16)
                    die("bad image header");
                // [16 readable bytes][mis][segment][16 readable bytes], the region's start 256-aligned
                m.o_in = in_total;
                in_total += align_up(16 + m.mis + size_t(m.len) + 16, 256);
                m.n_tile = size_t(compeg::scan_tiles(m.len)) * compeg::kScanTileStateBytes;
                m.n_starts = size_t(m.slots) * 4;
                m.n_words = size_t(m.len) + m.len / 3 + 4;
                m.o_tile = lay.take(m.n_tile);
                m.o_starts = lay.take(m.n_starts);
                m.o_words = lay.take(m.n_words);
                m.o_result = lay.take(compeg::kScanResultBytes, 32 * (i % 8));
                m.o_patch = m.patch ? lay.take(8) : 0;
                if (i >= skip)
                    max_tiles = std::max(max_tiles, compeg::scan_tiles(m.len));
                const size_t row[10] = {m.o_tile,   m.n_tile,   m.o_starts,
                                        m.n_starts, m.o_words,  m.n_words,
                                        m.o_result, compeg::kScanResultBytes, m.o_patch, m.patch ? size_t(8) : size_t(0)};
                for (size_t v : row)
                    table.push_back(uint32_t(v));
            }
            if (lay.total > 0xffffffffu)
                die("arena too large");
            if (keep && (lay.total != last_total || arena.cap < lay.total))
                die("keep: the layout differs from the previous group's");
            arena.reserve(lay.total);
            inputs.reserve(in_total + 256);
            descs.reserve(n * sizeof(compeg::ScanDesc));
            last_total = lay.total;
            // outputs and guards: the prefill, or what the last launch left
            const uint32_t zero = 0;
            if (!keep) {
                host.assign(lay.total, kPrefill);
                for (const Image &m : im)
                    memcpy(host.data() + m.o_result + 12, &zero, 4); // (flags are OR-ed in: the caller clears them)
                HIP_OK(hipMemcpy(arena.ptr, host.data(), lay.total, hipMemcpyHostToDevice));
            } else {
                for (const Image &m : im)
                    HIP_OK(hipMemcpy(arena.ptr + m.o_result + 12, &zero, 4, hipMemcpyHostToDevice));
            }
            // inputs
            std::vector<uint8_t> hin(in_total + 256);
            std::vector<compeg::ScanDesc> sd(n);
            for (uint32_t i = 0; i < n; i++) {
                const Image &m = im[i];
                const size_t region = align_up(16 + m.mis + size_t(m.len) + 16, 256);
                memset(hin.data() + m.o_in, int(m.fill), region);
                memcpy(hin.data() + m.o_in + 16 + m.mis, m.seg, m.len);
                compeg::ScanDesc &d = sd[i];
                d.raw = inputs.ptr + m.o_in + 16 + m.mis;
                d.len = m.len;
                d.ntiles = compeg::scan_tiles(m.len);
                d.slots = m.slots;
                d.tile_state = reinterpret_cast<uint32_t *>(arena.ptr + m.o_tile);
                d.starts_out = reinterpret_cast<uint32_t *>(arena.ptr + m.o_starts);
                d.words_out = arena.ptr + m.o_words;
                d.expected = m.expected;
                d.result = reinterpret_cast<uint32_t *>(arena.ptr + m.o_result);
                d.patch_nwords = m.patch ? reinterpret_cast<uint32_t *>(arena.ptr + m.o_patch) : nullptr;
                d.patch_nstarts = m.patch ? reinterpret_cast<uint32_t *>(arena.ptr + m.o_patch + 4) : nullptr;
            }
            HIP_OK(hipMemcpy(inputs.ptr, hin.data(), hin.size(), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(descs.ptr, sd.data(), n * sizeof(compeg::ScanDesc), hipMemcpyHostToDevice));
            HIP_OK(compeg::launch_scan(reinterpret_cast<const compeg::ScanDesc *>(descs.ptr) + skip, n - skip, max_tiles,
                                       stream, with_span != 0));
            HIP_OK(hipStreamSynchronize(stream));
            host.resize(lay.total);
            HIP_OK(hipMemcpy(host.data(), arena.ptr, lay.total, hipMemcpyDeviceToHost));
        } else if (kind == 1 || kind == 2) {
            const uint32_t nseg = in.u32();
            if (nseg != (kind == 1 ? 1u : 3u))
                die("bad pull group");
            size_t bytes[3] = {0, 0, 0}, o_dst[3] = {0, 0, 0}, o_src[3] = {0, 0, 0};
            const uint8_t *data[3] = {nullptr, nullptr, nullptr};
            Arena lay;
            size_t src_total = 0;
            for (uint32_t k = 0; k < nseg; k++) {
                bytes[k] = in.u32();
                data[k] = in.bytes(align_up(bytes[k], 16));
                o_dst[k] = lay.take(align_up(bytes[k], 16));
                o_src[k] = src_total;
                src_total += align_up(bytes[k], 16) + 256;
                table.push_back(uint32_t(o_dst[k]));
                table.push_back(uint32_t(align_up(bytes[k], 16)));
                for (int z = 0; z < 8; z++)
                    table.push_back(0u);
            }
            arena.reserve(lay.total);
            last_total = 0;
            host.assign(lay.total, kPrefill);
            HIP_OK(hipMemcpy(arena.ptr, host.data(), lay.total, hipMemcpyHostToDevice));
            uint8_t *pinned = nullptr;
            HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&pinned), src_total, hipHostMallocDefault));
            for (uint32_t k = 0; k < nseg; k++)
                memcpy(pinned + o_src[k], data[k], align_up(bytes[k], 16));
            if (kind == 1) {
                HIP_OK(compeg::launch_pull(arena.ptr + o_dst[0], pinned + o_src[0], bytes[0], stream));
            } else {
                void *const dst[3] = {arena.ptr + o_dst[0], arena.ptr + o_dst[1], arena.ptr + o_dst[2]};
                const void *const src[3] = {pinned + o_src[0], pinned + o_src[1], pinned + o_src[2]};
                HIP_OK(compeg::launch_pull3(dst, src, bytes, stream));
            }
            HIP_OK(hipStreamSynchronize(stream));
            HIP_OK(hipMemcpy(host.data(), arena.ptr, lay.total, hipMemcpyDeviceToHost));
            HIP_OK(hipHostFree(pinned));
        } else {
            die("unknown group kind");
        }
        write_result(outdir, g, kind, table, host);
    }
    HIP_OK(hipStreamDestroy(stream));
    printf("scan_harness: %u groups\n", ngroups);
    return 0;
}
