// CPU driver of the luma_tensor kernels' lane body (compeg_amd/csrc/luma_body.h), built by tests/test_luma_emulation.py
// with g++ -fsanitize=address,undefined: plans every launch with the library's own planners (records, axis tables, grid;
// dst -> dst' with orient_rect) and runs its grid lane by lane, with bands of 8 rows as the library compiles them or of 3
// (the result must not depend on it).
//
//   luma_driver IN OUT
//
// IN (little endian): u32 cases, then per case
//   u32 regions, images, downscale, dtype, order, kernel, out_width, out_height, band, weights[3]; f32 scale[3], bias[3],
//   pad (one value); u32 dst_offset, dst_bytes (the buffer the destination lies in, and where in it);
//   per image u32 width, height, src_pitch, src_rows (its allocation: src_pitch * src_rows bytes);
//   per region u32 image, src x, y, width, height, dst x, y, width, height (whole rectangles; dst in the upright slot),
//   orientation (1..8);
//   the images' allocations, one behind the other; the destination buffer's bytes as they are before the pack.
// OUT: per case the destination buffer's bytes after the pack.
// Every source image, the records with the tables and the destination buffer are heap blocks of exactly their size: a
// load beyond an image's allocation or a table, or a store beyond the buffer, is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "luma_body.h"

using namespace compeg;

template <uint32_t DTYPE, uint32_t K, uint32_t R>
static void run_grid(const LumaPack &n, uint32_t blocks)
{
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t lane = 0; lane < kTensorThreads; lane++)
            luma_tensor_block_lane<DTYPE, K, R>(n, b, lane);
}

template <uint32_t DTYPE, uint32_t K>
static void run_k(const LumaPack &n, uint32_t blocks, uint32_t band)
{
    if (band == 8u)
        run_grid<DTYPE, K, 8>(n, blocks);
    else
        run_grid<DTYPE, K, 3>(n, blocks);
}

template <uint32_t DTYPE>
static void run_dtype(const LumaPack &n, uint32_t blocks, uint32_t k, uint32_t band)
{
    switch (k) {
    case 1: run_k<DTYPE, 1>(n, blocks, band); break;
    case 2: run_k<DTYPE, 2>(n, blocks, band); break;
    case 4: run_k<DTYPE, 4>(n, blocks, band); break;
    default: run_k<DTYPE, 8>(n, blocks, band); break;
    }
}

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: luma_driver IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        perror("open");
        return 2;
    }
    uint32_t cases = 0;
    if (!read_exact(in, &cases, 4))
        return 2;
    for (uint32_t c = 0; c < cases; c++) {
        uint32_t head[12], where[2];
        float *pad = static_cast<float *>(malloc(4)); // (one value, a block of its own: a read of a second one shows)
        compeg_tensor_spec spec{};
        if (!pad || !read_exact(in, head, sizeof head) || !read_exact(in, spec.scale, 12) || !read_exact(in, spec.bias, 12) ||
            !read_exact(in, pad, 4) || !read_exact(in, where, sizeof where))
            return 2;
        const uint32_t regions = head[0], images = head[1];
        spec.downscale = head[2];
        spec.dtype = head[3];
        spec.order = head[4];
        const compeg_filter_spec filter{head[6], head[7], head[5], 0};
        const uint32_t band = head[8];
        const compeg_luma_spec luma{{head[9], head[10], head[11]}, 0u};
        if (band != 8u && band != 3u) {
            fprintf(stderr, "case %u: no such band\n", c);
            return 3;
        }
        const size_t dst_bytes = where[1];
        std::vector<uint32_t> geom(size_t(images) * 4u), list(size_t(regions) * 10u);
        if (!read_exact(in, geom.data(), geom.size() * 4u) || !read_exact(in, list.data(), list.size() * 4u))
            return 2;
        std::vector<uint8_t *> srcs(images);
        for (uint32_t i = 0; i < images; i++) {
            const uint32_t *g = &geom[size_t(i) * 4u];
            const size_t bytes = size_t(g[2]) * g[3];
            // (aligned like device allocations are; exactly as long as they are)
            srcs[i] = static_cast<uint8_t *>(aligned_alloc(256, (bytes + 255) / 256 * 256));
            if (bytes % 256 || !srcs[i] || !read_exact(in, srcs[i], bytes)) {
                fprintf(stderr, "case %u: bad input\n", c);
                return 2;
            }
        }
        std::vector<OrientSource> sources(regions);
        bool upright = false, transposed = false;
        for (uint32_t r = 0; r < regions; r++) {
            const uint32_t *l = &list[size_t(r) * 10u];
            if (l[0] >= images) {
                fprintf(stderr, "case %u: region %u: no such image\n", c, r);
                return 3;
            }
            const uint32_t *g = &geom[size_t(l[0]) * 4u];
            const compeg_rect src{l[1], l[2], l[3], l[4]}, dst{l[5], l[6], l[7], l[8]};
            compeg_rect turned{};
            if (uint64_t(src.x) + src.width > g[0] || uint64_t(src.y) + src.height > g[1] ||
                !orient_rect(filter.out_width, filter.out_height, l[9], dst, turned)) {
                fprintf(stderr, "case %u: region %u: a rectangle leaves its frame, or no such orientation\n", c, r);
                return 3;
            }
            sources[r] = OrientSource{RegionSource{srcs[l[0]], g[2], src, turned}, l[9]};
            (l[9] < 5u ? upright : transposed) = true;
        }
        std::vector<uint32_t> blob;
        size_t tables_at = 0, axes = 0;
        if (!plan_orient_slots(blob, tables_at, axes, sources.data(), regions, spec.downscale, filter.kernel, filter.out_width, filter.out_height)) {
            fprintf(stderr, "case %u: no records\n", c);
            return 3;
        }
        uint8_t *buf = static_cast<uint8_t *>(aligned_alloc(256, (dst_bytes + 255) / 256 * 256));
        if (dst_bytes % 256 || !buf || !read_exact(in, buf, dst_bytes)) {
            fprintf(stderr, "case %u: bad input\n", c);
            return 2;
        }
        LumaPack n;
        uint32_t blocks = 0;
        if (!plan_luma_pack(n, blocks, regions, spec, filter, luma, pad, buf + where[0], band, upright, transposed)) {
            fprintf(stderr, "case %u: no plan\n", c);
            return 3;
        }
        // (a block of exactly the records' and tables' size: the vector's capacity may be larger)
        uint32_t *words = static_cast<uint32_t *>(malloc(blob.size() * 4u));
        if (!words)
            return 2;
        memcpy(words, blob.data(), blob.size() * 4u);
        n.f.slots = words;
        n.f.tables = words + tables_at / 4u;
        switch (spec.dtype) {
        case COMPEG_TENSOR_U8: run_dtype<COMPEG_TENSOR_U8>(n, blocks, spec.downscale, band); break;
        case COMPEG_TENSOR_F16: run_dtype<COMPEG_TENSOR_F16>(n, blocks, spec.downscale, band); break;
        case COMPEG_TENSOR_BF16: run_dtype<COMPEG_TENSOR_BF16>(n, blocks, spec.downscale, band); break;
        default: run_dtype<COMPEG_TENSOR_F32>(n, blocks, spec.downscale, band); break;
        }
        if (fwrite(buf, 1, dst_bytes, out) != dst_bytes)
            return 2;
        for (uint8_t *s : srcs)
            free(s);
        free(words);
        free(buf);
        free(pad);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
