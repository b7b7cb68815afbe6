// CPU driver of the resize_tensor_antialias kernels' lane body (compeg_amd/csrc/antialias_body.h), built by
// tests/test_antialias_emulation.py with g++ -fsanitize=address,undefined: plans every launch with the library's own
// planner (records and axis tables) and runs its grid lane by lane.
//
//   antialias_driver IN OUT
//
// IN (little endian): u32 cases, then per case
//   u32 images, downscale, dtype, order, filter, out_width, out_height; f32 scale[3], bias[3];
//   u32 dst_offset, dst_bytes (the buffer the destination lies in, and where in it);
//   per image u32 width, height, src_pitch, src_rows (its allocation: src_pitch * src_rows bytes), crop x, y, width, height;
//   the images' allocations, one behind the other; the destination buffer's bytes as they are before the pack.
// OUT: per case the destination buffer's bytes after the pack, then u32 the number of axis tables the launch built.
// Every source image, the tables and the destination buffer are heap blocks of exactly their size: a load beyond an
// image's allocation or a table, or a store beyond the buffer, is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "antialias_body.h"

using namespace compeg;

template <uint32_t DTYPE, uint32_t K>
static void run_grid(const AntialiasPack &t, uint32_t blocks)
{
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t lane = 0; lane < kTensorThreads; lane++)
            antialias_tensor_block_lane<DTYPE, K>(t, b, lane);
}

template <uint32_t DTYPE>
static void run_dtype(const AntialiasPack &t, uint32_t blocks, uint32_t k)
{
    switch (k) {
    case 1: run_grid<DTYPE, 1>(t, blocks); break;
    case 2: run_grid<DTYPE, 2>(t, blocks); break;
    case 4: run_grid<DTYPE, 4>(t, blocks); break;
    default: run_grid<DTYPE, 8>(t, blocks); break;
    }
}

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: antialias_driver IN OUT\n");
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
    for (uint32_t n = 0; n < cases; n++) {
        uint32_t head[7], where[2];
        compeg_tensor_spec spec{};
        if (!read_exact(in, head, sizeof head) || !read_exact(in, spec.scale, 12) || !read_exact(in, spec.bias, 12) ||
            !read_exact(in, where, sizeof where))
            return 2;
        const uint32_t images = head[0];
        spec.downscale = head[1];
        spec.dtype = head[2];
        spec.order = head[3];
        const compeg_resize_spec resize{head[5], head[6], head[4], 0};
        const size_t dst_bytes = where[1];
        std::vector<uint32_t> geom(size_t(images) * 8u);
        if (!read_exact(in, geom.data(), geom.size() * 4u))
            return 2;
        std::vector<uint8_t *> srcs(images);
        std::vector<AntialiasImage> records(images);
        AntialiasTables tables;
        for (uint32_t i = 0; i < images; i++) {
            const uint32_t *g = &geom[size_t(i) * 8u];
            const size_t bytes = size_t(g[2]) * g[3];
            // (aligned like device allocations are; exactly as long as they are)
            srcs[i] = static_cast<uint8_t *>(aligned_alloc(256, (bytes + 255) / 256 * 256));
            if (bytes % 256 || !srcs[i] || !read_exact(in, srcs[i], bytes)) {
                fprintf(stderr, "case %u: bad input\n", n);
                return 2;
            }
            const compeg_rect crop{g[4], g[5], g[6], g[7]};
            if (uint64_t(crop.x) + crop.width > g[0] || uint64_t(crop.y) + crop.height > g[1] ||
                !plan_antialias_image(records[i], tables, srcs[i], g[2], crop, spec.downscale, resize.out_width, resize.out_height)) {
                fprintf(stderr, "case %u: image %u: no record\n", n, i);
                return 3;
            }
        }
        uint8_t *buf = static_cast<uint8_t *>(aligned_alloc(256, (dst_bytes + 255) / 256 * 256));
        if (dst_bytes % 256 || !buf || !read_exact(in, buf, dst_bytes)) {
            fprintf(stderr, "case %u: bad input\n", n);
            return 2;
        }
        AntialiasPack t;
        uint32_t blocks = 0;
        if (!plan_antialias_pack(t, blocks, images, spec, resize, buf + where[0])) {
            fprintf(stderr, "case %u: no plan\n", n);
            return 3;
        }
        // (a block of exactly the tables' size: the vector's capacity may be larger)
        uint32_t *words = static_cast<uint32_t *>(malloc(tables.words.size() * 4u));
        if (!words)
            return 2;
        memcpy(words, tables.words.data(), tables.words.size() * 4u);
        t.images = records.data();
        t.tables = words;
        switch (spec.dtype) {
        case COMPEG_TENSOR_U8: run_dtype<COMPEG_TENSOR_U8>(t, blocks, spec.downscale); break;
        case COMPEG_TENSOR_F16: run_dtype<COMPEG_TENSOR_F16>(t, blocks, spec.downscale); break;
        case COMPEG_TENSOR_BF16: run_dtype<COMPEG_TENSOR_BF16>(t, blocks, spec.downscale); break;
        default: run_dtype<COMPEG_TENSOR_F32>(t, blocks, spec.downscale); break;
        }
        const uint32_t axes = uint32_t(tables.axes.size());
        if (fwrite(buf, 1, dst_bytes, out) != dst_bytes || fwrite(&axes, 4, 1, out) != 1)
            return 2;
        for (uint8_t *s : srcs)
            free(s);
        free(words);
        free(buf);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
