// CPU driver of the pack_tensor kernels' lane body (compeg_amd/csrc/tensor_body.h), built by
// tests/test_tensor_emulation.py with g++ -fsanitize=address,undefined: plans every launch like the library does and
// runs its grid lane by lane.
//
//   pack_driver IN OUT
//
// IN (little endian): u32 cases, then per case
//   u32 width, height, images, downscale, dtype, order; f32 scale[3], bias[3];
//   u32 src_pitch, src_rows (one image's allocation: src_pitch * src_rows bytes, the next one right behind it);
//   u32 dst_offset, dst_bytes (the buffer the destination lies in, and where in it);
//   the source allocations' bytes; the destination buffer's bytes as they are before the pack.
// OUT: per case the destination buffer's bytes after the pack.
// Both buffers are heap blocks of exactly their size: a load beyond the source allocation or a store beyond the
// buffer is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tensor_body.h"

using namespace compeg;

template <uint32_t DTYPE, uint32_t K>
static void run_grid(const TensorPack &t, uint32_t blocks)
{
    for (uint32_t b = 0; b < blocks; b++)
        for (uint32_t lane = 0; lane < kTensorThreads; lane++)
            pack_tensor_block_lane<DTYPE, K>(t, b, lane);
}

template <uint32_t DTYPE>
static void run_dtype(const TensorPack &t, uint32_t blocks, uint32_t k)
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
        fprintf(stderr, "usage: pack_driver IN OUT\n");
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
        uint32_t head[6], geom[4];
        compeg_tensor_spec spec{};
        if (!read_exact(in, head, sizeof head) || !read_exact(in, spec.scale, 12) || !read_exact(in, spec.bias, 12) ||
            !read_exact(in, geom, sizeof geom))
            return 2;
        const uint32_t width = head[0], height = head[1], images = head[2];
        spec.downscale = head[3];
        spec.dtype = head[4];
        spec.order = head[5];
        const size_t image_bytes = size_t(geom[0]) * geom[1], src_bytes = image_bytes * images, dst_bytes = geom[3];
        // (aligned like device allocations are; exactly as long as they are)
        uint8_t *src = static_cast<uint8_t *>(aligned_alloc(256, (src_bytes + 255) / 256 * 256));
        uint8_t *buf = static_cast<uint8_t *>(aligned_alloc(256, (dst_bytes + 255) / 256 * 256));
        if (src_bytes % 256 || dst_bytes % 256 || !src || !buf || !read_exact(in, src, src_bytes) || !read_exact(in, buf, dst_bytes)) {
            fprintf(stderr, "case %u: bad input\n", n);
            return 2;
        }
        TensorPack t;
        uint32_t blocks = 0;
        if (!plan_tensor_pack(t, blocks, src, image_bytes, geom[0], width, height, images, spec, buf + geom[2])) {
            fprintf(stderr, "case %u: no plan\n", n);
            return 3;
        }
        switch (spec.dtype) {
        case COMPEG_TENSOR_U8: run_dtype<COMPEG_TENSOR_U8>(t, blocks, spec.downscale); break;
        case COMPEG_TENSOR_F16: run_dtype<COMPEG_TENSOR_F16>(t, blocks, spec.downscale); break;
        case COMPEG_TENSOR_BF16: run_dtype<COMPEG_TENSOR_BF16>(t, blocks, spec.downscale); break;
        default: run_dtype<COMPEG_TENSOR_F32>(t, blocks, spec.downscale); break;
        }
        if (fwrite(buf, 1, dst_bytes, out) != dst_bytes)
            return 2;
        free(src);
        free(buf);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
