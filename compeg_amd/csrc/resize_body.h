// Per-lane body of the resize_tensor_* kernels (resize_kernels.hip): a crop of the RGBA8 output of a decode,
// block-averaged, resized to a fixed extent and packed into the planar tensor a model reads (include/compeg_hip.h,
// "Resized tensor output").
//
// Written like tensor_body.h, whose conversions and stores it uses: what one lane executes, GPU-only instructions
// behind __HIP_DEVICE_COMPILE__, so that tests/emul_resize compiles the very same code with g++ under ASan/UBSan and
// drives it lane by lane.  No lane talks to another one and there is no LDS.
//
// Arithmetic contract, k = downscale, the crop (cx, cy, cw, ch), pw = cw / k, ph = ch / k:
//   P[c][j][i] = float(s) * (1 / k^2), s the integer sum of the channel over the k x k pixels at rows cy + k*j ..,
//                columns cx + k*i ..                                  (exact in f32)
//   rx = float(double(pw) / double(ow)), ry likewise: made by the host (plan_resize_image), no division here
//   per axis:  a = float(x) + 0.5f;  b = a * rx
//     nearest:   i = min(int(floor(b)), pw - 1)
//     bilinear:  s = max(b - 0.5f, 0);  i0 = min(int(floor(s)), pw - 1);  i1 = min(i0 + 1, pw - 1);
//                w1 = s - float(i0);  w0 = 1.0f - w1
//   nearest:   m = P[c][j][i]
//   bilinear:  top = (P[j0][i0] * wx0) + (P[j0][i1] * wx1);  bot likewise on row j1;  m = (top * wy0) + (bot * wy1)
//   v = (m * scale[c]) + bias[c], converted and stored as tensor_body.h does
// Every operation is rounded on its own: compile with -ffp-contract=off.  All taps lie inside the crop.
//
// Shape: like pack_tensor a lane produces, for each of the three planes, the run of output elements that is 16 bytes
// of one output row; its y taps and weights are computed once.  The grid is flat over (image, row, run); the
// workgroup's image selects a ResizeImage record in device memory (the images of a launch differ in extent, crop and
// address), read with wave-uniform loads.  A tap is loaded as RGBA pixels and feeds all three planes.  A crop begins
// at any pixel, so 4 bytes is the alignment a tap's address has, and a pixel is what a load of this file asks for.
#pragma once

#include "tensor_body.h"

namespace compeg {

// One image of a launch (device memory; built by the host per call).
struct alignas(8) ResizeImage {
    const uint8_t *src; // RGBA8 of the image's first pixel (not the crop's)
    uint32_t pitch;     // bytes between rows
    uint32_t cx, cy;    // the crop's origin
    uint32_t pw, ph;    // the prefiltered crop's extent
    float rx, ry;       // float(double(pw) / double(ow)), float(double(ph) / double(oh))
    uint32_t reserved;
};
static_assert(sizeof(ResizeImage) == 40, "the host writes these records as the kernels read them");

struct ResizePack {
    const ResizeImage *images; // one per image of the launch
    uint8_t *dst;              // [images][3][oh][ow], tight
    uint32_t ow, oh;
    uint32_t runs_per_row;     // ceil(ow / elements of a 16-byte run)
    uint32_t items_per_image;  // oh * runs_per_row: one lane each
    uint32_t blocks_per_image; // workgroups that hold them (every image has the same output extent)
    uint32_t bgr;              // plane c takes source channel 2 - c
    float scale[3], bias[3];   // per plane
};

// One axis' taps for output coordinate x of an axis with n prefiltered samples.
struct ResizeTaps {
    uint32_t i0, i1;
    float w0, w1;
};

template <uint32_t FILTER>
CG_DEV ResizeTaps resize_taps(uint32_t x, float ratio, uint32_t n)
{
    const float a = float(x) + 0.5f;
    const float b = a * ratio;
    ResizeTaps t;
    if (FILTER == COMPEG_RESIZE_NEAREST) {
        const uint32_t i = uint32_t(b); // b >= 0: truncation is floor
        t.i0 = t.i1 = i < n - 1u ? i : n - 1u;
        t.w0 = 1.0f;
        t.w1 = 0.0f;
    } else {
        const float d = b - 0.5f;
        const float s = d > 0.0f ? d : 0.0f;
        const uint32_t i = uint32_t(s);
        t.i0 = i < n - 1u ? i : n - 1u;
        t.i1 = t.i0 + 1u < n - 1u ? t.i0 + 1u : n - 1u;
        t.w1 = s - float(t.i0);
        t.w0 = 1.0f - t.w1;
    }
    return t;
}

// The record of the workgroup's image: wave-uniform loads.
CG_DEV ResizeImage resize_image(const ResizeImage *p)
{
    ResizeImage im;
#if defined(__HIP_DEVICE_COMPILE__)
    const auto *q = CG_GLOBAL(const uint64_t, reinterpret_cast<const uint64_t *>(p));
    const uint64_t w[5] = {q[0], q[1], q[2], q[3], q[4]};
    __builtin_memcpy(&im, w, sizeof im);
#else
    memcpy(&im, p, sizeof im);
#endif
    return im;
}

// Sums of R | B << 16 and of G | A << 16 over the K x K pixels whose first one is at p: 64 pixels of 255 stay below 2^16.
// Every load is one pixel, 4 bytes at an address that 4 divides -- all a crop's origin guarantees.  (The compiler joins
// the loads of a block row into one of 8 or 16 bytes, for which the hardware asks no more than that.)
template <uint32_t K>
CG_DEV void resize_block(const uint8_t *p, uint32_t pitch, uint32_t &rb, uint32_t &ga)
{
    rb = ga = 0u;
    for (uint32_t r = 0; r < K; r++, p += pitch) {
#pragma unroll
        for (uint32_t i = 0; i < K; i++) {
            const uint32_t v = *CG_GLOBAL(const uint32_t, reinterpret_cast<const uint32_t *>(p + 4u * i));
            rb += v & 0x00ff00ffu;
            ga += (v >> 8) & 0x00ff00ffu;
        }
    }
}

CG_DEV uint32_t resize_channel(uint32_t rb, uint32_t ga, uint32_t ch)
{
    return ch == 0u ? rb & 0xffffu : (ch == 1u ? ga & 0xffffu : rb >> 16);
}

// v, moved up by one element of kElem bytes, with `bits` as its new first element (runs are built last element first:
// every index is a constant, nothing lives in private memory)
template <uint32_t kElem>
CG_DEV void resize_push(TensorVec &v, uint32_t bits)
{
    if constexpr (kElem == 4u) {
        v.w[3] = v.w[2];
        v.w[2] = v.w[1];
        v.w[1] = v.w[0];
        v.w[0] = bits;
    } else {
        constexpr uint32_t sh = 8u * kElem, back = 32u - sh;
        v.w[3] = (v.w[3] << sh) | (v.w[2] >> back);
        v.w[2] = (v.w[2] << sh) | (v.w[1] >> back);
        v.w[1] = (v.w[1] << sh) | (v.w[0] >> back);
        v.w[0] = (v.w[0] << sh) | bits;
    }
}

// Lane `item` of image `image`: row item / runs_per_row, run item % runs_per_row.
template <uint32_t DTYPE, uint32_t K, uint32_t FILTER>
CG_DEV void resize_tensor_lane(const ResizePack &t, uint32_t image, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    constexpr uint32_t kRun = 16u / kElem; // output elements of a lane, per plane
    constexpr float kInv = 1.0f / float(K * K);
    if (item >= t.items_per_image)
        return;
    // (the image is the workgroup's: these are wave-uniform loads)
    const ResizeImage im = resize_image(t.images + image);
    const uint32_t y = item / t.runs_per_row, run = item - y * t.runs_per_row;
    const uint32_t x0 = run * kRun;
    const uint32_t count = t.ow - x0 < kRun ? t.ow - x0 : kRun; // elements of this run inside the row

    const ResizeTaps ty = resize_taps<FILTER>(y, im.ry, im.ph);
    const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + size_t(im.cx) * 4u;
    const uint8_t *row0 = origin + size_t(ty.i0) * K * im.pitch, *row1 = origin + size_t(ty.i1) * K * im.pitch;

    TensorVec out[3] = {{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}}; // by source channel
    for (uint32_t j = count; j-- > 0u;) {
        const ResizeTaps tx = resize_taps<FILTER>(x0 + j, im.rx, im.pw);
        const size_t at0 = size_t(tx.i0) * K * 4u, at1 = size_t(tx.i1) * K * 4u;
        uint32_t rb00, ga00, rb01 = 0u, ga01 = 0u, rb10 = 0u, ga10 = 0u, rb11 = 0u, ga11 = 0u;
        resize_block<K>(row0 + at0, im.pitch, rb00, ga00);
        if (FILTER == COMPEG_RESIZE_BILINEAR) {
            resize_block<K>(row0 + at1, im.pitch, rb01, ga01);
            resize_block<K>(row1 + at0, im.pitch, rb10, ga10);
            resize_block<K>(row1 + at1, im.pitch, rb11, ga11);
        }
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            // (constant indices: the launch's arguments stay in scalar registers)
            const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
            float m = float(resize_channel(rb00, ga00, ch)) * kInv;
            if (FILTER == COMPEG_RESIZE_BILINEAR) {
                const float p01 = float(resize_channel(rb01, ga01, ch)) * kInv;
                const float p10 = float(resize_channel(rb10, ga10, ch)) * kInv;
                const float p11 = float(resize_channel(rb11, ga11, ch)) * kInv;
                const float t0 = m * tx.w0, t1 = p01 * tx.w1;
                const float top = t0 + t1;
                const float b0 = p10 * tx.w0, b1 = p11 * tx.w1;
                const float bot = b0 + b1;
                const float mt = top * ty.w0, mb = bot * ty.w1;
                m = mt + mb;
            }
            const float scaled = m * scale;
            const float val = scaled + bias;
            resize_push<kElem>(out[ch], tensor_bits<DTYPE>(val));
        }
    }

    const size_t plane = size_t(t.oh) * t.ow;
    const size_t at = size_t(y) * t.ow + x0;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const uint32_t c = t.bgr ? 2u - ch : ch;
        uint8_t *p = t.dst + ((size_t(image) * 3u + c) * plane + at) * kElem;
        tensor_store_run(p, out[ch], count * kElem);
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_image workgroups for every image, one image behind
// the other.
template <uint32_t DTYPE, uint32_t K, uint32_t FILTER>
CG_DEV void resize_tensor_block_lane(const ResizePack &t, uint32_t block, uint32_t lane)
{
    const uint32_t image = block / t.blocks_per_image;
    resize_tensor_lane<DTYPE, K, FILTER>(t, image, (block - image * t.blocks_per_image) * kTensorThreads + lane);
}

// One image's record (host side; the emulator plans with it too): the crop (x, y, width, height) of the image at src
// whose rows are pitch bytes apart, for an output of ow x oh.  False: the crop is smaller than the downscale factor.
// (That the crop lies inside the image is the caller's to check.)
inline bool plan_resize_image(ResizeImage &im, const void *src, uint32_t pitch, const compeg_rect &crop, uint32_t k, uint32_t ow,
                              uint32_t oh)
{
    if (k == 0u || crop.width < k || crop.height < k || ow == 0u || oh == 0u)
        return false;
    im = ResizeImage{};
    im.src = static_cast<const uint8_t *>(src);
    im.pitch = pitch;
    im.cx = crop.x;
    im.cy = crop.y;
    im.pw = crop.width / k;
    im.ph = crop.height / k;
    im.rx = float(double(im.pw) / double(ow));
    im.ry = float(double(im.ph) / double(oh));
    return true;
}

// The launch of one pack (host side): fills t, all but the records' address, and says how many workgroups the grid's
// one dimension has.  False: the specs are not ones the kernels take, or the grid would not fit.
inline bool plan_resize_pack(ResizePack &t, uint32_t &grid_blocks, uint32_t images, const compeg_tensor_spec &spec,
                             const compeg_resize_spec &resize, void *dst)
{
    const uint32_t k = spec.downscale;
    if (spec.dtype > COMPEG_TENSOR_F32 || (k != 1u && k != 2u && k != 4u && k != 8u) || resize.filter > COMPEG_RESIZE_BILINEAR ||
        resize.out_width == 0u || resize.out_height == 0u || resize.out_width > 65535u || resize.out_height > 65535u || images == 0u)
        return false;
    const uint32_t run = 16u / tensor_elem_bytes(spec.dtype);
    t = ResizePack{};
    t.dst = static_cast<uint8_t *>(dst);
    t.ow = resize.out_width;
    t.oh = resize.out_height;
    t.runs_per_row = (t.ow + run - 1u) / run;
    const uint64_t items = uint64_t(t.oh) * t.runs_per_row;
    const uint64_t blocks = (items + kTensorThreads - 1u) / kTensorThreads;
    // (65535 rows of 16384 runs at the most: an image's lanes fit 32 bits; the grid's workgroups must fit 31)
    if (blocks * images > 0x7fffffffull)
        return false;
    t.items_per_image = uint32_t(items);
    t.blocks_per_image = uint32_t(blocks);
    t.bgr = spec.order == COMPEG_TENSOR_BGR ? 1u : 0u;
    for (int c = 0; c < 3; c++) {
        t.scale[c] = spec.scale[c];
        t.bias[c] = spec.bias[c];
    }
    grid_blocks = uint32_t(blocks * images);
    return true;
}

} // namespace compeg
