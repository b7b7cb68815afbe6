// Per-lane body of the pack_tensor_* kernels (tensor_kernels.hip): the RGBA8 output of a decode, packed into the
// planar tensor a model reads (include/compeg_hip.h, "Tensor output").
//
// Written like kernels_body.h: what one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__ next to a
// plain C++ equivalent, so that tests/emul_tensor compiles the very same code with g++ under ASan/UBSan and drives it
// lane by lane.  No lane talks to another one and there is no LDS.
//
// Arithmetic contract, per output element (plane c, row y, column x), k = downscale:
//   s = integer sum of the plane's source channel over the k x k block of pixels at row k*y, column k*x
//   m = float(s) * (1 / k^2)                  exact in f32: s <= 64 * 255, the factor a power of two
//   v = (m * scale[c]) + bias[c]              two f32 operations, each rounded: compile with -ffp-contract=off
//   stored: v (f32); v rounded to nearest even (f16, bf16); rint(v), half to even, clamped to 0..255 (u8)
//
// Shape: a lane produces, for each of the three planes, the run of output elements that is 16 bytes of one output
// row -- 16 x u8, 8 x f16 / bf16, 4 x f32 -- and reads the k source rows under it with 16-byte loads.  Source rows begin
// on 64-byte boundaries and the allocation has whole 16-pixel MCUs both ways, so a 16-byte load that starts on a
// pixel of the image stays inside the allocation; what it brings in from beyond the columns the row needs lands in
// elements that are never stored.  The destination is tight: rows, planes and images begin wherever the element
// counts put them, so a run goes out as one 16-byte store where its address allows it and in aligned pieces of
// 8, 4, 2 and 1 bytes where it does not (or where the row ends inside the run); no byte outside the tensor is written.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "compeg_hip.h"

#if defined(__HIPCC__)
#define CG_DEV __device__ __forceinline__
#else
#define CG_DEV static inline
#endif

// (see kernels_body.h: states that p is a global-memory pointer; a plain pointer on the host)
#if defined(__HIP_DEVICE_COMPILE__)
#define CG_GLOBAL(T, p) (reinterpret_cast<__attribute__((address_space(1))) T *>(reinterpret_cast<uintptr_t>(p)))
#else
#define CG_GLOBAL(T, p) (p)
#endif

#ifndef CG_TENSOR_NT_STORES
#define CG_TENSOR_NT_STORES 1 // whole 16-byte runs leave as non-temporal stores (written once, read by another kernel much later)
#endif
#ifndef CG_TENSOR_NT_LOADS
#define CG_TENSOR_NT_LOADS 1 // the source is read once
#endif

namespace compeg {

constexpr uint32_t kTensorThreads = 256; // lanes per workgroup of the pack kernels

// One launch: `images` sources of the same extent, `src_image_stride` bytes apart, rows `src_pitch` bytes apart.
struct TensorPack {
    const uint8_t *src; // RGBA8 of the first image
    uint8_t *dst;       // [images][3][oh][ow], tight
    size_t src_image_stride;
    uint32_t src_pitch;
    uint32_t ow, oh;           // output extent: floor(W / k), floor(H / k)
    uint32_t runs_per_row;     // ceil(ow / elements of a 16-byte run)
    uint32_t items_per_image;  // oh * runs_per_row: one lane each
    uint32_t blocks_per_image; // workgroups that hold them
    uint32_t bgr;              // plane c takes source channel 2 - c
    float scale[3], bias[3];   // per plane
};

struct alignas(16) TensorVec {
    uint32_t w[4];
};

constexpr uint32_t tensor_elem_bytes(uint32_t dtype)
{
    return dtype == COMPEG_TENSOR_U8 ? 1u : (dtype == COMPEG_TENSOR_F32 ? 4u : 2u);
}

CG_DEV uint32_t tensor_f32_bits(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// f32 -> f16, round to nearest even, subnormals and overflow to infinity as IEEE 754 has them.
CG_DEV uint32_t tensor_f16_bits(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = static_cast<_Float16>(v); // v_cvt_f16_f32: round to nearest even, f16 denormals on
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
#else
    const uint32_t u = tensor_f32_bits(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u)
        return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u | ((a >> 13) & 0x3ffu) : 0u);
    if (a >= 0x47800000u) // 65536 and beyond (what rounds up to it from below is handled by the carry further down)
        return sign | 0x7c00u;
    if (a < 0x38800000u) { // below 2^-14: a subnormal half, or zero
        if (a < 0x33000000u) // below 2^-25: rounds to zero (2^-25 itself is a tie, to even: zero)
            return sign;
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - (a >> 23); // value = mant * 2^(e - 150); ulp 2^-24
        const uint32_t q = mant >> shift, rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
    }
    const uint32_t r = a - 0x38000000u; // exponent rebias (127 - 15) << 23
    return sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
#endif
}

// f32 -> bf16, round to nearest even on the bit pattern.
CG_DEV uint32_t tensor_bf16_bits(float v)
{
    const uint32_t u = tensor_f32_bits(v);
    if ((u & 0x7fffffffu) > 0x7f800000u)
        return (u >> 16) | 0x40u; // NaN stays NaN
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

CG_DEV uint32_t tensor_u8_bits(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_fmed3f(__builtin_rintf(v), 0.0f, 255.0f); // (NaN: 0)
    return uint32_t(r);
#else
    const float r = __builtin_rintf(v); // half to even in the default rounding mode
    return !(r > 0.0f) ? 0u : (r > 255.0f ? 255u : uint32_t(r));
#endif
}

template <uint32_t DTYPE>
CG_DEV uint32_t tensor_bits(float v)
{
    return DTYPE == COMPEG_TENSOR_U8 ? tensor_u8_bits(v)
           : DTYPE == COMPEG_TENSOR_F16 ? tensor_f16_bits(v)
           : DTYPE == COMPEG_TENSOR_BF16 ? tensor_bf16_bits(v)
                                         : tensor_f32_bits(v);
}

CG_DEV TensorVec tensor_load16(const uint8_t *p)
{
#if CG_TENSOR_NT_LOADS && defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_nontemporal_load(
        reinterpret_cast<const __attribute__((address_space(1))) u32x4 *>(reinterpret_cast<uintptr_t>(p)));
    return TensorVec{{v.x, v.y, v.z, v.w}};
#else
    return *CG_GLOBAL(const TensorVec, reinterpret_cast<const TensorVec *>(p));
#endif
}

CG_DEV void tensor_store16(uint8_t *p, const TensorVec &v)
{
#if CG_TENSOR_NT_STORES && defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(u32x4{v.w[0], v.w[1], v.w[2], v.w[3]},
                                reinterpret_cast<__attribute__((address_space(1))) u32x4 *>(reinterpret_cast<uintptr_t>(p)));
#else
    *CG_GLOBAL(TensorVec, reinterpret_cast<TensorVec *>(p)) = v;
#endif
}

// The first `nbytes` (a multiple of the element size, like p) of v to p: one 16-byte store if that is what the
// address and the count allow, else pieces, each as wide as its own address and what is left allow.
CG_DEV void tensor_store_run(uint8_t *p, const TensorVec &v, uint32_t nbytes)
{
    const uintptr_t addr = reinterpret_cast<uintptr_t>(p);
    if (nbytes == 16u && (addr & 15u) == 0u) {
        tensor_store16(p, v);
        return;
    }
    const uint64_t lo = uint64_t(v.w[0]) | (uint64_t(v.w[1]) << 32), hi = uint64_t(v.w[2]) | (uint64_t(v.w[3]) << 32);
    uint32_t at = 0;
    while (at < nbytes) {
        const uint32_t a = uint32_t(addr + at) & 15u;
        uint32_t size = a ? (a & (0u - a)) : 16u; // the address's alignment ...
        while (size > nbytes - at)                // ... and no more than what is left
            size >>= 1;
        // bytes at .. at + 7 of the run (a piece is 8 bytes at most here: 16 left at an aligned address went out above)
        const uint64_t piece = at >= 8u ? hi >> (8u * (at - 8u)) : (at ? (lo >> (8u * at)) | (hi << (64u - 8u * at)) : lo);
        uint8_t *q = p + at;
        if (size >= 8u)
            *CG_GLOBAL(uint64_t, reinterpret_cast<uint64_t *>(q)) = piece;
        else if (size == 4u)
            *CG_GLOBAL(uint32_t, reinterpret_cast<uint32_t *>(q)) = uint32_t(piece);
        else if (size == 2u)
            *CG_GLOBAL(uint16_t, reinterpret_cast<uint16_t *>(q)) = uint16_t(piece);
        else
            *CG_GLOBAL(uint8_t, q) = uint8_t(piece);
        at += size >= 8u ? 8u : size;
    }
}

// Lane `item` of image `image`: row item / runs_per_row, run item % runs_per_row.
template <uint32_t DTYPE, uint32_t K>
CG_DEV void pack_tensor_lane(const TensorPack &t, uint32_t image, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    constexpr uint32_t kRun = 16u / kElem;      // output elements of a lane, per plane
    constexpr uint32_t kLoads = kRun * K / 4u;  // 16-byte loads (four pixels) per source row
    if (item >= t.items_per_image)
        return;
    const uint32_t y = item / t.runs_per_row, run = item - y * t.runs_per_row;
    const uint32_t x0 = run * kRun;
    const uint32_t count = t.ow - x0 < kRun ? t.ow - x0 : kRun; // elements of this run inside the row
    const uint32_t need_px = count * K;                         // source pixels a row of the run needs

    // sums of R | B << 16 and of G | A << 16 per output element: 64 pixels of 255 stay below 2^16
    uint32_t rb[kRun], ga[kRun];
#pragma unroll
    for (uint32_t j = 0; j < kRun; j++)
        rb[j] = ga[j] = 0u;
    const uint8_t *row = t.src + size_t(image) * t.src_image_stride + size_t(y) * K * t.src_pitch + size_t(x0) * K * 4u;
    for (uint32_t r = 0; r < K; r++, row += t.src_pitch) {
#pragma unroll
        for (uint32_t i = 0; i < kLoads; i++) {
            // a load that begins beyond the run's pixels feeds elements that are not stored: it reads the run's first
            // pixels instead (inside the image)
            const TensorVec v = tensor_load16(row + (4u * i < need_px ? 16u * i : 0u));
#pragma unroll
            for (uint32_t p = 0; p < 4u; p++) {
                const uint32_t j = (4u * i + p) / K;
                rb[j] += v.w[p] & 0x00ff00ffu;
                ga[j] += (v.w[p] >> 8) & 0x00ff00ffu;
            }
        }
    }

    constexpr float kInv = 1.0f / float(K * K);
    const size_t plane = size_t(t.oh) * t.ow;
    const size_t at = size_t(y) * t.ow + x0;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) { // source channel; its plane: ch, or 2 - ch
        const uint32_t c = t.bgr ? 2u - ch : ch;
        // (constant indices: the launch's arguments stay in scalar registers)
        const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
        TensorVec out{{0u, 0u, 0u, 0u}};
#pragma unroll
        for (uint32_t j = 0; j < kRun; j++) {
            const uint32_t s = ch == 0u ? rb[j] & 0xffffu : (ch == 1u ? ga[j] & 0xffffu : rb[j] >> 16);
            const float m = float(s) * kInv;
            const float scaled = m * scale;
            const float val = scaled + bias;
            out.w[j * kElem / 4u] |= tensor_bits<DTYPE>(val) << (8u * (j * kElem % 4u));
        }
        uint8_t *p = t.dst + ((size_t(image) * 3u + c) * plane + at) * kElem;
        tensor_store_run(p, out, count * kElem);
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_image workgroups for every image, one image behind
// the other.
template <uint32_t DTYPE, uint32_t K>
CG_DEV void pack_tensor_block_lane(const TensorPack &t, uint32_t block, uint32_t lane)
{
    const uint32_t image = block / t.blocks_per_image;
    pack_tensor_lane<DTYPE, K>(t, image, (block - image * t.blocks_per_image) * kTensorThreads + lane);
}

// The launch of one pack (host side; the emulator plans with it too): fills t and says how many workgroups the grid's
// one dimension has.  False: the spec or the extent is not one the kernels take, or the grid would not fit.
inline bool plan_tensor_pack(TensorPack &t, uint32_t &grid_blocks, const void *src, size_t src_image_stride, uint32_t src_pitch,
                             uint32_t width, uint32_t height, uint32_t images, const compeg_tensor_spec &spec, void *dst)
{
    const uint32_t k = spec.downscale;
    if (spec.dtype > COMPEG_TENSOR_F32 || (k != 1u && k != 2u && k != 4u && k != 8u) || width < k || height < k || images == 0u)
        return false;
    const uint32_t run = 16u / tensor_elem_bytes(spec.dtype);
    t = TensorPack{};
    t.src = static_cast<const uint8_t *>(src);
    t.dst = static_cast<uint8_t *>(dst);
    t.src_image_stride = src_image_stride;
    t.src_pitch = src_pitch;
    t.ow = width / k;
    t.oh = height / k;
    t.runs_per_row = (t.ow + run - 1u) / run;
    const uint64_t items = uint64_t(t.oh) * t.runs_per_row;
    const uint64_t blocks = (items + kTensorThreads - 1u) / kTensorThreads;
    // 32 bits hold an image's lanes (65535 rows of 16384 runs at the most), 31 the grid's workgroups: every tensor that
    // fits a card's memory stays far below that
    if (items > 0xffffffffull - kTensorThreads || blocks * images > 0x7fffffffull)
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
