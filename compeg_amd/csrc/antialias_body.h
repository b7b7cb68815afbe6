// Per-lane body of the resize_tensor_antialias_* kernels (resize_kernels.hip): the resized tensor output of
// resize_body.h with a triangle filter that widens with the reduction, as PIL and torch's interpolate(antialias=True)
// have it (include/compeg_hip.h, "Antialiased bilinear").
//
// Written like resize_body.h, whose block sums it uses, and tensor_body.h, whose conversions and stores it uses: what
// one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_antialias compiles the
// very same code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and there is no
// LDS.
//
// Arithmetic contract.  P[c][j][i], the crop, k, scale, bias, the order and the conversions are
// resize_body.h's.  Each axis on its own, n its prefiltered extent (pw or ph), o its output extent, x the output
// coordinate; the host makes, per axis, first(x), count(x) and the weights w_t(x), t = 0 .. count - 1:
//   n <= o (the axis does not shrink): first = i0, count = 2, (w_0, w_1) = (w0, w1) of resize_body.h's bilinear (f32)
//   n > o, in double:  s = double(n) / double(o);  c = s * (x + 0.5)
//     lo = max(int64(c - s + 0.5), 0);  hi = min(int64(c + s + 0.5), n)      (truncated toward zero)
//     first = lo;  count = hi - lo  (>= 1)
//     u_t = max(0, 1 - |(t + lo - c + 0.5) * (1.0 / s)|);  total = u_0 + u_1 + ..  (ascending t);  w_t = float(u_t / total)
//   tap t reads index min(first + t, n - 1)  (the clamp binds only where the axis does not shrink)
// The lane, in f32, every operation rounded on its own (compile with -ffp-contract=off):
//   h(j) = P[j][i_0] * wx_0;  then h = h + (P[j][i_t] * wx_t), t = 1 ..          (horizontal, for row j)
//   m = h(j_0) * wy_0;  then m = m + (h(j_t) * wy_t), t = 1 ..                    (vertical, rows in ascending order)
//   v = (m * scale[c]) + bias[c], converted and stored as tensor_body.h does
// With neither axis shrinking this is resize_body.h's bilinear operation for operation.
//
// Shape: a lane owns one output element (x, y) of all three planes and walks its y taps and, inside them, its x taps in
// the contract's order; a tap is loaded as RGBA pixels and feeds the three planes.  The grid is flat over (image, y, x),
// so the lanes of a wave are neighbours in x: their taps at one t lie s pixels apart and the next t finds the same
// cache lines, their stores are neighbouring elements.  An axis' table is [first[o] | count[o] | w_0[o] | w_1[o] | ..],
// 32-bit words: at one t the lanes of a wave read neighbouring words.  The workgroup's image selects an AntialiasImage
// record (wave-uniform loads) that says where its two tables begin.  count is 129 at the most (the ratio limit, below).
#pragma once

#include <vector>

#include "resize_body.h"

namespace compeg {

constexpr uint32_t kAntialiasMaxRatio = 64; // the flag is rejected beyond n > 64 * o: count <= 2 * 64 + 1

// One image of a launch (device memory; built by the host per call).
struct alignas(8) AntialiasImage {
    const uint8_t *src; // RGBA8 of the image's first pixel (not the crop's)
    uint32_t pitch;     // bytes between rows
    uint32_t cx, cy;    // the crop's origin
    uint32_t pw, ph;    // the prefiltered crop's extent
    uint32_t xtab, ytab; // where the image's x and y tables begin, in words from AntialiasPack::tables
    uint32_t reserved;
};
static_assert(sizeof(AntialiasImage) == 40, "the host writes these records as the kernels read them");

struct AntialiasPack {
    const AntialiasImage *images; // one per image of the launch
    const uint32_t *tables;       // the axis tables of the launch, each once
    uint8_t *dst;                 // [images][3][oh][ow], tight
    uint32_t ow, oh;
    uint32_t items_per_image;  // oh * ow: one lane each
    uint32_t blocks_per_image; // workgroups that hold them (every image has the same output extent)
    uint32_t bgr;              // plane c takes source channel 2 - c
    float scale[3], bias[3];   // per plane
};

// The record of the workgroup's image: wave-uniform loads.
CG_DEV AntialiasImage antialias_image(const AntialiasImage *p)
{
    AntialiasImage im;
#if defined(__HIP_DEVICE_COMPILE__)
    const auto *q = CG_GLOBAL(const uint64_t, reinterpret_cast<const uint64_t *>(p));
    const uint64_t w[5] = {q[0], q[1], q[2], q[3], q[4]};
    __builtin_memcpy(&im, w, sizeof im);
#else
    memcpy(&im, p, sizeof im);
#endif
    return im;
}

CG_DEV uint32_t antialias_word(const uint32_t *p)
{
    return *CG_GLOBAL(const uint32_t, p);
}

CG_DEV float antialias_weight(const uint32_t *p)
{
    const uint32_t u = antialias_word(p);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// One x tap into h (by source channel): h = P * w for a row's first tap, h = h + (P * w) after it; two rounded operations.
template <uint32_t K>
CG_DEV void antialias_tap(float (&h)[3], uint32_t rb, uint32_t ga, float w, bool first)
{
    constexpr float kInv = 1.0f / float(K * K);
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const float p = float(resize_channel(rb, ga, ch)) * kInv;
        const float q = p * w;
        const float sum = h[ch] + q;
        h[ch] = first ? q : sum;
    }
}

// Lane `item` of image `image`: row item / ow, column item % ow.
template <uint32_t DTYPE, uint32_t K>
CG_DEV void antialias_tensor_lane(const AntialiasPack &t, uint32_t image, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    if (item >= t.items_per_image)
        return;
    // (the image is the workgroup's: these are wave-uniform loads)
    const AntialiasImage im = antialias_image(t.images + image);
    const uint32_t y = item / t.ow, x = item - y * t.ow;

    // (axis tables: first[o], count[o], then a row of o weights per t)
    const uint32_t *xtab = t.tables + im.xtab, *ytab = t.tables + im.ytab;
    const uint32_t xfirst = antialias_word(xtab + x), xcount = antialias_word(xtab + t.ow + x);
    const uint32_t yfirst = antialias_word(ytab + y), ycount = antialias_word(ytab + t.oh + y);
    const uint32_t *wx = xtab + 2u * size_t(t.ow) + x, *wy = ytab + 2u * size_t(t.oh) + y;
    const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + size_t(im.cx) * 4u;

    float m[3] = {0.0f, 0.0f, 0.0f}; // by source channel
    for (uint32_t ty = 0; ty < ycount; ty++) {
        const uint32_t j = yfirst + ty < im.ph - 1u ? yfirst + ty : im.ph - 1u;
        const uint8_t *row = origin + size_t(j) * K * im.pitch;
        float h[3] = {0.0f, 0.0f, 0.0f};
        uint32_t tx = 0;
        // k = 1, where a tap is one pixel: four taps at a time while the lane has four left, so that their loads are in
        // flight together (the sums stay in order); at larger k a tap's own k x k loads already overlap, and those
        // kernels walk tap by tap.  What the grouping gained and where it lost: DESIGN.md 5.9, "Measured".
        for (; K == 1u && tx + 4u <= xcount; tx += 4u) {
            uint32_t rb[4], ga[4];
            float w[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) {
                const uint32_t i = xfirst + tx + u < im.pw - 1u ? xfirst + tx + u : im.pw - 1u;
                w[u] = antialias_weight(wx + size_t(tx + u) * t.ow);
                resize_block<K>(row + size_t(i) * K * 4u, im.pitch, rb[u], ga[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++)
                antialias_tap<K>(h, rb[u], ga[u], w[u], tx + u == 0u);
        }
        for (; tx < xcount; tx++) {
            const uint32_t i = xfirst + tx < im.pw - 1u ? xfirst + tx : im.pw - 1u;
            const float w = antialias_weight(wx + size_t(tx) * t.ow);
            uint32_t rb, ga;
            resize_block<K>(row + size_t(i) * K * 4u, im.pitch, rb, ga);
            antialias_tap<K>(h, rb, ga, w, tx == 0u);
        }
        const float w = antialias_weight(wy + size_t(ty) * t.oh);
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            const float q = h[ch] * w;
            const float sum = m[ch] + q;
            m[ch] = ty == 0u ? q : sum;
        }
    }

    const size_t plane = size_t(t.oh) * t.ow;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const uint32_t c = t.bgr ? 2u - ch : ch;
        // (constant indices: the launch's arguments stay in scalar registers)
        const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
        const float scaled = m[ch] * scale;
        const float val = scaled + bias;
        uint8_t *p = t.dst + ((size_t(image) * 3u + c) * plane + item) * kElem;
        tensor_store_run(p, TensorVec{{tensor_bits<DTYPE>(val), 0u, 0u, 0u}}, kElem);
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_image workgroups for every image, one image behind
// the other.
template <uint32_t DTYPE, uint32_t K>
CG_DEV void antialias_tensor_block_lane(const AntialiasPack &t, uint32_t block, uint32_t lane)
{
    const uint32_t image = block / t.blocks_per_image;
    antialias_tensor_lane<DTYPE, K>(t, image, (block - image * t.blocks_per_image) * kTensorThreads + lane);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

// Whether the flag takes an axis of n prefiltered samples and o outputs.
inline bool antialias_ratio_ok(uint32_t n, uint32_t o)
{
    return uint64_t(n) <= uint64_t(kAntialiasMaxRatio) * o;
}

// The axis tables of one launch, each distinct (n, o) once.  `words` may begin with `front` words that are not tables
// (the library keeps the launch's records there, so that records and tables are built in the one block that travels).
struct AntialiasTables {
    struct Axis {
        uint32_t n, o, at;
    };
    std::vector<Axis> axes;
    std::vector<uint32_t> words;
    size_t front = 0;

    explicit AntialiasTables(size_t front_words = 0) : words(front_words, 0u), front(front_words) {}

    // Where the table of an axis of n samples and o outputs begins, in words behind `front`, built if this launch has
    // none yet.  False: more words than 32 bits count.
    bool axis(uint32_t n, uint32_t o, uint32_t &at)
    {
        for (const Axis &a : axes)
            if (a.n == n && a.o == o) {
                at = a.at;
                return true;
            }
        const size_t begin = words.size() - front;
        std::vector<double> u;
        std::vector<uint32_t> first, count;
        uint32_t taps = 2;
        const double s = double(n) / double(o), inv = 1.0 / s;
        if (n > o) {
            taps = 1;
            first.resize(o);
            count.resize(o);
            for (uint32_t x = 0; x < o; x++) {
                const double c = s * (double(x) + 0.5);
                const int64_t a = int64_t(c - s + 0.5), b = int64_t(c + s + 0.5);
                const int64_t lo = a > 0 ? a : 0, hi = b < int64_t(n) ? b : int64_t(n);
                first[x] = uint32_t(lo);
                count[x] = uint32_t(hi - lo);
                taps = count[x] > taps ? count[x] : taps;
            }
        }
        const uint64_t total_words = uint64_t(begin) + (uint64_t(taps) + 2u) * o;
        if (total_words > 0xffffffffull)
            return false;
        words.resize(front + size_t(total_words), 0u); // (a weight past an output's own count: 0, never read)
        uint32_t *tab = words.data() + front + begin;
        const auto bits = [](float f) {
            uint32_t b;
            memcpy(&b, &f, 4);
            return b;
        };
        if (n <= o) {
            const float ratio = float(s);
            for (uint32_t x = 0; x < o; x++) {
                // resize_body.h's bilinear taps, operation for operation
                const float a = float(x) + 0.5f;
                const float b = a * ratio;
                const float d = b - 0.5f;
                const float f = d > 0.0f ? d : 0.0f;
                const uint32_t i = uint32_t(f), i0 = i < n - 1u ? i : n - 1u;
                const float w1 = f - float(i0);
                const float w0 = 1.0f - w1;
                tab[x] = i0;
                tab[size_t(o) + x] = 2u;
                tab[2u * size_t(o) + x] = bits(w0);
                tab[3u * size_t(o) + x] = bits(w1);
            }
        } else {
            u.resize(taps);
            for (uint32_t x = 0; x < o; x++) {
                const double c = s * (double(x) + 0.5);
                double total = 0.0;
                for (uint32_t t = 0; t < count[x]; t++) {
                    const double d = (double(int64_t(t) + int64_t(first[x])) - c + 0.5) * inv;
                    const double v = 1.0 - (d < 0.0 ? -d : d);
                    u[t] = v > 0.0 ? v : 0.0;
                    total = t == 0u ? u[t] : total + u[t];
                }
                tab[x] = first[x];
                tab[size_t(o) + x] = count[x];
                for (uint32_t t = 0; t < count[x]; t++)
                    tab[(2u + size_t(t)) * o + x] = bits(float(u[t] / total));
            }
        }
        axes.push_back(Axis{n, o, uint32_t(begin)});
        at = uint32_t(begin);
        return true;
    }
};

// One image's record, its tables made in `tables` if they are not there yet: the crop (x, y, width, height) of the image
// at src whose rows are pitch bytes apart, for an output of ow x oh.  False: the crop is smaller than the downscale
// factor, an axis shrinks by more than kAntialiasMaxRatio, or the tables outgrow 32 bits.  (That the crop lies inside
// the image is the caller's to check.)
inline bool plan_antialias_image(AntialiasImage &im, AntialiasTables &tables, const void *src, uint32_t pitch, const compeg_rect &crop,
                                 uint32_t k, uint32_t ow, uint32_t oh)
{
    if (k == 0u || crop.width < k || crop.height < k || ow == 0u || oh == 0u)
        return false;
    im = AntialiasImage{};
    im.src = static_cast<const uint8_t *>(src);
    im.pitch = pitch;
    im.cx = crop.x;
    im.cy = crop.y;
    im.pw = crop.width / k;
    im.ph = crop.height / k;
    if (!antialias_ratio_ok(im.pw, ow) || !antialias_ratio_ok(im.ph, oh))
        return false;
    return tables.axis(im.pw, ow, im.xtab) && tables.axis(im.ph, oh, im.ytab);
}

// The launch of one pack: fills t, all but the records' and the tables' addresses, and says how many workgroups the
// grid's one dimension has.  False: the specs are not ones the kernels take, or the grid would not fit.
inline bool plan_antialias_pack(AntialiasPack &t, uint32_t &grid_blocks, uint32_t images, const compeg_tensor_spec &spec,
                                const compeg_resize_spec &resize, void *dst)
{
    const uint32_t k = spec.downscale;
    if (spec.dtype > COMPEG_TENSOR_F32 || (k != 1u && k != 2u && k != 4u && k != 8u) ||
        resize.filter != (COMPEG_RESIZE_BILINEAR | COMPEG_RESIZE_ANTIALIAS) || resize.out_width == 0u || resize.out_height == 0u ||
        resize.out_width > 65535u || resize.out_height > 65535u || images == 0u)
        return false;
    t = AntialiasPack{};
    t.dst = static_cast<uint8_t *>(dst);
    t.ow = resize.out_width;
    t.oh = resize.out_height;
    const uint64_t items = uint64_t(t.oh) * t.ow;
    const uint64_t blocks = (items + kTensorThreads - 1u) / kTensorThreads;
    // 32 bits hold an image's lanes, the last workgroup's beyond the image included; 31 the grid's workgroups
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
