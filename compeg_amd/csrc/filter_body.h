// Per-lane body of the filter_tensor_* kernels (filter_kernels.hip): the region tensor output of region_body.h with
// PIL's separable resampling kernels -- box, triangle, bicubic (a = -0.5), Lanczos of support 3 -- each widened with the
// reduction (include/compeg_hip.h, "Filtered tensor output").  The four differ in their tables only: one body serves all.
//
// Written like region_body.h and antialias_body.h, whose records, table layout, block sums, conversions and stores it
// uses: what one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_filter compiles
// the very same code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and there is
// no LDS.
//
// Arithmetic contract.  P[c][j][i], the crop, k, scale, bias, the order, the conversions and the pad
// value are region_body.h's.  Each axis on its own, n its prefiltered extent, o the inner extent (dw or dh), S the
// kernel's support (0.5, 1, 2, 3), x the output coordinate; the host makes, per axis, in double:
//   s = double(n) / double(o);  sc = max(s, 1.0);  sup = S * sc;  inv = 1.0 / sc;  c = s * (x + 0.5)
//   lo = max(int64(c - sup + 0.5), 0);  hi = min(int64(c + sup + 0.5), n)      (truncated toward zero)
//   first = lo;  count = hi - lo  (>= 1)
//   u_t = f((t + lo - c + 0.5) * inv);  total = u_0 + u_1 + ..  (ascending t);  w_t = float(u_t / total)
//   tap t reads index first + t  (always inside the axis; weights may be negative)
// f: filter_kernel_value, below.  The lane, in f32, every operation rounded on its own (compile with -ffp-contract=off):
//   h(j) = P[j][i_0] * wx_0;  then h = h + (P[j][i_t] * wx_t), t = 1 ..          (horizontal, for row j)
//   m = h(j_0) * wy_0;  then m = m + (h(j_t) * wy_t), t = 1 ..                    (vertical, rows in ascending order)
//   v = (m * scale[c]) + bias[c], converted and stored as tensor_body.h does
//
// Shape: a lane owns one column x of a slot and a band of R consecutive rows, R a compile-time constant.  Bands are
// counted from the inner rectangle's first row, so every band but the rectangle's last holds R of its rows; the rows of
// the slot above and below the rectangle fall into bands of the same grid (band 0 may begin above the slot: those rows
// are nobody's), and every element of the slot is one lane's.  A lane inside the rectangle walks the source rows its
// band's outputs tap -- first(y_0) .. first(y_last) + count(y_last) - 1, first and first + count never fall as y grows --
// once, in ascending order; it makes h(j) once per row with the contract's x walk and gives it to every band row whose
// tap range holds j: m_r = (j is the row's first tap) ? q : m_r + q -- for each output exactly the contract's
// operations in the contract's order, so the result does not depend on R.  The R x 3 sums are indexed by constants only
// (full unrolling, predicates).  The lanes of a wave are neighbours in x within a band: the y table words are the same
// for the whole wave, a row's stores are neighbouring elements.  A lane outside the rectangle stores the pad and loads
// neither a pixel nor a table word.  count is 129 at the most (the tap limit, below).
#pragma once

#include <cmath>

#include "region_body.h"

namespace compeg {

constexpr uint32_t kFilterKernels = 4;
constexpr uint32_t kFilterMaxTaps = 128; // an axis is rejected when n * 2S > 128 * o: count <= 129

// Twice the support of a kernel: 1, 2, 4, 6.
constexpr uint32_t filter_twice_support(uint32_t kernel)
{
    return kernel == COMPEG_FILTER_BOX ? 1u : kernel == COMPEG_FILTER_TRIANGLE ? 2u : kernel == COMPEG_FILTER_BICUBIC ? 4u : 6u;
}

// One launch.  `slots`: RegionAntialiasSlot records (region_body.h) whose tables are this file's.
struct FilterPack {
    const void *slots;
    const uint32_t *tables;
    uint8_t *dst;             // [slots][3][oh][ow], tight
    uint32_t ow, oh;
    uint32_t bands_per_slot;  // ceil(oh / R) + 1: the rectangle's first row begins a band wherever it lies
    uint32_t items_per_slot;  // lanes of a slot: bands_per_slot * ow
    uint32_t blocks_per_slot; // workgroups that hold them
    uint32_t bgr;             // plane c takes source channel 2 - c
    float scale[3], bias[3];  // per plane
    float pad[3];             // per source channel, on the pixel scale
};

// The pad value of source channel ch, as the contract has it: two rounded operations (region_body.h's region_pad).
CG_DEV float filter_pad(const FilterPack &t, uint32_t ch)
{
    // (constant indices: the launch's arguments stay in scalar registers)
    const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
    const float scaled = t.pad[ch] * scale;
    return scaled + bias;
}

// h(j) of one source row for one output column: the contract's x walk over `count` taps from `p` on, the weights
// `stride` words apart from `w` on.  k = 1: four taps at a time while four are left, their loads in flight together,
// the sums in order (antialias_body.h).
template <uint32_t K>
CG_DEV void filter_row(float (&h)[3], const uint8_t *p, uint32_t pitch, uint32_t count, const uint32_t *w, uint32_t stride)
{
    uint32_t tx = 0;
    for (; K == 1u && tx + 4u <= count; tx += 4u) {
        uint32_t rb[4], ga[4];
        float wt[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            wt[u] = antialias_weight(w + size_t(tx + u) * stride);
            resize_block<K>(p + size_t(tx + u) * K * 4u, pitch, rb[u], ga[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++)
            antialias_tap<K>(h, rb[u], ga[u], wt[u], tx + u == 0u);
    }
    for (; tx < count; tx++) {
        const float wt = antialias_weight(w + size_t(tx) * stride);
        uint32_t rb, ga;
        resize_block<K>(p + size_t(tx) * K * 4u, pitch, rb, ga);
        antialias_tap<K>(h, rb, ga, wt, tx == 0u);
    }
}

// Lane `item` of slot `slot`: band item / ow, column item % ow.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void filter_tensor_lane(const FilterPack &t, uint32_t slot, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    if (item >= t.items_per_slot)
        return;
    // (the slot is the workgroup's: these are wave-uniform loads)
    const RegionAntialiasSlot rs = region_slot<RegionAntialiasSlot>(t.slots, slot);
    const AntialiasImage &im = rs.im;
    const uint32_t band = item / t.ow, x = item - band * t.ow;
    const uint32_t dx = rs.dx, dy = rs.dy, dw = rs.dw, dh = rs.dh;
    // Band `lead` begins at the rectangle's first row; band 0 begins `shift` rows above the slot.
    const uint32_t shift = (R - dy % R) % R, lead = (dy + shift) / R;
    const uint32_t yi0 = band >= lead ? (band - lead) * R : dh; // the band's first row, counted in the rectangle
    const bool inside = x >= dx && x - dx < dw && yi0 < dh;
    const uint32_t rows = !inside ? 0u : (dh - yi0 < R ? dh - yi0 : R); // band rows 0 .. rows - 1 are the rectangle's

    float m[R][3]; // by source channel
#pragma unroll
    for (uint32_t r = 0; r < R; r++)
        m[r][0] = m[r][1] = m[r][2] = 0.0f;
    if (rows != 0u) {
        const uint32_t xi = x - dx;
        // (axis tables: first[o], count[o], then a row of o weights per t)
        const uint32_t *xtab = t.tables + im.xtab, *ytab = t.tables + im.ytab;
        const uint32_t xfirst = antialias_word(xtab + xi), xcount = antialias_word(xtab + dw + xi);
        const uint32_t *wx = xtab + 2u * size_t(dw) + xi, *wy = ytab + 2u * size_t(dh) + yi0;
        uint32_t from[R], to[R]; // band row r taps source rows from[r] .. to[r] - 1 (not the rectangle's: none)
        uint32_t jend = 0u;
#pragma unroll
        for (uint32_t r = 0; r < R; r++) {
            from[r] = to[r] = 0u;
            if (r < rows) {
                from[r] = antialias_word(ytab + yi0 + r);
                to[r] = from[r] + antialias_word(ytab + dh + yi0 + r);
            }
            jend = to[r] > jend ? to[r] : jend;
        }
        const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + (size_t(im.cx) + size_t(xfirst) * K) * 4u;
        for (uint32_t j = from[0]; j < jend; j++) {
            float h[3] = {0.0f, 0.0f, 0.0f};
            filter_row<K>(h, origin + size_t(j) * K * im.pitch, im.pitch, xcount, wx, dw);
#pragma unroll
            for (uint32_t r = 0; r < R; r++) {
                if (j >= from[r] && j < to[r]) {
                    const float w = antialias_weight(wy + size_t(j - from[r]) * dh + r);
#pragma unroll
                    for (uint32_t ch = 0; ch < 3u; ch++) {
                        const float q = h[ch] * w;
                        const float sum = m[r][ch] + q;
                        m[r][ch] = j == from[r] ? q : sum;
                    }
                }
            }
        }
    }

    const float pad[3] = {filter_pad(t, 0u), filter_pad(t, 1u), filter_pad(t, 2u)};
    const size_t plane = size_t(t.oh) * t.ow;
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
        const uint32_t y = band * R + r - shift; // (above the slot: wraps, and is no row of it)
        if (y >= t.oh)
            continue;
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            const uint32_t c = t.bgr ? 2u - ch : ch;
            // (constant indices: the launch's arguments stay in scalar registers)
            const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
            const float scaled = m[r][ch] * scale;
            const float filtered = scaled + bias;
            const float val = r < rows ? filtered : pad[ch];
            uint8_t *p = t.dst + ((size_t(slot) * 3u + c) * plane + size_t(y) * t.ow + x) * kElem;
            tensor_store_run(p, TensorVec{{tensor_bits<DTYPE>(val), 0u, 0u, 0u}}, kElem);
        }
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_slot workgroups for every slot, one slot behind the
// other.
template <uint32_t DTYPE, uint32_t K, uint32_t R>
CG_DEV void filter_tensor_block_lane(const FilterPack &t, uint32_t block, uint32_t lane)
{
    const uint32_t slot = block / t.blocks_per_slot;
    filter_tensor_lane<DTYPE, K, R>(t, slot, (block - slot * t.blocks_per_slot) * kTensorThreads + lane);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

// Whether a kernel takes an axis of n prefiltered samples and o outputs: n * 2S <= 128 * o.
inline bool filter_taps_ok(uint32_t kernel, uint32_t n, uint32_t o)
{
    return uint64_t(n) * filter_twice_support(kernel) <= uint64_t(kFilterMaxTaps) * o;
}

// f(z) of the contract, in double, every operation on its own.
inline double filter_kernel_value(uint32_t kernel, double z)
{
    switch (kernel) {
    case COMPEG_FILTER_BOX:
        return z > -0.5 && z <= 0.5 ? 1.0 : 0.0;
    case COMPEG_FILTER_TRIANGLE: {
        const double v = 1.0 - (z < 0.0 ? -z : z);
        return v > 0.0 ? v : 0.0;
    }
    case COMPEG_FILTER_BICUBIC: {
        const double a = -0.5, q = z < 0.0 ? -z : z;
        if (q < 1.0) {
            const double p = (a + 2.0) * q - (a + 3.0);
            const double pq = p * q;
            return pq * q + 1.0;
        }
        if (q < 2.0) {
            const double p = (q - 5.0) * q + 8.0;
            const double pq = p * q - 4.0;
            return pq * a;
        }
        return 0.0;
    }
    default: {
        if (!(z >= -3.0 && z < 3.0))
            return 0.0;
        const double pi = 3.141592653589793;
        const auto sinc = [pi](double v) {
            if (v == 0.0)
                return 1.0;
            const double pv = pi * v;
            return std::sin(pv) / pv;
        };
        const double third = z / 3.0;
        return sinc(z) * sinc(third);
    }
    }
}

// The axis tables of one launch in antialias_body.h's layout, each distinct (n, o) once; every table of a launch is the
// same kernel's.  `words` may begin with `front` words that are not tables (the launch's records).
struct FilterTables {
    struct Axis {
        uint32_t n, o, at;
    };
    std::vector<Axis> axes;
    std::vector<uint32_t> words;
    size_t front = 0;
    uint32_t kernel;

    explicit FilterTables(uint32_t kernel_, size_t front_words = 0) : words(front_words, 0u), front(front_words), kernel(kernel_) {}

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
        const double s = double(n) / double(o), sc = s > 1.0 ? s : 1.0;
        const double sup = (double(filter_twice_support(kernel)) / 2.0) * sc, inv = 1.0 / sc;
        std::vector<uint32_t> first(o), count(o);
        uint32_t taps = 1;
        for (uint32_t x = 0; x < o; x++) {
            const double c = s * (double(x) + 0.5);
            const int64_t a = int64_t(c - sup + 0.5), b = int64_t(c + sup + 0.5);
            const int64_t lo = a > 0 ? a : 0, hi = b < int64_t(n) ? b : int64_t(n);
            first[x] = uint32_t(lo);
            count[x] = uint32_t(hi - lo);
            taps = count[x] > taps ? count[x] : taps;
        }
        const uint64_t total_words = uint64_t(begin) + (uint64_t(taps) + 2u) * o;
        if (total_words > 0xffffffffull)
            return false;
        words.resize(front + size_t(total_words), 0u); // (a weight past an output's own count: 0, never read)
        uint32_t *tab = words.data() + front + begin;
        std::vector<double> u(taps);
        for (uint32_t x = 0; x < o; x++) {
            const double c = s * (double(x) + 0.5);
            double total = 0.0;
            for (uint32_t t = 0; t < count[x]; t++) {
                u[t] = filter_kernel_value(kernel, (double(int64_t(t) + int64_t(first[x])) - c + 0.5) * inv);
                total = t == 0u ? u[t] : total + u[t];
            }
            tab[x] = first[x];
            tab[size_t(o) + x] = count[x];
            for (uint32_t t = 0; t < count[x]; t++) {
                const float w = float(u[t] / total);
                memcpy(&tab[(2u + size_t(t)) * o + x], &w, 4);
            }
        }
        axes.push_back(Axis{n, o, uint32_t(begin)});
        at = uint32_t(begin);
        return true;
    }
};

// The records of a launch and behind them its axis tables: `blob` is the one block that travels, the tables begin
// tables_at bytes into it.  The inner rectangles lie inside ow x oh and have no side of 0 (the caller's to check, like
// the crops' lying inside their images).  False: a crop is smaller than the downscale factor k, an axis is beyond the
// tap limit, or the tables outgrow 32 bits.
inline bool plan_filter_slots(std::vector<uint32_t> &blob, size_t &tables_at, size_t &axes, const RegionSource *sources, uint32_t slots,
                              uint32_t k, uint32_t kernel)
{
    if (kernel >= kFilterKernels || k == 0u)
        return false;
    FilterTables tables(kernel, size_t(slots) * kRegionSlotWords);
    for (uint32_t i = 0; i < slots; i++) {
        const RegionSource &s = sources[i];
        if (s.dst.width == 0u || s.dst.height == 0u || s.dst.width > 65535u || s.dst.height > 65535u || s.dst.x > 65535u || s.dst.y > 65535u ||
            s.crop.width < k || s.crop.height < k)
            return false;
        RegionAntialiasSlot r{};
        r.im.src = static_cast<const uint8_t *>(s.src);
        r.im.pitch = s.pitch;
        r.im.cx = s.crop.x;
        r.im.cy = s.crop.y;
        r.im.pw = s.crop.width / k;
        r.im.ph = s.crop.height / k;
        if (!filter_taps_ok(kernel, r.im.pw, s.dst.width) || !filter_taps_ok(kernel, r.im.ph, s.dst.height) ||
            !tables.axis(r.im.pw, s.dst.width, r.im.xtab) || !tables.axis(r.im.ph, s.dst.height, r.im.ytab))
            return false;
        r.dx = uint16_t(s.dst.x);
        r.dy = uint16_t(s.dst.y);
        r.dw = uint16_t(s.dst.width);
        r.dh = uint16_t(s.dst.height);
        memcpy(tables.words.data() + i * kRegionSlotWords, &r, sizeof r); // (after the tables grew)
    }
    tables_at = size_t(slots) * sizeof(RegionAntialiasSlot);
    axes = tables.axes.size();
    blob.swap(tables.words);
    return true;
}

// The launch of one pack with bands of `band` rows: fills t, all but the records' and the tables' addresses, and says
// how many workgroups the grid's one dimension has.  pad: three values by source channel, or null for zeros.  False: the
// specs are not ones the kernels take, or the grid would not fit.
inline bool plan_filter_pack(FilterPack &t, uint32_t &grid_blocks, uint32_t slots, const compeg_tensor_spec &spec,
                             const compeg_filter_spec &filter, const float *pad, void *dst, uint32_t band)
{
    const uint32_t k = spec.downscale;
    if (spec.dtype > COMPEG_TENSOR_F32 || (k != 1u && k != 2u && k != 4u && k != 8u) || filter.kernel >= kFilterKernels ||
        filter.out_width == 0u || filter.out_height == 0u || filter.out_width > 65535u || filter.out_height > 65535u || slots == 0u || band == 0u)
        return false;
    t = FilterPack{};
    t.dst = static_cast<uint8_t *>(dst);
    t.ow = filter.out_width;
    t.oh = filter.out_height;
    t.bands_per_slot = (t.oh + band - 1u) / band + 1u;
    // (65537 bands of 65535 columns at the most: a slot's lanes, the last workgroup's beyond it included, fit 32 bits;
    // the grid's workgroups must fit 31)
    const uint64_t items = uint64_t(t.bands_per_slot) * t.ow;
    const uint64_t blocks = (items + kTensorThreads - 1u) / kTensorThreads;
    if (items > 0xffffffffull - kTensorThreads || blocks * slots > 0x7fffffffull)
        return false;
    t.items_per_slot = uint32_t(items);
    t.blocks_per_slot = uint32_t(blocks);
    t.bgr = spec.order == COMPEG_TENSOR_BGR ? 1u : 0u;
    for (int c = 0; c < 3; c++) {
        t.scale[c] = spec.scale[c];
        t.bias[c] = spec.bias[c];
        t.pad[c] = pad ? pad[c] : 0.0f;
    }
    grid_blocks = uint32_t(blocks * slots);
    return true;
}

} // namespace compeg
