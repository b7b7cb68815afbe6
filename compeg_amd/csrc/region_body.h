// Per-lane bodies of the region_tensor_* kernels (region_kernels.hip): the resized tensor output of resize_body.h and
// antialias_body.h, placed (include/compeg_hip.h, "Region tensor output").  A launch has `slots` output slots of
// ow x oh; a slot's record names the image and the crop it reads and the inner rectangle (dx, dy, dw, dh) of the slot
// that the resized crop fills.  Everything else of the slot is a pad value.
//
// Written like resize_body.h and antialias_body.h, whose taps, block sums, tables, conversions and stores it calls: what
// one lane executes, GPU-only instructions behind __HIP_DEVICE_COMPILE__, so that tests/emul_region compiles the very
// same code with g++ under ASan/UBSan and drives it lane by lane.  No lane talks to another one and there is no LDS.
//
// Arithmetic contract.  Inside the inner rectangle, element (c, y, x) is element (c, y - dy, x - dx)
// of resize_body.h's (nearest, bilinear) or antialias_body.h's contract with (ow, oh) := (dw, dh), operation for
// operation.  Outside it, v = (pad[ch] * scale[c]) + bias[c], ch the source channel of plane c: two rounded operations
// (compile with -ffp-contract=off), made by the lane itself so that they are the very operations of its other elements;
// converted and stored like them.
//
// Shape, nearest and bilinear: resize_body.h's -- a lane is one 16-byte run of an output row of a slot, for the three
// planes.  The run's elements fall into three stretches: pad behind the inner rectangle, filtered, pad in front of it;
// the lane walks them last element first, one loop each, so the filtered loop is resize_body.h's and what diverges is
// three trip counts, in the runs that hold a border only.  A row outside dy .. dy + dh has no filtered stretch: no
// source load.  Antialiased: antialias_body.h's -- a lane is one output element; an outside one stores the pad and
// loads nothing, no table word either.  An axis' table is as wide as the inner extent (dw or dh), not the slot's.
#pragma once

#include "antialias_body.h"
#include "region_types.h"

namespace compeg {

// One slot of a launch (device memory; built by the host per call): the 40-byte record of the filter plus the inner
// rectangle, whose extents fit 16 bits each (an output extent is 65535 at the most).
struct alignas(8) RegionSlot {
    ResizeImage im; // rx, ry: against (dw, dh)
    uint16_t dx, dy, dw, dh;
};
static_assert(sizeof(RegionSlot) == 48, "the host writes these records as the kernels read them");

struct alignas(8) RegionAntialiasSlot {
    AntialiasImage im; // xtab, ytab: tables of (pw, dw) and (ph, dh)
    uint16_t dx, dy, dw, dh;
};
static_assert(sizeof(RegionAntialiasSlot) == sizeof(RegionSlot), "one record size for all three filters");

// One launch.  `slots` is RegionSlot records (nearest, bilinear) or RegionAntialiasSlot ones (antialiased; then
// `tables` are the launch's axis tables).
struct RegionPack {
    const void *slots;
    const uint32_t *tables;
    uint8_t *dst;              // [slots][3][oh][ow], tight
    uint32_t ow, oh;
    uint32_t runs_per_row;     // nearest, bilinear: ceil(ow / elements of a 16-byte run)
    uint32_t items_per_slot;   // lanes of a slot: oh * runs_per_row, antialiased oh * ow
    uint32_t blocks_per_slot;  // workgroups that hold them
    uint32_t bgr;              // plane c takes source channel 2 - c
    float scale[3], bias[3];   // per plane
    float pad[3];              // per source channel, on the pixel scale
};

// The record of the workgroup's slot: wave-uniform loads.
template <typename Slot>
CG_DEV Slot region_slot(const void *slots, uint32_t slot)
{
    const Slot *p = static_cast<const Slot *>(slots) + slot;
    Slot s;
#if defined(__HIP_DEVICE_COMPILE__)
    const auto *q = CG_GLOBAL(const uint64_t, reinterpret_cast<const uint64_t *>(p));
    const uint64_t w[6] = {q[0], q[1], q[2], q[3], q[4], q[5]};
    __builtin_memcpy(&s, w, sizeof s);
#else
    memcpy(&s, p, sizeof s);
#endif
    return s;
}

// The pad value of source channel ch, as the contract has it: two rounded operations.
CG_DEV float region_pad(const RegionPack &t, uint32_t ch)
{
    // (constant indices: the launch's arguments stay in scalar registers)
    const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
    const float scaled = t.pad[ch] * scale;
    return scaled + bias;
}

// Lane `item` of slot `slot`: row item / runs_per_row, run item % runs_per_row.
template <uint32_t DTYPE, uint32_t K, uint32_t FILTER>
CG_DEV void region_tensor_lane(const RegionPack &t, uint32_t slot, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    constexpr uint32_t kRun = 16u / kElem; // output elements of a lane, per plane
    constexpr float kInv = 1.0f / float(K * K);
    if (item >= t.items_per_slot)
        return;
    // (the slot is the workgroup's: these are wave-uniform loads)
    const RegionSlot rs = region_slot<RegionSlot>(t.slots, slot);
    const ResizeImage &im = rs.im;
    const uint32_t y = item / t.runs_per_row, run = item - y * t.runs_per_row;
    const uint32_t x0 = run * kRun;
    const uint32_t count = t.ow - x0 < kRun ? t.ow - x0 : kRun; // elements of this run inside the row

    // The run's elements lo .. hi - 1 lie inside the inner rectangle (none: lo = hi = 0).
    const uint32_t dx = rs.dx, dy = rs.dy, dx1 = dx + uint32_t(rs.dw);
    const bool row_inside = y >= dy && y - dy < uint32_t(rs.dh);
    const uint32_t first = dx > x0 ? dx - x0 : 0u, last = dx1 > x0 ? dx1 - x0 : 0u;
    const uint32_t hi = !row_inside ? 0u : (last < count ? last : count);
    const uint32_t lo = first < hi ? first : hi;

    const uint32_t padbits[3] = {tensor_bits<DTYPE>(region_pad(t, 0u)), tensor_bits<DTYPE>(region_pad(t, 1u)),
                                 tensor_bits<DTYPE>(region_pad(t, 2u))};
    TensorVec out[3] = {{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}}; // by source channel
    for (uint32_t j = count; j-- > hi;) {
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++)
            resize_push<kElem>(out[ch], padbits[ch]);
    }

    // resize_body.h's loop, its coordinates relative to the inner rectangle
    const ResizeTaps ty = resize_taps<FILTER>(row_inside ? y - dy : 0u, im.ry, im.ph);
    const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + size_t(im.cx) * 4u;
    const uint8_t *row0 = origin + size_t(ty.i0) * K * im.pitch, *row1 = origin + size_t(ty.i1) * K * im.pitch;
    for (uint32_t j = hi; j-- > lo;) {
        const ResizeTaps tx = resize_taps<FILTER>(x0 + j - dx, im.rx, im.pw);
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

    for (uint32_t j = lo; j-- > 0u;) {
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++)
            resize_push<kElem>(out[ch], padbits[ch]);
    }

    const size_t plane = size_t(t.oh) * t.ow;
    const size_t at = size_t(y) * t.ow + x0;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const uint32_t c = t.bgr ? 2u - ch : ch;
        uint8_t *p = t.dst + ((size_t(slot) * 3u + c) * plane + at) * kElem;
        tensor_store_run(p, out[ch], count * kElem);
    }
}

// Antialiased: lane `item` of slot `slot` is row item / ow, column item % ow.
template <uint32_t DTYPE, uint32_t K>
CG_DEV void region_antialias_lane(const RegionPack &t, uint32_t slot, uint32_t item)
{
    constexpr uint32_t kElem = tensor_elem_bytes(DTYPE);
    if (item >= t.items_per_slot)
        return;
    // (the slot is the workgroup's: these are wave-uniform loads)
    const RegionAntialiasSlot rs = region_slot<RegionAntialiasSlot>(t.slots, slot);
    const AntialiasImage &im = rs.im;
    const uint32_t y = item / t.ow, x = item - y * t.ow;
    const uint32_t dx = rs.dx, dy = rs.dy, dw = rs.dw, dh = rs.dh;
    const bool inside = x >= dx && x - dx < dw && y >= dy && y - dy < dh;

    float val[3]; // by source channel
    if (!inside) {
        val[0] = region_pad(t, 0u);
        val[1] = region_pad(t, 1u);
        val[2] = region_pad(t, 2u);
    } else {
        // antialias_body.h's lane at (x - dx, y - dy) of a dw x dh output
        const uint32_t xi = x - dx, yi = y - dy;
        // (axis tables: first[o], count[o], then a row of o weights per t)
        const uint32_t *xtab = t.tables + im.xtab, *ytab = t.tables + im.ytab;
        const uint32_t xfirst = antialias_word(xtab + xi), xcount = antialias_word(xtab + dw + xi);
        const uint32_t yfirst = antialias_word(ytab + yi), ycount = antialias_word(ytab + dh + yi);
        const uint32_t *wx = xtab + 2u * size_t(dw) + xi, *wy = ytab + 2u * size_t(dh) + yi;
        const uint8_t *origin = im.src + size_t(im.cy) * im.pitch + size_t(im.cx) * 4u;

        float m[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t ty = 0; ty < ycount; ty++) {
            const uint32_t j = yfirst + ty < im.ph - 1u ? yfirst + ty : im.ph - 1u;
            const uint8_t *row = origin + size_t(j) * K * im.pitch;
            float h[3] = {0.0f, 0.0f, 0.0f};
            uint32_t tx = 0;
            // (k = 1: four taps' loads in flight together, the sums in order -- antialias_body.h)
            for (; K == 1u && tx + 4u <= xcount; tx += 4u) {
                uint32_t rb[4], ga[4];
                float w[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++) {
                    const uint32_t i = xfirst + tx + u < im.pw - 1u ? xfirst + tx + u : im.pw - 1u;
                    w[u] = antialias_weight(wx + size_t(tx + u) * dw);
                    resize_block<K>(row + size_t(i) * K * 4u, im.pitch, rb[u], ga[u]);
                }
#pragma unroll
                for (uint32_t u = 0; u < 4u; u++)
                    antialias_tap<K>(h, rb[u], ga[u], w[u], tx + u == 0u);
            }
            for (; tx < xcount; tx++) {
                const uint32_t i = xfirst + tx < im.pw - 1u ? xfirst + tx : im.pw - 1u;
                const float w = antialias_weight(wx + size_t(tx) * dw);
                uint32_t rb, ga;
                resize_block<K>(row + size_t(i) * K * 4u, im.pitch, rb, ga);
                antialias_tap<K>(h, rb, ga, w, tx == 0u);
            }
            const float w = antialias_weight(wy + size_t(ty) * dh);
#pragma unroll
            for (uint32_t ch = 0; ch < 3u; ch++) {
                const float q = h[ch] * w;
                const float sum = m[ch] + q;
                m[ch] = ty == 0u ? q : sum;
            }
        }
#pragma unroll
        for (uint32_t ch = 0; ch < 3u; ch++) {
            const float scale = t.bgr ? t.scale[2u - ch] : t.scale[ch], bias = t.bgr ? t.bias[2u - ch] : t.bias[ch];
            const float scaled = m[ch] * scale;
            val[ch] = scaled + bias;
        }
    }

    const size_t plane = size_t(t.oh) * t.ow;
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ch++) {
        const uint32_t c = t.bgr ? 2u - ch : ch;
        uint8_t *p = t.dst + ((size_t(slot) * 3u + c) * plane + item) * kElem;
        tensor_store_run(p, TensorVec{{tensor_bits<DTYPE>(val[ch]), 0u, 0u, 0u}}, kElem);
    }
}

// Lane `lane` of workgroup `block` of the flat grid: blocks_per_slot workgroups for every slot, one slot behind the
// other.  FILTER: COMPEG_RESIZE_NEAREST, COMPEG_RESIZE_BILINEAR, or the latter with COMPEG_RESIZE_ANTIALIAS.
template <uint32_t DTYPE, uint32_t K, uint32_t FILTER>
CG_DEV void region_tensor_block_lane(const RegionPack &t, uint32_t block, uint32_t lane)
{
    const uint32_t slot = block / t.blocks_per_slot;
    const uint32_t item = (block - slot * t.blocks_per_slot) * kTensorThreads + lane;
    if constexpr ((FILTER & COMPEG_RESIZE_ANTIALIAS) != 0u)
        region_antialias_lane<DTYPE, K>(t, slot, item);
    else
        region_tensor_lane<DTYPE, K, FILTER>(t, slot, item);
}

// ---- host side (the library and the emulator plan with it) ---------------------------------------------------------

constexpr size_t kRegionSlotWords = sizeof(RegionSlot) / 4u;

// The records of a launch, and behind them, antialiased, its axis tables: `blob` is the one block that travels, the
// tables begin tables_at bytes into it.  The inner rectangles lie inside ow x oh and have no side of 0 (the caller's to
// check, like the crops' lying inside their images).  False: a crop is smaller than the downscale factor k, an axis
// shrinks by more than the antialias flag takes, or the tables outgrow 32 bits.
inline bool plan_region_slots(std::vector<uint32_t> &blob, size_t &tables_at, size_t &axes, const RegionSource *sources, uint32_t slots,
                              uint32_t k, uint32_t filter)
{
    const bool antialias = (filter & COMPEG_RESIZE_ANTIALIAS) != 0u;
    AntialiasTables tables(size_t(slots) * kRegionSlotWords);
    for (uint32_t i = 0; i < slots; i++) {
        const RegionSource &s = sources[i];
        if (s.dst.width == 0u || s.dst.height == 0u || s.dst.width > 65535u || s.dst.height > 65535u || s.dst.x > 65535u || s.dst.y > 65535u)
            return false;
        const uint16_t rect[4] = {uint16_t(s.dst.x), uint16_t(s.dst.y), uint16_t(s.dst.width), uint16_t(s.dst.height)};
        uint32_t *at = nullptr;
        if (antialias) {
            RegionAntialiasSlot r{};
            if (!plan_antialias_image(r.im, tables, s.src, s.pitch, s.crop, k, s.dst.width, s.dst.height))
                return false;
            memcpy(&r.dx, rect, sizeof rect);
            at = tables.words.data() + i * kRegionSlotWords; // (after the tables grew)
            memcpy(at, &r, sizeof r);
        } else {
            RegionSlot r{};
            if (!plan_resize_image(r.im, s.src, s.pitch, s.crop, k, s.dst.width, s.dst.height))
                return false;
            memcpy(&r.dx, rect, sizeof rect);
            at = tables.words.data() + i * kRegionSlotWords;
            memcpy(at, &r, sizeof r);
        }
    }
    tables_at = size_t(slots) * sizeof(RegionSlot);
    axes = tables.axes.size();
    blob.swap(tables.words);
    return true;
}

// The launch of one pack: fills t, all but the records' and the tables' addresses, and says how many workgroups the
// grid's one dimension has.  pad: three values by source channel, or null for zeros.  False: the specs are not ones the
// kernels take, or the grid would not fit -- plan_resize_pack's and plan_antialias_pack's limits, `slots` for images.
inline bool plan_region_pack(RegionPack &t, uint32_t &grid_blocks, uint32_t slots, const compeg_tensor_spec &spec,
                             const compeg_resize_spec &resize, const float *pad, void *dst)
{
    t = RegionPack{};
    if (resize.filter & COMPEG_RESIZE_ANTIALIAS) {
        AntialiasPack a;
        if (!plan_antialias_pack(a, grid_blocks, slots, spec, resize, dst))
            return false;
        t.items_per_slot = a.items_per_image;
        t.blocks_per_slot = a.blocks_per_image;
    } else {
        ResizePack r;
        if (!plan_resize_pack(r, grid_blocks, slots, spec, resize, dst))
            return false;
        t.runs_per_row = r.runs_per_row;
        t.items_per_slot = r.items_per_image;
        t.blocks_per_slot = r.blocks_per_image;
    }
    t.dst = static_cast<uint8_t *>(dst);
    t.ow = resize.out_width;
    t.oh = resize.out_height;
    t.bgr = spec.order == COMPEG_TENSOR_BGR ? 1u : 0u;
    for (int c = 0; c < 3; c++) {
        t.scale[c] = spec.scale[c];
        t.bias[c] = spec.bias[c];
        t.pad[c] = pad ? pad[c] : 0.0f;
    }
    return true;
}

} // namespace compeg
