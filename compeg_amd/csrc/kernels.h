// Host-callable launchers of the gfx950 kernels (kernels.hip).
#pragma once

#include <vector>

#include <hip/hip_runtime_api.h>

#include "compeg_hip.h"
#include "crop_regions_types.h"
#include "crop_types.h"
#include "device_types.h"
#include "levels_types.h"
#include "planes_types.h"
#include "reduced_types.h"
#include "region_types.h"
#include "scaled_types.h"

namespace compeg {

// The compute units and the LDS per compute unit of the device the calling thread has current, asked once per device
// (kernels.hip): what the planners size workgroups and grids for and the launches raise their kernels' LDS limit to.
struct DeviceLimits {
    uint32_t cus, lds_bytes;
};
DeviceLimits device_limits();

// Chooses workgroup shape and LDS carve-up for a decode of `images` images
// whose largest image has `max_intervals` restart intervals and `max_l2`
// L2 entries; max_wave_words (largest scan span of 64 consecutive intervals)
// sizes the per-wave scan window.
// wave_cap: at most that many waves per workgroup (0: the kernel family's own limit)
// slot_bytes: a lane's data-unit slot (the levels kernels keep 64 positions: kLevelsSlotBytes)
HuffLdsPlan plan_huffman(uint32_t max_intervals, uint32_t images, uint32_t max_l2,
                         uint32_t max_wave_words, bool fused, uint32_t wave_cap = 0, uint32_t slot_bytes = kDuSlotBytes);
// Largest word span covered by any group of 64 consecutive restart intervals.
uint32_t max_wave_span(const uint32_t *starts, size_t nstarts, size_t nwords, uint32_t intervals,
                       uint32_t group = kWave);

// descs: device array of `images` descriptors.  Grid = (blocks for the
// largest image, images); blocks past an image's own extent exit at once.
hipError_t launch_huffman(const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                          const HuffLdsPlan &plan, hipStream_t stream);
// Same outputs as launch_huffman (coefficient records + DC terms) from the fast-mode decoder.
hipError_t launch_entropy(const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                          const HuffLdsPlan &plan, hipStream_t stream);
// uniform: all images have max_intervals intervals and byte-identical LUTs (workgroups may then span images)
// one_mcu_intervals: every image's restart interval is one MCU (the kernel whose rows leave wave-wide)
// from_records: descs are the images' descriptors of MCUs (ImageDesc::mcu_word), max_intervals the most MCUs of any
// queue: four bytes of device memory of the caller's (or null): the counter the resident waves of a uniform launch
// draw their units from (zeroed here, in stream order)
hipError_t launch_fused_422(const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                            const HuffLdsPlan &plan, hipStream_t stream, bool uniform = false, bool one_mcu_intervals = false,
                            uint32_t *queue = nullptr, bool from_records = false);
// The batch kernel with the window in its streamed form (kernels_body.h: decode_wave_fused_422_stream), for launches
// whose whole-interval windows would leave a CU fewer than its twelve waves.
struct StreamPlan {
    uint32_t rows = 0, waves_per_block = 0, l2_entries_in_lds = 0, total_bytes = 0;
    uint32_t waves_per_image = 0; // != 0: the flat grid (uniform launches)
    uint32_t stage_after = 8;     // bit k: rows may be staged anew behind data unit k of an MCU ...
    uint32_t stage_below = 0;     // ... and are, when some lane has fewer staged words than this in front of it
    uint32_t cu_waves = 12;       // waves of the kernel a CU holds
};
// uniform: all images have max_intervals intervals and byte-identical LUTs (workgroups may then span images)
// cu_waves / group_waves: 0 (4:2:2: twelve waves a CU, in one workgroup), or what the layout's kernel holds
StreamPlan plan_stream(uint32_t max_intervals, uint32_t images, uint32_t max_l2, uint32_t mcu_words, bool uniform, uint32_t cu_waves = 0,
                       uint32_t group_waves = 0);
// (plan: plan_huffman's for the same launch)
bool stream_plan_preferred(const HuffLdsPlan &plan, uint32_t max_intervals, uint32_t images, uint32_t cu_waves = 0, uint32_t group_waves = 0);
// (hs, vs: the luma sampling all images of the launch share: 2x1, or an extension layout's -- paired kernels for 1x1 / 1x2)
hipError_t launch_fused_stream(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const StreamPlan &plan,
                                   hipStream_t stream, uint32_t hs = 2, uint32_t vs = 1, uint32_t *queue = nullptr);
// The first kernel of the walk + lane-per-MCU route (kernels_body.h): a lane per restart interval, entropy decode only,
// every MCU's record into ImageDesc::mcu_word / mcu_state; the second one is launch_fused_422(..., from_records) over the
// images' descriptors of MCUs.
// walk_tables: every image has ImageDesc::walk (launch_walk_tables): two symbols a step
struct WalkPlan {
    uint32_t rows = 0, stage_below = 0, waves_per_block = 0, l2_entries_in_lds = 0, total_bytes = 0;
    uint32_t chunk = 1;           // MCUs a lane walks between two looks at what it found (walk_body.h)
    uint32_t waves_per_image = 0; // != 0: the flat grid (uniform launches)
    bool walk_tables = false;
};
// restart_interval: the smallest of the launch's images
WalkPlan plan_walk(uint32_t max_intervals, uint32_t images, uint32_t max_l2, uint32_t mcu_words, uint32_t restart_interval, bool uniform, bool walk_tables);
hipError_t launch_walk_mcus(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const WalkPlan &plan, hipStream_t stream,
                            uint32_t *queue = nullptr);
// Extension layouts (luma hs x vs = 1x1, 1x2, 2x2), fused like the 4:2:2 kernel; plan with wave_cap = fused_layout_wave_cap.
// hs x vs = 1x0: grayscale images (one component, no chroma: 8-pixel MCUs of one data unit; gray_body.h).
// pairs: (8-pixel MCUs) every image of the launch has restart intervals of two MCUs or more -- a lane composites its MCUs two at a time (an odd interval's last alone)
uint32_t fused_layout_wave_cap(uint32_t hs, uint32_t vs, bool pairs);
hipError_t launch_fused_layout(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan,
                               uint32_t hs, uint32_t vs, bool pairs, hipStream_t stream);
// Latency variant: one decoder wave + one transformer wave per 64 intervals.
hipError_t launch_pair_422(const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                           const HuffLdsPlan &plan, hipStream_t stream);
// Cooperative kernel (coop_body.h) for launches too small to fill the chip with a lane per restart interval.
struct CoopPlan {
    bool usable;
    uint32_t group_waves; // 4, 2 or 1: a team takes coop_shape(restart_interval, group_waves).ipw whole intervals
    uint32_t intervals_per_wave, waves_per_block, window_words, l2_entries_in_lds, total_bytes, total_waves; // (intervals_per_wave: per team)
    uint32_t fit_teams; // teams a CU's LDS holds at once with this window (1..4)
    uint32_t places;    // ... and the chip: teams resident at once
};
// The kernel's teams of four waves take the whole restart intervals of 4 x 64 data units -- of 2 x 64 or 64 where
// those do not fit the largest window (dense streams: bit positions inside a window are 16-bit).
// words[k]: largest word span of any group of coop_shape(restart_interval, 4 >> k).ipw consecutive intervals
// (max_wave_span with that group size), or an upper estimate of it
struct CoopSpans {
    uint32_t words[3];
};
CoopPlan plan_coop(uint32_t max_intervals, uint32_t images, uint32_t restart_interval, uint32_t max_l2,
                   const CoopSpans &spans);
hipError_t launch_coop_422(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const CoopPlan &plan,
                           hipStream_t stream);
// Fills ImageDesc::walk (kWalkTableBytes each) of every image that has one, from its direct tables.
constexpr size_t kWalkTableBytes = 4u * 2048u * 4u;
hipError_t launch_walk_tables(const ImageDesc *descs, uint32_t images, hipStream_t stream);
hipError_t launch_idct_composite(const ImageDesc *descs, uint32_t images, uint32_t max_dus,
                                 hipStream_t stream);

// Extension pipeline for layouts other than 4:2:2: entropy decode + IDCT into sample records (plan as for
// the fused kernel), then the composite of every output the descriptors name (max_w x max_h: largest output).
hipError_t launch_entropy_samples(const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                                  const HuffLdsPlan &plan, hipStream_t stream);
hipError_t launch_generic_composite(const ImageDesc *descs, uint32_t images, uint32_t max_w, uint32_t max_h,
                                    hipStream_t stream);

// Tensor output (tensor_kernels.hip, tensor_body.h): packs the WxH corner of `images` RGBA8 outputs, src_image_stride
// bytes apart with rows of src_pitch bytes, into [images][3][H / k][W / k] at dst, tight.  spec: validated by the caller.
hipError_t launch_pack_tensor(const void *src, size_t src_image_stride, uint32_t src_pitch, uint32_t width, uint32_t height,
                              uint32_t images, const compeg_tensor_spec &spec, void *dst, hipStream_t stream);

// Resized tensor output (resize_kernels.hip, resize_body.h): `images` records (device memory, resize_body.h: ResizeImage)
// into [images][3][oh][ow] at dst, tight.  Both specs: validated by the caller.
constexpr size_t kResizeRecordBytes = 40;
// ... and one image's record, written at `record` (kResizeRecordBytes bytes, 8-byte aligned): the crop of the image at
// src, rows pitch bytes apart, for downscale factor k and an ow x oh output.  False: the crop is smaller than k.
bool make_resize_record(void *record, const void *src, uint32_t pitch, const compeg_rect &crop, uint32_t k, uint32_t ow, uint32_t oh);
hipError_t launch_resize_tensor(const void *device_records, uint32_t images, const compeg_tensor_spec &spec,
                                const compeg_resize_spec &resize, void *dst, hipStream_t stream);

// Antialiased bilinear (resize_kernels.hip, antialias_body.h): the launch's records and axis tables travel as one blob,
// `images` records of kResizeRecordBytes first, the tables (each distinct axis once) behind them from tables_at on.
struct AntialiasSource {
    const void *src; // the image's first pixel, rows pitch bytes apart
    uint32_t pitch;
    compeg_rect crop;
};
// False: a crop is smaller than k or an axis shrinks by more than the flag takes (the caller has checked both), or the
// call's tables outgrow the 32 bits their offsets have (thousands of images of different sizes at the largest extents).
bool make_antialias_blob(std::vector<uint32_t> &blob, size_t &tables_at, const AntialiasSource *sources, uint32_t images, uint32_t k,
                         uint32_t ow, uint32_t oh);
hipError_t launch_resize_tensor_antialias(const void *device_blob, size_t tables_at, uint32_t images, const compeg_tensor_spec &spec,
                                          const compeg_resize_spec &resize, void *dst, hipStream_t stream);

// Region tensor output (region_kernels.hip, region_body.h): `slots` records of kRegionRecordBytes and, antialiased, the
// axis tables behind them from tables_at on, as one blob.  A slot's record says which crop of which image fills which
// rectangle of the slot (region_types.h: RegionSource); the rest of the slot is the pad value.
constexpr size_t kRegionRecordBytes = 48;
// filter: compeg_resize_spec's.  False: a crop is smaller than k or an axis shrinks by more than the antialias flag
// takes (the caller has checked both), or the call's tables outgrow the 32 bits their offsets have.
bool make_region_blob(std::vector<uint32_t> &blob, size_t &tables_at, const RegionSource *sources, uint32_t slots, uint32_t k,
                      uint32_t filter);
// Whether the launch's grid fits (the planners' limits of the resized packs, `slots` for images).
bool region_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_resize_spec &resize);
// pad: three values on the pixel scale by source channel (R, G, B), or null for zeros.
hipError_t launch_region_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_resize_spec &resize, const float *pad, void *dst, hipStream_t stream);

// Filtered tensor output (filter_kernels.hip, filter_body.h): the region pack's records with the axis tables of one of
// the four kernels (COMPEG_FILTER_*) behind them, as one blob; a lane is a column of a band of kFilterBand output rows.
#if defined(CG_FILTER_BAND)
constexpr uint32_t kFilterBand = CG_FILTER_BAND; // (a measurement build with another band: DESIGN.md 5.11, "Measured")
#else
constexpr uint32_t kFilterBand = 8;
#endif
// False: a crop is smaller than k or an axis is beyond the tap limit (the caller has checked both), or the call's tables
// outgrow the 32 bits their offsets have.
bool make_filter_blob(std::vector<uint32_t> &blob, size_t &tables_at, const RegionSource *sources, uint32_t slots, uint32_t k,
                      uint32_t kernel);
bool filter_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter);
// pad: three values on the pixel scale by source channel (R, G, B), or null for zeros.
hipError_t launch_filter_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_filter_spec &filter, const float *pad, void *dst, hipStream_t stream);

// Oriented tensor output (orient_kernels.hip, orient_body.h): the filtered pack's lane with an EXIF orientation per slot;
// `slots` records of kOrientRecordBytes and the axis tables behind them, as one blob.  ow x oh: the upright slot.
constexpr size_t kOrientRecordBytes = 56;
// False: what make_filter_blob refuses, an orientation outside 1..8 or a dst' outside T (the caller has checked them).
bool make_orient_blob(std::vector<uint32_t> &blob, size_t &tables_at, const OrientSource *sources, uint32_t slots, uint32_t k,
                      uint32_t kernel, uint32_t ow, uint32_t oh);
// upright / transposed: whether some slot has an orientation in 1..4 / in 5..8; a slot's lanes are the larger count.
bool orient_grid_fits(uint32_t slots, const compeg_tensor_spec &spec, const compeg_filter_spec &filter, bool upright, bool transposed);
// pad: three values on the pixel scale by source channel (R, G, B), or null for zeros.
hipError_t launch_orient_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                                const compeg_filter_spec &filter, bool upright, bool transposed, const float *pad, void *dst,
                                hipStream_t stream);

// Channels-last tensor output (nhwc_kernels.hip, nhwc_body.h): the oriented pack's blob (make_orient_blob) and grid
// (orient_grid_fits), its lane with a pixel's 3 or 4 channel values stored next to each other; dst: [slots][oh][ow][C].
hipError_t launch_nhwc_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                              const compeg_filter_spec &filter, const compeg_nhwc_spec &nhwc, bool upright, bool transposed, const float *pad,
                              void *dst, hipStream_t stream);

// Luma tensor output (luma_kernels.hip, luma_body.h): the oriented pack's blob (make_orient_blob) and grid
// (orient_grid_fits), one channel a slot, the weighted sum of R, G and B; dst: [slots][oh][ow]; pad: one value.
hipError_t launch_luma_tensor(const void *device_blob, size_t tables_at, uint32_t slots, const compeg_tensor_spec &spec,
                              const compeg_filter_spec &filter, const compeg_luma_spec &luma, bool upright, bool transposed, const float *pad,
                              void *dst, hipStream_t stream);

// Planes decode (planes_kernels.hip, planes_body.h): the images' samples, component by component at the component's own
// resolution, into the caller's memory as `target` lays it out; a lane per restart interval behind whole windows.
// hs x vs: the luma sampling all images of the launch share (1 x 0: grayscale images); plan: plan_huffman's with
// wave_cap = planes_wave_cap.  target: validated by the caller.
uint32_t planes_wave_cap(uint32_t hs, uint32_t vs);
hipError_t launch_planes(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const PlanesTarget &target, hipStream_t stream);

// Reduced decode (reduced_kernels.hip, reduced_body.h): the images at 1/8 scale, one RGB pixel per luma data unit from
// the DC terms alone, into the caller's memory as `target` lays it out; a lane per restart interval behind whole
// windows.  hs x vs as for launch_planes; plan: plan_huffman's with fused = false (the entropy walk's occupancy) and
// wave_cap = reduced_wave_cap.  target: validated by the caller.
uint32_t reduced_wave_cap();
hipError_t launch_reduced(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                          const ReducedTarget &target, hipStream_t stream);

// Cropped decode (crop_kernels.hip, crop_body.h): one rectangle of every image, pixel for pixel the RGBA decode's, into
// the caller's memory as `target` lays it out; a lane per restart interval behind whole windows, and no work for an
// interval, a wave or a workgroup without an MCU in the rectangle.  hs x vs as for launch_planes; plan: plan_huffman's
// with wave_cap = crop_wave_cap.  target: validated by the caller.
uint32_t crop_wave_cap(uint32_t hs, uint32_t vs);
hipError_t launch_cropped(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                          const CropTarget &target, hipStream_t stream);

// Cropped decode of a region list (crop_regions_kernels.hip, crop_regions_body.h): `regions` records from `records` on
// (device memory), all of images of one luma sampling -- group: crop_region_group's -- each a rectangle of the image
// descs[record.image] into the place its record's offset names; the cropped decode's prologue and lane body.
// max_intervals: the largest interval count among the images the records name; at most 65535 regions a launch; plan:
// plan_huffman's with wave_cap = crop_regions_wave_cap.  records and target: validated by the caller.
uint32_t crop_regions_wave_cap(uint32_t hs, uint32_t vs);
hipError_t launch_cropped_regions(const ImageDesc *descs, const CropRegionRecord *records, uint32_t regions, uint32_t max_intervals,
                                  const HuffLdsPlan &plan, uint32_t group, const CropRegionsTarget &target, hipStream_t stream);

// Scaled decode (scaled_kernels.hip, scaled_body.h): the images at 1/2 or 1/4 scale, target.n x target.n pixels per luma
// data unit from an n-point inverse DCT of each data unit's lowest frequencies, into the caller's memory as `target` lays
// it out; a lane per restart interval behind whole windows.  hs x vs as for launch_planes; plan: plan_huffman's with
// fused = false and wave_cap = scaled_wave_cap for the target's n.  target: validated by the caller.
uint32_t scaled_wave_cap(uint32_t hs, uint32_t vs, uint32_t n);
hipError_t launch_scaled(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const ScaledTarget &target, hipStream_t stream);

// A decode into the caller's memory, as the runtime's one road for them takes it (compeg_decoder::enqueue,
// compeg_batch::decode_into): how to plan it, how to launch it, what to record.  A further output of this shape is a
// further maker below, nothing in the runtime.
struct CallerDecode {
    const void *target; // the family's target (the maker's argument: it outlives the call), validated by the caller
    // images first .. first + images - 1 of the target, their descriptors from descs on
    hipError_t (*launch)(const void *target, uint32_t first, const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                         const HuffLdsPlan &plan, uint32_t hs, uint32_t vs, hipStream_t stream);
    bool fused;                                     // plan_huffman's flag ...
    uint32_t (*wave_cap)(uint32_t hs, uint32_t vs); // ... and its wave_cap
    int kernel_id;                                  // COMPEG_KERNEL_*
    uint32_t slot_bytes = kDuSlotBytes;             // ... and its slot_bytes
};
template <class Target, hipError_t (*Launch)(const ImageDesc *, uint32_t, uint32_t, const HuffLdsPlan &, uint32_t, uint32_t, const Target &, hipStream_t)>
hipError_t launch_caller_decode(const void *target, uint32_t first, const ImageDesc *descs, uint32_t images, uint32_t max_intervals,
                                const HuffLdsPlan &plan, uint32_t hs, uint32_t vs, hipStream_t stream)
{
    Target part = *static_cast<const Target *>(target);
    part.dst += uint64_t(first) * part.image_stride;
    return Launch(descs, images, max_intervals, plan, hs, vs, part, stream);
}
inline CallerDecode planes_decode(const PlanesTarget &target)
{
    return CallerDecode{&target, launch_caller_decode<PlanesTarget, launch_planes>, true, planes_wave_cap, COMPEG_KERNEL_PLANES};
}
// (fused = false: the entropy walk's occupancy)
inline CallerDecode reduced_decode(const ReducedTarget &target)
{
    return CallerDecode{&target, launch_caller_decode<ReducedTarget, launch_reduced>, false,
                        [](uint32_t, uint32_t) { return reduced_wave_cap(); }, COMPEG_KERNEL_REDUCED};
}
inline CallerDecode cropped_decode(const CropTarget &target)
{
    return CallerDecode{&target, launch_caller_decode<CropTarget, launch_cropped>, true, crop_wave_cap, COMPEG_KERNEL_CROPPED};
}

// (fused = false as for the reduced decode; the wave cap is the one of the target's transform size)
inline CallerDecode scaled_decode(const ScaledTarget &target)
{
    return CallerDecode{&target, launch_caller_decode<ScaledTarget, launch_scaled>, false,
                        target.n == 4u ? +[](uint32_t hs, uint32_t vs) { return scaled_wave_cap(hs, vs, 4u); }
                                       : +[](uint32_t hs, uint32_t vs) { return scaled_wave_cap(hs, vs, 2u); },
                        COMPEG_KERNEL_SCALED};
}

// Levels decode (levels_kernels.hip, levels_body.h): the images' quantised DCT coefficients as the entropy decode
// yields them, all 64 positions of every data unit as int16 blocks of 128 bytes, component after component, into the
// caller's memory as `target` lays it out; a lane per restart interval behind whole windows with slots of
// kLevelsSlotBytes.  hs x vs as for launch_planes; plan: plan_huffman's with fused = false, wave_cap = levels_wave_cap
// and slot_bytes = kLevelsSlotBytes.  target: validated by the caller.
uint32_t levels_wave_cap();
hipError_t launch_levels(const ImageDesc *descs, uint32_t images, uint32_t max_intervals, const HuffLdsPlan &plan, uint32_t hs, uint32_t vs,
                         const LevelsTarget &target, hipStream_t stream);
inline CallerDecode levels_decode(const LevelsTarget &target)
{
    return CallerDecode{&target, launch_caller_decode<LevelsTarget, launch_levels>, false,
                        [](uint32_t, uint32_t) { return levels_wave_cap(); }, COMPEG_KERNEL_LEVELS, kLevelsSlotBytes};
}

#if defined(CG_AC_STAMPS)
// diagnostic build: AC-loop cycle counters (kernels_body.h)
hipError_t read_ac_stamps(unsigned long long out[4], bool reset);
#endif

} // namespace compeg
