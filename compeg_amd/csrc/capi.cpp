// extern "C" surface of libcompeg_hip (include/compeg_hip.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include <cstring>
#include <new>
#include <string>

#include "compeg_hip.h"
#include "runtime.h"

using namespace compeg;

struct compeg_image {
    ImageData *data;
};

struct compeg_scanbuffer {
    ScanBuffer buf;
};

namespace {

thread_local std::string g_error;

int fail(const Status &s)
{
    g_error = s.message;
    return s.code;
}

int fail(int code, const char *msg)
{
    g_error = msg;
    return code;
}

int ok()
{
    return COMPEG_OK;
}

// Runs body(), turning C++ exceptions (allocation failure) into an error code
// so that nothing propagates across the C boundary.
template <class F>
int guarded(F &&body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(COMPEG_E_HIP, "out of host memory");
    } catch (const std::exception &e) {
        return fail(COMPEG_E_INVALID_ARG, e.what());
    }
}

int open_gpu(int device, hipStream_t stream, bool adopt, compeg_gpu **out)
{
    if (!out)
        return fail(COMPEG_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(COMPEG_E_HIP, "no HIP device available (libcompeg_hip needs a gfx950 GPU; "
                                  "there is no CPU fallback)");
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess)
            device = 0;
    }
    if (device >= ndev)
        return fail(COMPEG_E_INVALID_ARG, "HIP device index out of range");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess)
        return fail(hip_status(e, "hipGetDeviceProperties"));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string m = std::string("device is ") + prop.gcnArchName +
                        ", but libcompeg_hip carries gfx950 (MI355X) code objects only";
        return fail(COMPEG_E_HIP, m.c_str());
    }
    e = hipSetDevice(device);
    if (e != hipSuccess)
        return fail(hip_status(e, "hipSetDevice"));
    compeg_gpu *g = new compeg_gpu();
    g->device = device;
    g->name = prop.name[0] ? std::string(prop.name) + " (" + prop.gcnArchName + ")" : std::string(prop.gcnArchName);
    if (adopt) {
        g->stream = stream;
        g->owns_stream = false;
    } else {
        e = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete g;
            return fail(hip_status(e, "hipStreamCreate"));
        }
        g->owns_stream = true;
    }
    *out = g;
    return ok();
}

// compeg_tensor_spec as the header has it: 0 with the element size, or the error recorded.  (The texts name values,
// not the header's macros.)
int check_tensor_spec(const compeg_tensor_spec *spec, size_t *elem_bytes)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (spec->dtype > COMPEG_TENSOR_F32)
        return fail(COMPEG_E_INVALID_ARG, ("tensor spec: dtype " + std::to_string(spec->dtype) + " is none of 0 (u8), 1 (f16), 2 (bf16), 3 (f32)").c_str());
    if (spec->order > COMPEG_TENSOR_BGR)
        return fail(COMPEG_E_INVALID_ARG, ("tensor spec: order " + std::to_string(spec->order) + " is neither 0 (rgb) nor 1 (bgr)").c_str());
    const uint32_t k = spec->downscale;
    if (k != 1u && k != 2u && k != 4u && k != 8u)
        return fail(COMPEG_E_INVALID_ARG, ("tensor spec: downscale " + std::to_string(k) + " is none of 1, 2, 4, 8").c_str());
    if (spec->reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, "tensor spec: reserved must be 0");
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(spec->scale[c]) || !std::isfinite(spec->bias[c]))
            return fail(COMPEG_E_INVALID_ARG, ("tensor spec: scale or bias of plane " + std::to_string(c) + " is not finite").c_str());
    *elem_bytes = spec->dtype == COMPEG_TENSOR_U8 ? 1u : (spec->dtype == COMPEG_TENSOR_F32 ? 4u : 2u);
    return COMPEG_OK;
}

// ... and the geometry of one image's tensor; every count in size_t
int tensor_geometry(const compeg_tensor_spec *spec, uint32_t width, uint32_t height, uint32_t *ow, uint32_t *oh, size_t *bytes,
                    size_t *elem_bytes)
{
    const int rc = check_tensor_spec(spec, elem_bytes);
    if (rc != COMPEG_OK)
        return rc;
    const uint32_t k = spec->downscale;
    if (width < k || height < k)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: a " + std::to_string(width) + "x" + std::to_string(height) + " image is smaller than the downscale factor " +
                                           std::to_string(k)).c_str());
    *ow = width / k;
    *oh = height / k;
    *bytes = size_t(3) * size_t(*oh) * size_t(*ow) * *elem_bytes;
    return COMPEG_OK;
}

// What both pack calls ask of the destination.
int check_tensor_destination(const void *device_dst, size_t dst_bytes, size_t needed, size_t elem_bytes)
{
    if (!device_dst)
        return fail(COMPEG_E_INVALID_ARG, "device_dst is NULL");
    if (reinterpret_cast<uintptr_t>(device_dst) % elem_bytes != 0)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: device_dst is not aligned to its element size of " + std::to_string(elem_bytes) + " bytes").c_str());
    if (dst_bytes < needed)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: dst_bytes is " + std::to_string(dst_bytes) + ", the tensor needs " + std::to_string(needed)).c_str());
    return COMPEG_OK;
}

// compeg_resize_spec as the header has it.
int check_resize_spec(const compeg_resize_spec *resize)
{
    if (!resize)
        return fail(COMPEG_E_INVALID_ARG, "resize is NULL");
    if (resize->out_width == 0u || resize->out_height == 0u || resize->out_width > 65535u || resize->out_height > 65535u)
        return fail(COMPEG_E_INVALID_ARG, ("resize: output size " + std::to_string(resize->out_width) + "x" + std::to_string(resize->out_height) +
                                           " is not within 1..65535 both ways").c_str());
    // (the low byte is the filter; above it the antialias flag, 0x100, and nothing else)
    const uint32_t mode = resize->filter & ~uint32_t(COMPEG_RESIZE_ANTIALIAS);
    if (mode > COMPEG_RESIZE_BILINEAR)
        return fail(COMPEG_E_INVALID_ARG, ("resize: filter " + std::to_string(resize->filter) + " is neither 0 (nearest) nor 1 (bilinear)").c_str());
    if (resize->filter != mode && mode != COMPEG_RESIZE_BILINEAR)
        return fail(COMPEG_E_INVALID_ARG, ("resize: filter " + std::to_string(resize->filter) + " asks for antialias (256), which goes with 1 (bilinear) only").c_str());
    if (resize->reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, "resize: reserved must be 0");
    return COMPEG_OK;
}

// The antialias flag's ratio limit for the crop `rect` (already checked) at downscale factor k: the prefiltered extent is
// at most 64 times the output extent both ways.
int check_antialias_ratio(const compeg_resize_spec *resize, const compeg_rect &rect, uint32_t k, const std::string &which)
{
    if (!(resize->filter & COMPEG_RESIZE_ANTIALIAS))
        return COMPEG_OK;
    const uint32_t pw = rect.width / k, ph = rect.height / k;
    if (uint64_t(pw) > 64u * uint64_t(resize->out_width) || uint64_t(ph) > 64u * uint64_t(resize->out_height))
        return fail(COMPEG_E_INVALID_ARG, ("resize: " + which + "antialias reduces by 64 at the most either way, " + std::to_string(pw) + "x" + std::to_string(ph) +
                                           " to " + std::to_string(resize->out_width) + "x" + std::to_string(resize->out_height) +
                                           " is more: choose a larger downscale")
                                              .c_str());
    return COMPEG_OK;
}

// The crop of a WxH image (NULL: all of it) for downscale factor k, into `rect`; `which`: what the messages call the image.
int check_crop(const compeg_rect *crop, uint32_t width, uint32_t height, uint32_t k, const std::string &which, compeg_rect *rect)
{
    const compeg_rect r = crop ? *crop : compeg_rect{0, 0, width, height};
    const std::string text = std::to_string(r.width) + "x" + std::to_string(r.height);
    if (crop) {
        if (r.width == 0u || r.height == 0u)
            return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "crop " + text + " has a side of 0").c_str());
        // (64 bits: x + width must not wrap)
        if (uint64_t(r.x) + r.width > width || uint64_t(r.y) + r.height > height)
            return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "crop " + text + " at (" + std::to_string(r.x) + ", " + std::to_string(r.y) +
                                               ") leaves the " + std::to_string(width) + "x" + std::to_string(height) + " image").c_str());
    }
    if (r.width < k || r.height < k)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + (crop ? "a " + text + " crop" : "a " + text + " image") +
                                           " is smaller than the downscale factor " + std::to_string(k)).c_str());
    *rect = r;
    return COMPEG_OK;
}

// One region of a call whose image is WxH, into whole rectangles: `out` is the region with src and dst resolved.
// `which`: what the messages call it ("region 3: ").  The antialias limit is taken against the inner extent.
int check_region(const compeg_region *region, const compeg_tensor_spec *spec, const compeg_resize_spec *resize, uint32_t width,
                 uint32_t height, const std::string &which, compeg_region *out)
{
    const compeg_region whole{};
    const compeg_region &g = region ? *region : whole;
    if (g.reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "reserved must be 0").c_str());
    const bool src_whole = !g.src.x && !g.src.y && !g.src.width && !g.src.height;
    const bool dst_whole = !g.dst.x && !g.dst.y && !g.dst.width && !g.dst.height;
    compeg_region r{};
    r.image = g.image;
    int rc = check_crop(src_whole ? nullptr : &g.src, width, height, spec->downscale, which, &r.src);
    if (rc != COMPEG_OK)
        return rc;
    r.dst = dst_whole ? compeg_rect{0, 0, resize->out_width, resize->out_height} : g.dst;
    const std::string text = std::to_string(r.dst.width) + "x" + std::to_string(r.dst.height);
    if (r.dst.width == 0u || r.dst.height == 0u)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "dst " + text + " has a side of 0").c_str());
    // (64 bits: x + width must not wrap)
    if (uint64_t(r.dst.x) + r.dst.width > resize->out_width || uint64_t(r.dst.y) + r.dst.height > resize->out_height)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "dst " + text + " at (" + std::to_string(r.dst.x) + ", " + std::to_string(r.dst.y) +
                                           ") leaves the " + std::to_string(resize->out_width) + "x" + std::to_string(resize->out_height) + " output").c_str());
    compeg_resize_spec inner = *resize;
    inner.out_width = r.dst.width;
    inner.out_height = r.dst.height;
    rc = check_antialias_ratio(&inner, r.src, spec->downscale, which);
    if (rc != COMPEG_OK)
        return rc;
    *out = r;
    return COMPEG_OK;
}

// What every slot pack checks, behind its specs, before it looks at its object: the list and the pad's values (three by
// source channel; the luma packs': one).
int check_slot_list(const void *regions, size_t count, const float *pad, int pad_values)
{
    if (!regions)
        return fail(COMPEG_E_INVALID_ARG, "tensor: regions is NULL");
    if (count == 0)
        return fail(COMPEG_E_INVALID_ARG, "tensor: a region count of 0");
    for (int c = 0; pad && c < pad_values; c++)
        if (!std::isfinite(pad[c]))
            return fail(COMPEG_E_INVALID_ARG, pad_values == 1 ? "tensor: pad is not finite"
                                                              : ("tensor: pad of channel " + std::to_string(c) + " is not finite").c_str());
    return COMPEG_OK;
}

// compeg_filter_spec as the header has it.  (The texts name values, not the header's macros.)
int check_filter_spec(const compeg_filter_spec *filter)
{
    if (!filter)
        return fail(COMPEG_E_INVALID_ARG, "filter is NULL");
    if (filter->out_width == 0u || filter->out_height == 0u || filter->out_width > 65535u || filter->out_height > 65535u)
        return fail(COMPEG_E_INVALID_ARG, ("filter: output size " + std::to_string(filter->out_width) + "x" + std::to_string(filter->out_height) +
                                           " is not within 1..65535 both ways").c_str());
    if (filter->kernel > COMPEG_FILTER_LANCZOS3)
        return fail(COMPEG_E_INVALID_ARG, ("filter: kernel " + std::to_string(filter->kernel) +
                                           " is none of 0 (box), 1 (triangle), 2 (bicubic), 3 (lanczos3)").c_str());
    if (filter->reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, "filter: reserved must be 0");
    return COMPEG_OK;
}

// The kernel's tap limit for a checked region, n * 2S <= 128 * o both ways against the inner extent; `note`: what the
// message adds behind the extents.
int check_filter_taps(const compeg_region *out, const compeg_tensor_spec *spec, const compeg_filter_spec *filter, const std::string &which,
                      const std::string &note)
{
    static const char *const names[] = {"box", "triangle", "bicubic", "lanczos3"};
    static const uint32_t twice_support[] = {1u, 2u, 4u, 6u}, most[] = {128u, 64u, 32u, 21u};
    const uint32_t pw = out->src.width / spec->downscale, ph = out->src.height / spec->downscale, s2 = twice_support[filter->kernel];
    if (uint64_t(pw) * s2 > 128u * uint64_t(out->dst.width) || uint64_t(ph) * s2 > 128u * uint64_t(out->dst.height))
        return fail(COMPEG_E_INVALID_ARG, ("filter: " + which + names[filter->kernel] + " reduces by " + std::to_string(most[filter->kernel]) +
                                           " at the most either way, " + std::to_string(pw) + "x" + std::to_string(ph) + " to " +
                                           std::to_string(out->dst.width) + "x" + std::to_string(out->dst.height) + " is more" + note +
                                           ": choose a larger downscale")
                                              .c_str());
    return COMPEG_OK;
}

// One region of a filtered call: check_region with the kernel's tap limit in place of the antialias flag's.
int check_filtered_region(const compeg_region *region, const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width,
                          uint32_t height, const std::string &which, compeg_region *out)
{
    const compeg_resize_spec extent{filter->out_width, filter->out_height, COMPEG_RESIZE_BILINEAR, 0u}; // (no flag: no ratio check there)
    const int rc = check_region(region, spec, &extent, width, height, which, out);
    if (rc != COMPEG_OK)
        return rc;
    return check_filter_taps(out, spec, filter, which, "");
}

// One region of an oriented call whose stored image is WxH and carries the tag image_orientation: `out` is the region
// with src resolved, dst replaced by dst' (inside T, include/compeg_hip.h) and the orientation 1..8.  The messages about
// dst speak of it as the caller gave it, in the upright output.
int check_oriented_region(const compeg_oriented_region *region, const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width,
                          uint32_t height, uint32_t image_orientation, const std::string &which, compeg_oriented_region *out)
{
    const compeg_oriented_region whole{};
    const compeg_oriented_region &g = region ? *region : whole;
    if (g.reserved != 0u || g.region.reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "reserved must be 0").c_str());
    if (g.orientation > 8u)
        return fail(COMPEG_E_INVALID_ARG, ("orient: " + which + "orientation " + std::to_string(g.orientation) +
                                           " is none of 0 (the image's own tag), 1 .. 8 (the EXIF values)").c_str());
    const uint32_t o = g.orientation == COMPEG_ORIENT_FROM_IMAGE ? image_orientation : g.orientation;
    const uint32_t ow = filter->out_width, oh = filter->out_height;
    const compeg_rect &d = g.region.dst;
    const bool dst_whole = !d.x && !d.y && !d.width && !d.height;
    const compeg_rect upright = dst_whole ? compeg_rect{0, 0, ow, oh} : d;
    const std::string text = std::to_string(upright.width) + "x" + std::to_string(upright.height);
    if (upright.width == 0u || upright.height == 0u)
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "dst " + text + " has a side of 0").c_str());
    compeg_region turned = g.region;
    if (!compeg::orient_rect(ow, oh, o, upright, turned.dst))
        return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + "dst " + text + " at (" + std::to_string(upright.x) + ", " + std::to_string(upright.y) +
                                           ") leaves the " + std::to_string(ow) + "x" + std::to_string(oh) + " output").c_str());
    const bool transposes = o >= 5u;
    const compeg_resize_spec extent{transposes ? oh : ow, transposes ? ow : oh, COMPEG_RESIZE_BILINEAR, 0u}; // T's (no flag: no ratio check there)
    const int rc = check_region(&turned, spec, &extent, width, height, which, &out->region);
    if (rc != COMPEG_OK)
        return rc;
    out->orientation = o;
    out->reserved = 0u;
    return check_filter_taps(&out->region, spec, filter, which,
                             transposes ? " (orientation " + std::to_string(o) + " transposes: the crop's width goes against dst's height)" : "");
}

// compeg_nhwc_spec as the header has it.
int check_nhwc_spec(const compeg_nhwc_spec *nhwc)
{
    if (!nhwc)
        return fail(COMPEG_E_INVALID_ARG, "nhwc is NULL");
    if (nhwc->channels != 3u && nhwc->channels != 4u)
        return fail(COMPEG_E_INVALID_ARG, ("nhwc: channels " + std::to_string(nhwc->channels) + " is neither 3 nor 4").c_str());
    if (!std::isfinite(nhwc->fill))
        return fail(COMPEG_E_INVALID_ARG, "nhwc: fill is not finite");
    if (nhwc->reserved[0] != 0u || nhwc->reserved[1] != 0u)
        return fail(COMPEG_E_INVALID_ARG, "nhwc: reserved must be 0");
    return COMPEG_OK;
}

// compeg_luma_spec as the header has it.
int check_luma_spec(const compeg_luma_spec *luma)
{
    static const char *const names[] = {"R", "G", "B"};
    if (!luma)
        return fail(COMPEG_E_INVALID_ARG, "luma is NULL");
    uint64_t sum = 0;
    for (int c = 0; c < 3; c++) {
        if (luma->weights[c] > 65536u)
            return fail(COMPEG_E_INVALID_ARG, ("luma: weight " + std::to_string(luma->weights[c]) + " of " + names[c] + " is above 65536").c_str());
        sum += luma->weights[c];
    }
    if (sum != 65536u)
        return fail(COMPEG_E_INVALID_ARG, ("luma: the weights' sum " + std::to_string(sum) + " is not 65536").c_str());
    if (luma->reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, "luma: reserved must be 0");
    return COMPEG_OK;
}

// What the *_tensor_shape calls end with: the prefiltered extent of the checked source rectangle and a slot's bytes.
int shape_result(const compeg_rect &src, uint32_t k, size_t slot_bytes, uint32_t *pre_width, uint32_t *pre_height, size_t *bytes)
{
    if (pre_width)
        *pre_width = src.width / k;
    if (pre_height)
        *pre_height = src.height / k;
    if (bytes)
        *bytes = slot_bytes;
    return ok();
}

// What the pack calls ask of their object, a decoder (one image, its last: image 0) or a batch.
const char *null_text(const compeg_decoder *) { return "dec is NULL"; }
const char *null_text(const compeg_batch *) { return "batch is NULL"; }

bool output_decoded(const compeg_decoder &dec) { return dec.have_last && dec.out.ptr; }
bool output_decoded(const compeg_batch &batch) { return batch.count && batch.output_decoded; }

template <class Owner>
int check_decoded(const Owner &owner)
{
    return output_decoded(owner) ? COMPEG_OK : fail(COMPEG_E_INVALID_ARG, "tensor: nothing decoded yet");
}

template <class Owner>
hipStream_t stream_of(const Owner &owner, void *hip_stream)
{
    return hip_stream ? static_cast<hipStream_t>(hip_stream) : owner.gpu->stream;
}

// The orientation tag of image i, whatever i is (1 beyond the images: the index is refused where the list is checked)
uint32_t image_tag(const compeg_decoder &dec, uint32_t) { return dec.last_orientation; }
uint32_t image_tag(const compeg_batch &batch, uint32_t i) { return i < batch.orientations.size() ? batch.orientations[i] : 1u; }

// ... and its extent; false with what is wrong with i.  (The texture never shrinks: the last image's own extent.)
bool image_extent(const compeg_decoder &dec, uint32_t i, uint32_t *width, uint32_t *height, std::string *why)
{
    if (i != 0u) {
        *why = "image " + std::to_string(i) + ", a decoder has image 0 only";
        return false;
    }
    *width = dec.last_w;
    *height = dec.last_h;
    return true;
}

bool image_extent(const compeg_batch &batch, uint32_t i, uint32_t *width, uint32_t *height, std::string *why)
{
    if (i >= batch.count) {
        *why = "image " + std::to_string(i) + " is beyond the batch's " + std::to_string(batch.count) + " images";
        return false;
    }
    *width = batch.descs[i].out_w;
    *height = batch.descs[i].out_h;
    return true;
}

struct SlotImage {
    uint32_t width, height, orientation; // the image a region names: its stored extent and its tag
};

const compeg_region &plain(const compeg_region &region) { return region; }
const compeg_region &plain(const compeg_oriented_region &region) { return region.region; }

// What a slot family -- region, filtered, oriented, channels-last or luma tensor output -- adds to the two roads below: its
// specs (the layout's on its own: a pack checks it behind the list), how many pad values it reads, a slot's elements,
// its grid, its check of one region and its pack.
struct RegionPack {
    using Region = compeg_region;
    static constexpr int kPadValues = 3;
    const compeg_tensor_spec *spec;
    const compeg_resize_spec *resize;
    int check_specs(size_t *elem_bytes) const
    {
        const int rc = check_tensor_spec(spec, elem_bytes);
        return rc == COMPEG_OK ? check_resize_spec(resize) : rc;
    }
    int check_layout() const { return COMPEG_OK; }
    size_t slot_elements() const { return size_t(3) * size_t(resize->out_height) * size_t(resize->out_width); }
    template <class Owner>
    bool grid_fits(const Owner &, const Region *, size_t count) const { return compeg::region_grid_fits(uint32_t(count), *spec, *resize); }
    int check_one(const Region *region, const SlotImage &image, const std::string &which, Region *out) const
    {
        return check_region(region, spec, resize, image.width, image.height, which, out);
    }
    template <class Owner>
    Status pack(Owner &owner, const Region *list, size_t count, const float *pad, void *dst, hipStream_t stream) const
    {
        return owner.pack_tensor_regions(*spec, *resize, list, count, pad, dst, stream);
    }
};

struct FilterPack {
    using Region = compeg_region;
    static constexpr int kPadValues = 3;
    const compeg_tensor_spec *spec;
    const compeg_filter_spec *filter;
    int check_specs(size_t *elem_bytes) const
    {
        const int rc = check_tensor_spec(spec, elem_bytes);
        return rc == COMPEG_OK ? check_filter_spec(filter) : rc;
    }
    int check_layout() const { return COMPEG_OK; }
    size_t slot_elements() const { return size_t(3) * size_t(filter->out_height) * size_t(filter->out_width); }
    template <class Owner>
    bool grid_fits(const Owner &, const Region *, size_t count) const { return compeg::filter_grid_fits(uint32_t(count), *spec, *filter); }
    int check_one(const Region *region, const SlotImage &image, const std::string &which, Region *out) const
    {
        return check_filtered_region(region, spec, filter, image.width, image.height, which, out);
    }
    template <class Owner>
    Status pack(Owner &owner, const Region *list, size_t count, const float *pad, void *dst, hipStream_t stream) const
    {
        return owner.pack_tensor_filtered(*spec, *filter, list, count, pad, dst, stream);
    }
};

// Oriented (channels_last false: nhwc is not looked at) and channels-last tensor output (true: nhwc as the caller gave
// it, NULL included): one family, so that the two check the same things in the same order.
struct OrientPack {
    using Region = compeg_oriented_region;
    static constexpr int kPadValues = 3;
    const compeg_tensor_spec *spec;
    const compeg_filter_spec *filter;
    bool channels_last;
    const compeg_nhwc_spec *nhwc;
    int check_specs(size_t *elem_bytes) const { return FilterPack{spec, filter}.check_specs(elem_bytes); }
    int check_layout() const { return channels_last ? check_nhwc_spec(nhwc) : COMPEG_OK; }
    size_t slot_elements() const { return size_t(filter->out_height) * size_t(filter->out_width) * size_t(channels_last ? nhwc->channels : 3u); }
    // (which slot shapes the list needs takes the orientations alone; one above 8 is the list's check to name, an image
    // beyond the object's too)
    template <class Owner>
    bool grid_fits(const Owner &owner, const Region *regions, size_t count) const
    {
        bool upright = false, transposed = false;
        for (size_t r = 0; r < count; r++) {
            const uint32_t o = regions[r].orientation == COMPEG_ORIENT_FROM_IMAGE ? image_tag(owner, regions[r].region.image) : regions[r].orientation;
            (o < 5u ? upright : transposed) = true;
        }
        return compeg::orient_grid_fits(uint32_t(count), *spec, *filter, upright, transposed);
    }
    // (src as a whole rectangle, dst as dst', the orientation 1..8)
    int check_one(const Region *region, const SlotImage &image, const std::string &which, Region *out) const
    {
        return check_oriented_region(region, spec, filter, image.width, image.height, image.orientation, which, out);
    }
    template <class Owner>
    Status pack(Owner &owner, const Region *list, size_t count, const float *pad, void *dst, hipStream_t stream) const
    {
        return owner.pack_tensor_oriented(*spec, *filter, channels_last ? nhwc : nullptr, list, count, pad, dst, stream);
    }
};

// Luma tensor output: the oriented family's specs, grid and check of a region; one element a pixel, the weights for a
// layout (luma as the caller gave it, NULL included), one pad value.
struct LumaPack {
    using Region = compeg_oriented_region;
    static constexpr int kPadValues = 1;
    const compeg_tensor_spec *spec;
    const compeg_filter_spec *filter;
    const compeg_luma_spec *luma;
    OrientPack oriented() const { return OrientPack{spec, filter, false, nullptr}; }
    int check_specs(size_t *elem_bytes) const { return oriented().check_specs(elem_bytes); }
    int check_layout() const { return check_luma_spec(luma); }
    size_t slot_elements() const { return size_t(filter->out_height) * size_t(filter->out_width); }
    template <class Owner>
    bool grid_fits(const Owner &owner, const Region *regions, size_t count) const { return oriented().grid_fits(owner, regions, count); }
    int check_one(const Region *region, const SlotImage &image, const std::string &which, Region *out) const
    {
        return oriented().check_one(region, image, which, out);
    }
    template <class Owner>
    Status pack(Owner &owner, const Region *list, size_t count, const float *pad, void *dst, hipStream_t stream) const
    {
        return owner.pack_tensor_luma(*spec, *filter, *luma, list, count, pad, dst, stream);
    }
};

// compeg_{region,filtered,oriented,nhwc,luma}_tensor_shape: the family's specs and its check of one region of a width x height
// image that carries no tag; then the prefiltered extent of the region's source and a slot's bytes.
template <class Family>
int slot_tensor_shape(const Family &family, const typename Family::Region *region, uint32_t width, uint32_t height, uint32_t *pre_width,
                      uint32_t *pre_height, size_t *bytes_per_slot)
{
    return guarded([&] {
        size_t elem = 0;
        int rc = family.check_specs(&elem);
        if (rc == COMPEG_OK)
            rc = family.check_layout();
        typename Family::Region r{};
        if (rc == COMPEG_OK)
            rc = family.check_one(region, SlotImage{width, height, 1u}, "", &r);
        if (rc != COMPEG_OK)
            return rc;
        return shape_result(plain(r).src, family.spec->downscale, family.slot_elements() * elem, pre_width, pre_height, bytes_per_slot);
    });
}

// Every slot pack call, of either object: what does not depend on the object first (it is checked where no device
// is), the launch's limits and the destination before the list is copied (nothing is allocated for a count no call
// takes), then the copy of the caller's list, every region checked and resolved to whole rectangles.
template <class Owner, class Family>
int pack_slot_tensor(Owner *owner, const Family &family, const typename Family::Region *regions, size_t count, const float *pad,
                     void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return guarded([&] {
        size_t elem = 0;
        int rc = family.check_specs(&elem);
        if (rc == COMPEG_OK)
            rc = check_slot_list(regions, count, pad, Family::kPadValues);
        if (rc == COMPEG_OK)
            rc = family.check_layout();
        if (rc != COMPEG_OK)
            return rc;
        if (!owner)
            return fail(COMPEG_E_INVALID_ARG, null_text(owner));
        rc = check_decoded(*owner);
        if (rc != COMPEG_OK)
            return rc;
        const size_t slot = family.slot_elements() * elem;
        if (count > SIZE_MAX / slot)
            return fail(COMPEG_E_INVALID_ARG, "tensor: the byte count of this many regions does not fit size_t");
        if (count > 0xffffffffull || !family.grid_fits(*owner, regions, count))
            return fail(COMPEG_E_INVALID_ARG, "tensor: the grid of this many regions of this output extent does not fit one launch");
        rc = check_tensor_destination(device_dst, dst_bytes, slot * count, elem);
        if (rc != COMPEG_OK)
            return rc;
        std::vector<typename Family::Region> list(count);
        for (size_t r = 0; r < count; r++) {
            const std::string which = "region " + std::to_string(r) + ": ";
            const uint32_t i = plain(regions[r]).image;
            SlotImage image{0u, 0u, image_tag(*owner, i)};
            std::string why;
            if (!image_extent(*owner, i, &image.width, &image.height, &why))
                return fail(COMPEG_E_INVALID_ARG, ("tensor: " + which + why).c_str());
            rc = family.check_one(regions + r, image, which, &list[r]);
            if (rc != COMPEG_OK)
                return rc;
        }
        float pad_copy[3] = {0.0f, 0.0f, 0.0f};
        for (int c = 0; pad && c < Family::kPadValues; c++)
            pad_copy[c] = pad[c];
        Status s = family.pack(*owner, list.data(), count, pad_copy, device_dst, stream_of(*owner, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

} // namespace

extern "C" {

const char *compeg_last_error(void)
{
    return g_error.c_str();
}

const char *compeg_version(void)
{
    return "compeg-hip 0.1.0 (gfx950)";
}

int compeg_gpu_open(int device, compeg_gpu **out)
{
    return guarded([&] { return open_gpu(device, nullptr, false, out); });
}

int compeg_gpu_from_stream(int device, void *hip_stream, compeg_gpu **out)
{
    return guarded([&] { return open_gpu(device, static_cast<hipStream_t>(hip_stream), true, out); });
}

void compeg_gpu_retain(compeg_gpu *gpu)
{
    if (gpu)
        gpu->refs.fetch_add(1, std::memory_order_relaxed);
}

void compeg_gpu_release(compeg_gpu *gpu)
{
    if (!gpu)
        return;
    if (gpu->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {
        if (gpu->owns_stream && gpu->stream) {
            (void)hipSetDevice(gpu->device);
            (void)hipStreamSynchronize(gpu->stream);
            (void)hipStreamDestroy(gpu->stream);
        }
        delete gpu;
    }
}

int compeg_gpu_device(const compeg_gpu *gpu)
{
    return gpu ? gpu->device : -1;
}

const char *compeg_gpu_name(const compeg_gpu *gpu)
{
    return gpu ? gpu->name.c_str() : "";
}

/* ---- ImageData ------------------------------------------------------------ */

int compeg_image_parse(const uint8_t *jpeg, size_t len, int copy, compeg_image **out)
{
    return compeg_image_parse_ext(jpeg, len, copy, 0u, out);
}

int compeg_image_parse_ext(const uint8_t *jpeg, size_t len, int copy, unsigned flags, compeg_image **out)
{
    return guarded([&] {
        if (!out)
            return fail(COMPEG_E_INVALID_ARG, "out is NULL");
        *out = nullptr;
        if (flags & ~(COMPEG_PARSE_ANY_LUMA_SAMPLING | COMPEG_PARSE_STANDARD_ENTROPY | COMPEG_PARSE_GRAYSCALE))
            return fail(COMPEG_E_INVALID_ARG, "unknown parse flags");
        ImageData *d = nullptr;
        Status s = ImageData::parse(jpeg, len, copy != 0, &d, flags);
        if (!s.ok())
            return fail(s);
        *out = new compeg_image{d};
        return ok();
    });
}

void compeg_image_free(compeg_image *img)
{
    if (img) {
        delete img->data;
        delete img;
    }
}

uint32_t compeg_image_width(const compeg_image *img)
{
    return img ? img->data->width : 0;
}

uint32_t compeg_image_height(const compeg_image *img)
{
    return img ? img->data->height : 0;
}

uint32_t compeg_image_parallelism(const compeg_image *img)
{
    return img ? img->data->metadata.total_restart_intervals : 0;
}

uint32_t compeg_image_components(const compeg_image *img)
{
    return img ? img->data->components : 0;
}

const uint8_t *compeg_image_metadata(const compeg_image *img)
{
    return img ? reinterpret_cast<const uint8_t *>(&img->data->metadata) : nullptr;
}

const uint8_t *compeg_image_huffman_l1(const compeg_image *img)
{
    return img ? reinterpret_cast<const uint8_t *>(img->data->l1) : nullptr;
}

const uint8_t *compeg_image_huffman_l2(const compeg_image *img, size_t *nbytes)
{
    if (nbytes)
        *nbytes = img ? img->data->l2.size() * 2 : 0;
    return img ? reinterpret_cast<const uint8_t *>(img->data->l2.data()) : nullptr;
}

void compeg_image_scan_range(const compeg_image *img, size_t *offset, size_t *len)
{
    if (offset)
        *offset = img ? img->data->scan_offset : 0;
    if (len)
        *len = img ? img->data->scan_len : 0;
}

/* ---- ScanBuffer ----------------------------------------------------------- */

compeg_scanbuffer *compeg_scanbuffer_new(void)
{
    try {
        return new compeg_scanbuffer();
    } catch (...) {
        return nullptr;
    }
}

void compeg_scanbuffer_free(compeg_scanbuffer *sb)
{
    delete sb;
}

int compeg_scanbuffer_process(compeg_scanbuffer *sb, const uint8_t *scan, size_t len,
                              uint32_t expected_restart_intervals)
{
    return guarded([&] {
        if (!sb || (!scan && len))
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        Status s = sb->buf.process(scan, len, expected_restart_intervals);
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_scanbuffer_set_threads(compeg_scanbuffer *sb, unsigned threads)
{
    return guarded([&] {
        if (!sb || threads < 1 || threads > 16)
            return fail(COMPEG_E_INVALID_ARG, "threads must be 1..16");
        sb->buf.set_threads(threads);
        return ok();
    });
}

int compeg_scanbuffer_process_on_gpu(compeg_scanbuffer *sb, compeg_gpu *gpu, const uint8_t *scan,
                                     size_t len, uint32_t expected_restart_intervals)
{
    return guarded([&] {
        if (!sb || !gpu || (!scan && len))
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        Status s = sb->buf.process_on_gpu(gpu, scan, len, expected_restart_intervals);
        return s.ok() ? ok() : fail(s);
    });
}

const uint8_t *compeg_scanbuffer_data(const compeg_scanbuffer *sb, size_t *nbytes)
{
    if (nbytes)
        *nbytes = sb ? sb->buf.data_bytes() : 0;
    return sb ? sb->buf.data() : nullptr;
}

const uint8_t *compeg_scanbuffer_start_positions(const compeg_scanbuffer *sb, size_t *nbytes)
{
    if (nbytes)
        *nbytes = sb ? sb->buf.nstarts() * 4 : 0;
    return sb ? reinterpret_cast<const uint8_t *>(sb->buf.starts()) : nullptr;
}

/* ---- Decoder -------------------------------------------------------------- */

int compeg_decoder_new(compeg_gpu *gpu, compeg_decoder **out)
{
    return guarded([&] {
        if (!gpu || !out)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        hipError_t e = hipSetDevice(gpu->device);
        if (e != hipSuccess)
            return fail(hip_status(e, "hipSetDevice"));
        compeg_decoder *d = new compeg_decoder();
        compeg_gpu_retain(gpu);
        d->gpu = gpu;
        *out = d;
        return ok();
    });
}

void compeg_decoder_free(compeg_decoder *dec)
{
    if (dec) {
        (void)hipSetDevice(dec->gpu->device);
        delete dec;
    }
}

int compeg_decoder_enqueue(compeg_decoder *dec, const compeg_image *img, void *hip_stream,
                           int *texture_changed)
{
    return guarded([&] {
        if (!dec || !img)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        bool changed = false;
        Status s = dec->enqueue(*img->data, static_cast<hipStream_t>(hip_stream), &changed);
        if (texture_changed)
            *texture_changed = changed ? 1 : 0;
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_decoder_start_decode(compeg_decoder *dec, const compeg_image *img, compeg_op **op)
{
    return guarded([&] {
        if (!dec || !img || !op)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        *op = nullptr;
        bool changed = false;
        Status s = dec->enqueue(*img->data, dec->gpu->stream, &changed);
        if (!s.ok())
            return fail(s);
        compeg_op *o = new compeg_op();
        o->device = dec->gpu->device;
        o->texture_changed = changed;
        hipError_t e = hipEventCreateWithFlags(&o->done, hipEventDisableTiming);
        if (e == hipSuccess)
            e = hipEventRecord(o->done, dec->gpu->stream);
        if (e != hipSuccess) {
            compeg_op_free(o);
            return fail(hip_status(e, "hipEventRecord"));
        }
        *op = o;
        return ok();
    });
}

int compeg_decoder_decode_blocking(compeg_decoder *dec, const compeg_image *img, compeg_op **op)
{
    // like start_decode + wait; a blocking decode may run the device-side scan preprocessing
    // without the read-back in the middle and look at its outcome afterwards
    return guarded([&] {
        if (!dec || !img || !op)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        *op = nullptr;
        bool changed = false;
        Status s = dec->enqueue(*img->data, dec->gpu->stream, &changed, true);
        if (!s.ok())
            return fail(s);
        const auto t_poll = std::chrono::steady_clock::now();
        hipError_t e = hipStreamSynchronize(dec->gpu->stream);
        if (e != hipSuccess)
            return fail(hip_status(e, "hipStreamSynchronize"));
        // (the stream is drained: nothing of this decode is pending -- enqueue recorded no events for a blocking decode)
        dec->upload_pending = dec->decode_pending = false;
        const compeg_stage_times first = dec->stage_times; // (a re-decode through the host path would reset them)
        s = dec->finish_deferred(*img->data, dec->gpu->stream);
        if (!s.ok())
            return fail(s);
        dec->stage_times = first;
        dec->stage_times.poll_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_poll).count();
        // (an operation that is complete already: no event to wait for)
        compeg_op *o = new compeg_op();
        o->device = dec->gpu->device;
        o->texture_changed = changed;
        *op = o;
        return ok();
    });
}

int compeg_decoder_set_device_preprocess(compeg_decoder *dec, int on)
{
    if (!dec)
        return fail(COMPEG_E_INVALID_ARG, "dec is NULL");
    dec->device_preprocess = on != 0;
    return ok();
}

int compeg_decoder_set_scan_threads(compeg_decoder *dec, unsigned threads)
{
    return guarded([&] {
        if (!dec || threads < 1 || threads > 16)
            return fail(COMPEG_E_INVALID_ARG, "threads must be 1..16");
        dec->scan.set_threads(threads);
        return ok();
    });
}

const char *compeg_decoder_last_warning(const compeg_decoder *dec)
{
    return dec ? dec->warning.c_str() : "";
}

int compeg_decoder_last_kernel(const compeg_decoder *dec) { return dec ? dec->last_kernel : COMPEG_KERNEL_NONE; }

int compeg_decoder_last_stage_times(const compeg_decoder *dec, compeg_stage_times *out)
{
    if (!dec || !out)
        return fail(COMPEG_E_INVALID_ARG, "NULL argument");
    *out = dec->stage_times;
    return ok();
}

int compeg_op_wait(compeg_op *op)
{
    if (!op)
        return fail(COMPEG_E_INVALID_ARG, "op is NULL");
    if (!op->done)
        return ok(); // (a blocking decode's: complete when it was made)
    hipError_t e = hipEventSynchronize(op->done);
    return e == hipSuccess ? ok() : fail(hip_status(e, "hipEventSynchronize"));
}

int compeg_op_texture_changed(const compeg_op *op)
{
    return op && op->texture_changed ? 1 : 0;
}

void compeg_op_free(compeg_op *op)
{
    if (op) {
        if (op->done)
            (void)hipEventDestroy(op->done);
        delete op;
    }
}

int compeg_decoder_output(const compeg_decoder *dec, void **device_ptr, uint32_t *width,
                          uint32_t *height, size_t *pitch_bytes)
{
    if (!dec)
        return fail(COMPEG_E_INVALID_ARG, "dec is NULL");
    if (device_ptr)
        *device_ptr = dec->out.ptr;
    if (width)
        *width = dec->out_w;
    if (height)
        *height = dec->out_h;
    if (pitch_bytes)
        *pitch_bytes = dec->out_pitch;
    return ok();
}

int compeg_decoder_take_output(compeg_decoder *dec, void **device_ptr, uint32_t *width,
                               uint32_t *height, size_t *pitch_bytes)
{
    if (!dec || !device_ptr)
        return fail(COMPEG_E_INVALID_ARG, "NULL argument");
    (void)hipSetDevice(dec->gpu->device);
    hipError_t e = hipStreamSynchronize(dec->last_stream);
    if (e != hipSuccess)
        return fail(hip_status(e, "hipStreamSynchronize"));
    compeg_decoder_output(dec, nullptr, width, height, pitch_bytes);
    *device_ptr = dec->out.release();
    delete dec;
    return ok();
}

void compeg_device_free(void *device_ptr)
{
    if (device_ptr)
        (void)hipFree(device_ptr);
}

int compeg_decoder_read_output(compeg_decoder *dec, uint8_t *host_rgba, uint32_t width,
                               uint32_t height)
{
    return guarded([&] {
        if (!dec || !host_rgba)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        if (width > dec->out_w || height > dec->out_h)
            return fail(COMPEG_E_INVALID_ARG, "requested area exceeds the output");
        (void)hipSetDevice(dec->gpu->device);
        hipError_t e = hipStreamSynchronize(dec->last_stream);
        if (e == hipSuccess && width && height)
            e = hipMemcpy2D(host_rgba, size_t(width) * 4, dec->out.ptr, dec->out_pitch,
                            size_t(width) * 4, height, hipMemcpyDeviceToHost);
        return e == hipSuccess ? ok() : fail(hip_status(e, "read_output"));
    });
}

int compeg_decoder_read_coefficients(compeg_decoder *dec, int32_t *host, size_t count)
{
    return guarded([&] {
        if (!dec || !host || !dec->have_last)
            return fail(COMPEG_E_INVALID_ARG, "no decode to read back");
        const Metadata &md = dec->last_md;
        const size_t dus =
            size_t(md.total_restart_intervals) * md.restart_interval * md.dus_per_mcu;
        if (count < dus * kRetained)
            return fail(COMPEG_E_INVALID_ARG, "coefficient buffer too small");
        (void)hipSetDevice(dec->gpu->device);
        hipError_t e = hipStreamSynchronize(dec->last_stream);
        if (e != hipSuccess)
            return fail(hip_status(e, "hipStreamSynchronize"));
        std::vector<int16_t> ac(dus * kRetained);
        std::vector<int32_t> dc(dus);
        if (dus && !dec->coefficients_valid) {
            // the fused kernel keeps coefficients on chip: rerun the entropy
            // stage alone into the scratch buffers for this debug read-back
            const HuffLdsPlan plan = plan_huffman(md.total_restart_intervals, 1, dec->last_plan.l2_entries_in_lds,
                                                  dec->last_span, false);
            e = launch_huffman(static_cast<const ImageDesc *>(dec->last_desc_dev), 1,
                               md.total_restart_intervals, plan, dec->last_stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(dec->last_stream);
            if (e != hipSuccess)
                return fail(hip_status(e, "huffman_kernel (coefficient read-back)"));
            dec->coefficients_valid = true;
        }
        if (dus) {
            e = hipMemcpy(ac.data(), dec->ac.ptr, ac.size() * 2, hipMemcpyDeviceToHost);
            if (e == hipSuccess)
                e = hipMemcpy(dc.data(), dec->dc.ptr, dc.size() * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess)
                return fail(hip_status(e, "hipMemcpy"));
        }
        // component of every data unit inside an MCU, in scan order
        uint32_t comp_of[kMaxDusPerMcu] = {0};
        uint32_t k = 0;
        for (uint32_t c = 0; c < 3; c++)
            for (uint32_t i = 0; i < md.components[c].hsample * md.components[c].vsample &&
                                 k < uint32_t(kMaxDusPerMcu);
                 i++)
                comp_of[k++] = c;
        for (size_t du = 0; du < dus; du++) {
            const uint32_t *q = md.qtables[md.components[comp_of[du % md.dus_per_mcu]].qtable & 3];
            host[du * kRetained] = dc[du];
            for (int z = 1; z < kRetained; z++)
                host[du * kRetained + z] = int32_t(uint32_t(int32_t(ac[du * kRetained + z])) * q[z]);
        }
        return ok();
    });
}

#if defined(CG_AC_STAMPS)
extern "C" __attribute__((visibility("default"))) int compeg_debug_ac_stamps(unsigned long long *out, int reset)
{
    return compeg::read_ac_stamps(out, reset != 0) == hipSuccess ? 0 : -1;
}
#endif

/* Diagnostic builds (-DCG_STAMPS) park per-wave cycle stamps in the dc scratch buffers; these
 * two undeclared helpers read them back.  Not part of the API. */
__attribute__((visibility("default"))) int compeg_debug_read_dc(compeg_decoder *dec, void *host, size_t bytes)
{
    if (!dec || !dec->dc.ptr || bytes > dec->dc.capacity)
        return COMPEG_E_INVALID_ARG;
    (void)hipStreamSynchronize(dec->last_stream);
    return hipMemcpy(host, dec->dc.ptr, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : COMPEG_E_HIP;
}

__attribute__((visibility("default"))) int compeg_debug_read_batch_dc(compeg_batch *b, void *host, size_t bytes)
{
    if (!b || !b->dc.ptr || bytes > b->dc.capacity)
        return COMPEG_E_INVALID_ARG;
    (void)hipStreamSynchronize(b->last_stream);
    return hipMemcpy(host, b->dc.ptr, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : COMPEG_E_HIP;
}

/* ---- Batch ---------------------------------------------------------------- */

int compeg_batch_new(compeg_gpu *gpu, compeg_batch **out)
{
    return guarded([&] {
        if (!gpu || !out)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        compeg_batch *b = new compeg_batch();
        compeg_gpu_retain(gpu);
        b->gpu = gpu;
        *out = b;
        return ok();
    });
}

void compeg_batch_free(compeg_batch *batch)
{
    if (batch) {
        (void)hipSetDevice(batch->gpu->device);
        delete batch;
    }
}

int compeg_batch_upload(compeg_batch *batch, const compeg_image *const *images, size_t count,
                        int host_threads)
{
    return guarded([&] {
        if (!batch || (!images && count))
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        std::vector<const ImageData *> ptrs(count);
        for (size_t i = 0; i < count; i++) {
            if (!images[i])
                return fail(COMPEG_E_INVALID_ARG, "NULL image in batch");
            ptrs[i] = images[i]->data;
        }
        Status s = batch->upload(ptrs.data(), count, host_threads);
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_upload_jpegs(compeg_batch *batch, const uint8_t *const *jpegs, const size_t *lengths, size_t count,
                              int host_threads, unsigned flags)
{
    return guarded([&] {
        if (!batch || ((!jpegs || !lengths) && count))
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        for (size_t i = 0; i < count; i++)
            if (!jpegs[i])
                return fail(COMPEG_E_INVALID_ARG, "NULL image in batch");
        Status s = batch->upload_jpegs(jpegs, lengths, count, host_threads, flags);
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_upload_jpegs_begin(compeg_batch *batch, const uint8_t *const *jpegs, const size_t *lengths, size_t count,
                                    int host_threads, unsigned flags)
{
    return guarded([&] {
        if (!batch || ((!jpegs || !lengths) && count))
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        for (size_t i = 0; i < count; i++)
            if (!jpegs[i])
                return fail(COMPEG_E_INVALID_ARG, "NULL image in batch");
        Status s = batch->upload_jpegs(jpegs, lengths, count, host_threads, flags, true);
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_upload_end(compeg_batch *batch)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        Status s = batch->finish_upload();
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_decode(compeg_batch *batch, void *hip_stream)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : batch->gpu->stream;
        Status s = batch->decode(st);
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_wait(compeg_batch *batch)
{
    if (!batch)
        return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
    (void)hipSetDevice(batch->gpu->device);
    hipError_t e = hipStreamSynchronize(batch->last_stream ? batch->last_stream : batch->gpu->stream);
    return e == hipSuccess ? ok() : fail(hip_status(e, "hipStreamSynchronize"));
}

size_t compeg_batch_count(const compeg_batch *batch)
{
    return batch ? batch->count : 0;
}

int compeg_batch_set_device_preprocess(compeg_batch *batch, int mode)
{
    if (!batch || mode < 0 || mode > 2)
        return fail(COMPEG_E_INVALID_ARG, "bad argument");
    batch->preprocess_mode = mode;
    return ok();
}

size_t compeg_batch_host_fallbacks(const compeg_batch *batch)
{
    return batch ? batch->host_fallbacks : 0;
}

int compeg_batch_set_chunk(compeg_batch *batch, uint32_t images_per_launch)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        if (batch->chunk == images_per_launch)
            return ok();
        batch->chunk = images_per_launch;
        // (the launches change size: some of them may now be the cooperative kernel's, which wants its walk tables, or
        // take the walk + lane-per-MCU route, which wants its records' buffers)
        if (batch->count) {
            if (batch->last_stream && hipStreamSynchronize(batch->last_stream) != hipSuccess)
                return fail(COMPEG_E_HIP, "hipStreamSynchronize failed");
            if (hipSetDevice(batch->gpu->device) != hipSuccess)
                return fail(COMPEG_E_HIP, "hipSetDevice failed");
            compeg::Status st = batch->make_walk_tables(batch->gpu->stream, batch->count);
            if (!st.ok())
                return fail(st);
            if (hipStreamSynchronize(batch->gpu->stream) != hipSuccess)
                return fail(COMPEG_E_HIP, "hipStreamSynchronize failed");
        }
        return ok();
    });
}

int compeg_host_feed_work(const uint8_t *const *jpegs, const size_t *lengths, size_t count, int host_threads, unsigned flags,
                          int road, int reps, double *seconds)
{
    return guarded([&] {
        if (!jpegs || !lengths || !seconds || count == 0 || reps <= 0 || road < 0 || road > 2)
            return fail(COMPEG_E_INVALID_ARG, "bad arguments");
        const unsigned nthreads = unsigned(std::max(1, host_threads));
        // Roads 0 and 2 write what they make where an upload would: every image has a place of its own in one arena
        // (kept between calls: an upload's pinned arena is), so that a batch larger than the caches costs the memory
        // traffic it costs there -- every byte read once and written once.
        static std::mutex arena_lock;
        static std::vector<uint8_t> arena;
        std::vector<size_t> at(count + 1, 0);
        for (size_t i = 0; i < count; i++)
            at[i + 1] = at[i] + ((road == 0 ? compeg::ScanBuffer::output_capacity(lengths[i]) : lengths[i]) + 255) / 256 * 256;
        std::unique_lock<std::mutex> hold(arena_lock);
        if (road != 1 && arena.size() < at[count])
            arena.resize(at[count]);
        std::vector<std::vector<uint32_t>> starts(nthreads);
        std::vector<compeg::Status> status(nthreads);
        std::atomic<size_t> next{0};
        const size_t total = count * size_t(reps);
        auto work = [&](unsigned t) {
            for (;;) {
                const size_t k = next.fetch_add(1, std::memory_order_relaxed);
                if (k >= total || !status[t].ok())
                    return;
                const size_t i = k % count;
                compeg::ImageData *img = nullptr;
                compeg::Status st = compeg::ImageData::parse(jpegs[i], lengths[i], false, &img,
                                                             road != 0 ? flags | compeg::kParseDeferScanEnd : flags);
                std::unique_ptr<compeg::ImageData> owned(img);
                if (st.ok() && road == 0) {
                    const uint32_t expected = img->metadata.total_restart_intervals;
                    starts[t].resize(compeg::ScanBuffer::start_slots(expected));
                    size_t nwords = 0, nstarts = 0;
                    st = compeg::ScanBuffer::process_to(img->scan_data(), img->scan_len, expected, arena.data() + at[i], starts[t].data(),
                                                        nwords, nstarts);
                    if (st.code == COMPEG_E_COUNT_MISMATCH)
                        st = compeg::Status{};
                } else if (st.ok() && road == 2) {
                    memcpy(arena.data() + at[i], jpegs[i], lengths[i]); // (pageable bytes: into the pinned arena, whole)
                }
                if (!st.ok())
                    status[t] = st;
            }
        };
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> threads;
        struct JoinAll {
            std::vector<std::thread> &v;
            ~JoinAll()
            {
                for (std::thread &th : v)
                    if (th.joinable())
                        th.join();
            }
        } join_all{threads}; // (also when starting a thread throws midway)
        threads.reserve(nthreads);
        for (unsigned t = 1; t < nthreads; t++)
            threads.emplace_back(work, t);
        work(0);
        for (std::thread &th : threads)
            th.join();
        *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (const compeg::Status &st : status)
            if (!st.ok())
                return fail(st);
        return ok();
    });
}

int compeg_host_alloc(size_t bytes, void **out)
{
    if (!out)
        return fail(COMPEG_E_INVALID_ARG, "out is NULL");
    *out = nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess || !p)
        return fail(COMPEG_E_HIP, "hipHostMalloc failed");
    *out = p;
    return ok();
}

void compeg_host_free(void *ptr)
{
    if (ptr)
        (void)hipHostFree(ptr);
}

int compeg_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes)
        return fail(COMPEG_E_INVALID_ARG, "nothing to register");
    if (hipHostRegister(ptr, bytes, hipHostRegisterPortable) != hipSuccess)
        return fail(COMPEG_E_HIP, "hipHostRegister failed");
    return ok();
}

int compeg_host_unregister(void *ptr)
{
    if (!ptr)
        return fail(COMPEG_E_INVALID_ARG, "ptr is NULL");
    if (hipHostUnregister(ptr) != hipSuccess)
        return fail(COMPEG_E_HIP, "hipHostUnregister failed");
    return ok();
}

int compeg_batch_last_kernel(const compeg_batch *batch) { return batch ? batch->last_kernel : COMPEG_KERNEL_NONE; }

int compeg_batch_output(const compeg_batch *batch, size_t index, void **device_ptr, uint32_t *width,
                        uint32_t *height, size_t *pitch_bytes)
{
    if (!batch || index >= batch->count)
        return fail(COMPEG_E_INVALID_ARG, "batch index out of range");
    const ImageDesc &d = batch->descs[index];
    if (device_ptr)
        *device_ptr = d.out;
    if (width)
        *width = d.out_w;
    if (height)
        *height = d.out_h;
    if (pitch_bytes)
        *pitch_bytes = d.out_pitch;
    return ok();
}

int compeg_batch_read_output(compeg_batch *batch, size_t index, uint8_t *host_rgba)
{
    return guarded([&] {
        if (!batch || index >= batch->count || !host_rgba)
            return fail(COMPEG_E_INVALID_ARG, "bad argument");
        int rc = compeg_batch_wait(batch);
        if (rc != COMPEG_OK)
            return rc;
        const ImageDesc &d = batch->descs[index];
        // (tightly packed on the host; the device rows are out_pitch apart)
        hipError_t e = d.out_w && d.out_h ? hipMemcpy2D(host_rgba, size_t(d.out_w) * 4, d.out, d.out_pitch, size_t(d.out_w) * 4, d.out_h,
                                                        hipMemcpyDeviceToHost)
                                          : hipSuccess;
        return e == hipSuccess ? ok() : fail(hip_status(e, "hipMemcpy2D"));
    });
}

uint64_t compeg_batch_algorithmic_bytes(const compeg_batch *batch)
{
    return batch ? batch->algorithmic_bytes : 0;
}

uint64_t compeg_batch_pixels(const compeg_batch *batch)
{
    return batch ? batch->pixels : 0;
}

int compeg_batch_set_timing(compeg_batch *batch, int on)
{
    if (!batch)
        return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
    batch->timing_on = on != 0;
    return ok();
}

int compeg_batch_timing(compeg_batch *batch, int reset, uint32_t *decodes, double *total_ms,
                        double stage_ms[2])
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        (void)hipSetDevice(batch->gpu->device);
        double t = 0, a = 0, b = 0;
        const bool split = !batch->chunk || batch->chunk >= batch->count;
        for (size_t i = 0; i < batch->decodes_timed; i++) {
            hipEvent_t *ev = batch->events.data() + i * 3;
            hipError_t e = hipEventSynchronize(ev[2]);
            float x = 0, y = 0, z = 0;
            if (e == hipSuccess)
                e = hipEventElapsedTime(&x, ev[0], ev[2]);
            const bool staged = i < batch->has_stage_event.size() && batch->has_stage_event[i];
            if (e == hipSuccess && split && staged) {
                e = hipEventElapsedTime(&y, ev[0], ev[1]);
                if (e == hipSuccess)
                    e = hipEventElapsedTime(&z, ev[1], ev[2]);
            } else if (e == hipSuccess && split) {
                y = x; // (one kernel does the whole path)
            }
            if (e != hipSuccess)
                return fail(hip_status(e, "hipEventElapsedTime"));
            t += x;
            a += y;
            b += z;
        }
        if (decodes)
            *decodes = uint32_t(batch->decodes_timed);
        if (total_ms)
            *total_ms = t;
        if (stage_ms) {
            stage_ms[0] = a;
            stage_ms[1] = b;
        }
        if (reset)
            batch->decodes_timed = 0;
        return ok();
    });
}

/* ---- Tensor output -------------------------------------------------------- */

int compeg_tensor_shape(const compeg_tensor_spec *spec, uint32_t width, uint32_t height, uint32_t *out_width,
                        uint32_t *out_height, size_t *bytes_per_image)
{
    return guarded([&] {
        uint32_t ow = 0, oh = 0;
        size_t bytes = 0, elem = 0;
        const int rc = tensor_geometry(spec, width, height, &ow, &oh, &bytes, &elem);
        if (rc != COMPEG_OK)
            return rc;
        if (out_width)
            *out_width = ow;
        if (out_height)
            *out_height = oh;
        if (bytes_per_image)
            *bytes_per_image = bytes;
        return ok();
    });
}

int compeg_decoder_pack_tensor(compeg_decoder *dec, const compeg_tensor_spec *spec, void *device_dst, size_t dst_bytes,
                               void *hip_stream)
{
    return guarded([&] {
        if (!dec)
            return fail(COMPEG_E_INVALID_ARG, null_text(dec));
        size_t elem = 0;
        int rc = check_tensor_spec(spec, &elem);
        if (rc == COMPEG_OK)
            rc = check_decoded(*dec);
        if (rc != COMPEG_OK)
            return rc;
        // (the texture never shrinks: the last image's own extent, at the allocation's pitch)
        uint32_t ow = 0, oh = 0;
        size_t bytes = 0;
        rc = tensor_geometry(spec, dec->last_w, dec->last_h, &ow, &oh, &bytes, &elem);
        if (rc == COMPEG_OK)
            rc = check_tensor_destination(device_dst, dst_bytes, bytes, elem);
        if (rc != COMPEG_OK)
            return rc;
        Status s = dec->pack_tensor(*spec, device_dst, stream_of(*dec, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_pack_tensor(compeg_batch *batch, const compeg_tensor_spec *spec, void *device_dst, size_t dst_bytes,
                             void *hip_stream)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, null_text(batch));
        size_t elem = 0;
        int rc = check_tensor_spec(spec, &elem);
        if (rc == COMPEG_OK)
            rc = check_decoded(*batch);
        if (rc != COMPEG_OK)
            return rc;
        const ImageDesc &first = batch->descs[0];
        for (size_t i = 1; i < batch->count; i++)
            if (batch->descs[i].out_w != first.out_w || batch->descs[i].out_h != first.out_h)
                return fail(COMPEG_E_INVALID_ARG, ("tensor: the batch's images are not all of one size (image " + std::to_string(i) + " is " +
                                                   std::to_string(batch->descs[i].out_w) + "x" + std::to_string(batch->descs[i].out_h) + ", image 0 " +
                                                   std::to_string(first.out_w) + "x" + std::to_string(first.out_h) + ")").c_str());
        uint32_t ow = 0, oh = 0;
        size_t bytes = 0;
        rc = tensor_geometry(spec, first.out_w, first.out_h, &ow, &oh, &bytes, &elem);
        if (rc == COMPEG_OK)
            rc = check_tensor_destination(device_dst, dst_bytes, bytes * batch->count, elem);
        if (rc != COMPEG_OK)
            return rc;
        Status s = batch->pack_tensor(*spec, device_dst, stream_of(*batch, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

/* ---- Resized tensor output ------------------------------------------------ */

int compeg_resized_tensor_shape(const compeg_tensor_spec *spec, const compeg_resize_spec *resize, uint32_t width, uint32_t height,
                                const compeg_rect *crop, uint32_t *pre_width, uint32_t *pre_height, size_t *bytes_per_image)
{
    return guarded([&] {
        size_t elem = 0;
        int rc = check_tensor_spec(spec, &elem);
        if (rc == COMPEG_OK)
            rc = check_resize_spec(resize);
        compeg_rect r{};
        if (rc == COMPEG_OK)
            rc = check_crop(crop, width, height, spec->downscale, "", &r);
        if (rc == COMPEG_OK)
            rc = check_antialias_ratio(resize, r, spec->downscale, "");
        if (rc != COMPEG_OK)
            return rc;
        return shape_result(r, spec->downscale, size_t(3) * size_t(resize->out_height) * size_t(resize->out_width) * elem, pre_width, pre_height,
                            bytes_per_image);
    });
}

int compeg_decoder_pack_tensor_resized(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_resize_spec *resize,
                                       const compeg_rect *crop, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return guarded([&] {
        if (!dec)
            return fail(COMPEG_E_INVALID_ARG, null_text(dec));
        size_t elem = 0;
        int rc = check_tensor_spec(spec, &elem);
        if (rc == COMPEG_OK)
            rc = check_resize_spec(resize);
        if (rc == COMPEG_OK)
            rc = check_decoded(*dec);
        if (rc != COMPEG_OK)
            return rc;
        // (the texture never shrinks: the last image's own extent, at the allocation's pitch)
        compeg_rect r{};
        rc = check_crop(crop, dec->last_w, dec->last_h, spec->downscale, "", &r);
        if (rc == COMPEG_OK)
            rc = check_antialias_ratio(resize, r, spec->downscale, "");
        if (rc == COMPEG_OK)
            rc = check_tensor_destination(device_dst, dst_bytes, size_t(3) * size_t(resize->out_height) * size_t(resize->out_width) * elem, elem);
        if (rc != COMPEG_OK)
            return rc;
        Status s = dec->pack_tensor_resized(*spec, *resize, r, device_dst, stream_of(*dec, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_batch_pack_tensor_resized(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_resize_spec *resize,
                                     const compeg_rect *crops, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, null_text(batch));
        size_t elem = 0;
        int rc = check_tensor_spec(spec, &elem);
        if (rc == COMPEG_OK)
            rc = check_resize_spec(resize);
        if (rc == COMPEG_OK)
            rc = check_decoded(*batch);
        if (rc != COMPEG_OK)
            return rc;
        std::vector<compeg_rect> rects(batch->count);
        for (size_t i = 0; i < batch->count; i++) {
            rc = check_crop(crops ? crops + i : nullptr, batch->descs[i].out_w, batch->descs[i].out_h, spec->downscale,
                            "image " + std::to_string(i) + ": ", &rects[i]);
            if (rc == COMPEG_OK)
                rc = check_antialias_ratio(resize, rects[i], spec->downscale, "image " + std::to_string(i) + ": ");
            if (rc != COMPEG_OK)
                return rc;
        }
        rc = check_tensor_destination(device_dst, dst_bytes, size_t(3) * size_t(resize->out_height) * size_t(resize->out_width) * elem * batch->count, elem);
        if (rc != COMPEG_OK)
            return rc;
        Status s = batch->pack_tensor_resized(*spec, *resize, rects.data(), device_dst, stream_of(*batch, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

/* ---- Region tensor output -------------------------------------------------- */

int compeg_region_fit(uint32_t src_width, uint32_t src_height, uint32_t out_width, uint32_t out_height, unsigned align, compeg_rect *dst)
{
    return guarded([&] {
        if (!dst)
            return fail(COMPEG_E_INVALID_ARG, "dst is NULL");
        if (src_width == 0u || src_height == 0u)
            return fail(COMPEG_E_INVALID_ARG, ("region fit: a source extent of " + std::to_string(src_width) + "x" + std::to_string(src_height) +
                                               " has a side of 0").c_str());
        if (out_width == 0u || out_height == 0u || out_width > 65535u || out_height > 65535u)
            return fail(COMPEG_E_INVALID_ARG, ("region fit: output size " + std::to_string(out_width) + "x" + std::to_string(out_height) +
                                               " is not within 1..65535 both ways").c_str());
        if (align > COMPEG_FIT_TOP_LEFT)
            return fail(COMPEG_E_INVALID_ARG, ("region fit: align " + std::to_string(align) + " is neither 0 (center) nor 1 (top left)").c_str());
        // (a source side is below 2^32, an output side below 2^16: every product below 2^50)
        const uint64_t sw = src_width, sh = src_height, ow = out_width, oh = out_height;
        uint64_t dw, dh;
        if (ow * sh <= oh * sw) {
            dw = ow;
            dh = (2u * sh * ow + sw) / (2u * sw);
            dh = dh < 1u ? 1u : (dh > oh ? oh : dh);
        } else {
            dh = oh;
            dw = (2u * sw * oh + sh) / (2u * sh);
            dw = dw < 1u ? 1u : (dw > ow ? ow : dw);
        }
        const bool center = align == COMPEG_FIT_CENTER;
        *dst = compeg_rect{center ? uint32_t((ow - dw) / 2u) : 0u, center ? uint32_t((oh - dh) / 2u) : 0u, uint32_t(dw), uint32_t(dh)};
        return ok();
    });
}

int compeg_region_tensor_shape(const compeg_tensor_spec *spec, const compeg_resize_spec *resize, uint32_t width, uint32_t height,
                               const compeg_region *region, uint32_t *pre_width, uint32_t *pre_height, size_t *bytes_per_slot)
{
    return slot_tensor_shape(RegionPack{spec, resize}, region, width, height, pre_width, pre_height, bytes_per_slot);
}

int compeg_decoder_pack_tensor_regions(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_resize_spec *resize,
                                       const compeg_region *regions, size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                       void *hip_stream)
{
    return pack_slot_tensor(dec, RegionPack{spec, resize}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

int compeg_batch_pack_tensor_regions(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_resize_spec *resize,
                                     const compeg_region *regions, size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                     void *hip_stream)
{
    return pack_slot_tensor(batch, RegionPack{spec, resize}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

/* ---- Filtered tensor output ------------------------------------------------ */

int compeg_filtered_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width, uint32_t height,
                                 const compeg_region *region, uint32_t *pre_width, uint32_t *pre_height, size_t *bytes_per_slot)
{
    return slot_tensor_shape(FilterPack{spec, filter}, region, width, height, pre_width, pre_height, bytes_per_slot);
}

int compeg_decoder_pack_tensor_filtered(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                        const compeg_region *regions, size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                        void *hip_stream)
{
    return pack_slot_tensor(dec, FilterPack{spec, filter}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

int compeg_batch_pack_tensor_filtered(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                      const compeg_region *regions, size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                      void *hip_stream)
{
    return pack_slot_tensor(batch, FilterPack{spec, filter}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

/* ---- Oriented tensor output ------------------------------------------------ */

uint32_t compeg_image_orientation(const compeg_image *img)
{
    return img ? img->data->orientation : 1u;
}

int compeg_batch_image_orientation(const compeg_batch *batch, size_t index, uint32_t *out)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        if (!out)
            return fail(COMPEG_E_INVALID_ARG, "out is NULL");
        if (index >= batch->count || index >= batch->orientations.size())
            return fail(COMPEG_E_INVALID_ARG, ("orient: image " + std::to_string(index) + " is beyond the batch's " +
                                               std::to_string(batch->count) + " images").c_str());
        *out = batch->orientations[index];
        return ok();
    });
}

int compeg_orient_rect(uint32_t upright_width, uint32_t upright_height, uint32_t orientation, const compeg_rect *upright,
                       compeg_rect *stored)
{
    return guarded([&] {
        if (!upright || !stored)
            return fail(COMPEG_E_INVALID_ARG, "orient: a rectangle pointer is NULL");
        if (orientation < 1u || orientation > 8u)
            return fail(COMPEG_E_INVALID_ARG, ("orient: orientation " + std::to_string(orientation) + " is none of 1 .. 8 (the EXIF values)").c_str());
        compeg_rect r{};
        if (!compeg::orient_rect(upright_width, upright_height, orientation, *upright, r))
            return fail(COMPEG_E_INVALID_ARG, ("orient: rectangle " + std::to_string(upright->width) + "x" + std::to_string(upright->height) + " at (" +
                                               std::to_string(upright->x) + ", " + std::to_string(upright->y) + ") leaves the " +
                                               std::to_string(upright_width) + "x" + std::to_string(upright_height) + " image").c_str());
        *stored = r;
        return ok();
    });
}

int compeg_oriented_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width, uint32_t height,
                                 const compeg_oriented_region *region, uint32_t *pre_width, uint32_t *pre_height, size_t *bytes_per_slot)
{
    return slot_tensor_shape(OrientPack{spec, filter, false, nullptr}, region, width, height, pre_width, pre_height, bytes_per_slot);
}

int compeg_decoder_pack_tensor_oriented(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                        const compeg_oriented_region *regions, size_t count, const float *pad, void *device_dst,
                                        size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(dec, OrientPack{spec, filter, false, nullptr}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

int compeg_batch_pack_tensor_oriented(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                      const compeg_oriented_region *regions, size_t count, const float *pad, void *device_dst,
                                      size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(batch, OrientPack{spec, filter, false, nullptr}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

/* ---- Channels-last tensor output ------------------------------------------- */

int compeg_nhwc_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, const compeg_nhwc_spec *nhwc, uint32_t width,
                             uint32_t height, const compeg_oriented_region *region, uint32_t *pre_width, uint32_t *pre_height,
                             size_t *bytes_per_slot)
{
    return slot_tensor_shape(OrientPack{spec, filter, true, nhwc}, region, width, height, pre_width, pre_height, bytes_per_slot);
}

int compeg_decoder_pack_tensor_nhwc(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                    const compeg_nhwc_spec *nhwc, const compeg_oriented_region *regions, size_t count, const float *pad,
                                    void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(dec, OrientPack{spec, filter, true, nhwc}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

int compeg_batch_pack_tensor_nhwc(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                  const compeg_nhwc_spec *nhwc, const compeg_oriented_region *regions, size_t count, const float *pad,
                                  void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(batch, OrientPack{spec, filter, true, nhwc}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

/* ---- Luma tensor output ---------------------------------------------------- */

int compeg_luma_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, const compeg_luma_spec *luma, uint32_t width,
                             uint32_t height, const compeg_oriented_region *region, uint32_t *pre_width, uint32_t *pre_height,
                             size_t *bytes_per_slot)
{
    return slot_tensor_shape(LumaPack{spec, filter, luma}, region, width, height, pre_width, pre_height, bytes_per_slot);
}

int compeg_decoder_pack_tensor_luma(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                    const compeg_luma_spec *luma, const compeg_oriented_region *regions, size_t count, const float *pad,
                                    void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(dec, LumaPack{spec, filter, luma}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

int compeg_batch_pack_tensor_luma(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                  const compeg_luma_spec *luma, const compeg_oriented_region *regions, size_t count, const float *pad,
                                  void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return pack_slot_tensor(batch, LumaPack{spec, filter, luma}, regions, count, pad, device_dst, dst_bytes, hip_stream);
}

} // extern "C"

/* ---- Planar YCbCr output ---------------------------------------------------- */

namespace {

const char *sampling_name(uint32_t components, uint32_t hs, uint32_t vs)
{
    if (components == 1)
        return "grayscale";
    return hs == 2 && vs == 1 ? "4:2:2" : hs == 1 && vs == 1 ? "4:4:4" : hs == 1 && vs == 2 ? "4:4:0" : hs == 2 && vs == 2 ? "4:2:0" : "unknown";
}

// Decodes into the caller's memory (planes, reduced, cropped), every entry point of every output down one road (decode_to_caller).
// What such a decode is laid out for: a decoder's image, or the one size and sampling all images of a batch share.
struct DecodeFacts {
    uint32_t width, height, components, hs, vs; // (hs x vs: the file's luma sampling factors)
    size_t images;
};

// ... of the decoder's image: 0 with *f filled in, or the error recorded
int decode_facts(compeg_decoder *dec, const compeg_image *img, const char *, const void *, DecodeFacts *f)
{
    if (!dec || !img)
        return fail(COMPEG_E_INVALID_ARG, "NULL argument");
    const ImageData &data = *img->data;
    *f = DecodeFacts{data.width, data.height, data.components, data.metadata.components[0].hsample, data.metadata.components[0].vsample, 1};
    return COMPEG_OK;
}

// ... of the batch's finished upload, whose images must be of one size and one sampling (prefix: the output's name)
int decode_facts(compeg_batch *batch, const compeg_image *, const char *prefix, const void *spec, DecodeFacts *f)
{
    if (!batch)
        return fail(COMPEG_E_INVALID_ARG, null_text(batch));
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    const Status s = batch->finish_upload(); // (the descriptors looked at below are the finished upload's)
    if (!s.ok())
        return fail(s);
    const std::string name = prefix;
    if (batch->count == 0)
        return fail(COMPEG_E_INVALID_ARG, (name + ": nothing uploaded yet").c_str());
    const ImageDesc &first = batch->descs[0];
    const uint32_t comps0 = first.dus_per_mcu == 1 ? 1u : 3u;
    for (size_t i = 1; i < batch->count; i++) {
        const ImageDesc &d = batch->descs[i];
        if (d.out_w != first.out_w || d.out_h != first.out_h)
            return fail(COMPEG_E_INVALID_ARG, (name + ": the batch's images are not all of one size (image " + std::to_string(i) + " is " +
                                               std::to_string(d.out_w) + "x" + std::to_string(d.out_h) + ", image 0 " + std::to_string(first.out_w) + "x" +
                                               std::to_string(first.out_h) + ")").c_str());
        const uint32_t comps = d.dus_per_mcu == 1 ? 1u : 3u;
        if (comps != comps0 || d.hsample[0] != first.hsample[0] || d.vsample[0] != first.vsample[0])
            return fail(COMPEG_E_INVALID_ARG, (name + ": the batch's images are not all of one sampling (image " + std::to_string(i) + " is " +
                                               sampling_name(comps, d.hsample[0], d.vsample[0]) + ", image 0 " +
                                               sampling_name(comps0, first.hsample[0], first.vsample[0]) + ")").c_str());
    }
    *f = DecodeFacts{first.out_w, first.out_h, comps0, first.hsample[0], first.vsample[0], batch->count};
    return COMPEG_OK;
}

// The destination holds `images` images of `total` bytes.
int check_destination(const char *prefix, const void *device_dst, size_t dst_bytes, uint64_t total, size_t images)
{
    if (!device_dst)
        return fail(COMPEG_E_INVALID_ARG, "device_dst is NULL");
    if (uint64_t(dst_bytes) / total < images)
        return fail(COMPEG_E_INVALID_ARG, (std::string(prefix) + ": dst_bytes is " + std::to_string(dst_bytes) + ", " + std::to_string(images) +
                                           " image(s) of " + std::to_string(total) + " bytes need " + std::to_string(total * images)).c_str());
    return COMPEG_OK;
}

// (luma sampling as the kernels take it: 1 x 0 for a grayscale image)
Status decode_into(compeg_decoder &dec, const compeg_image *img, const CallerDecode &into, const DecodeFacts &, hipStream_t stream)
{
    return dec.enqueue(*img->data, stream, nullptr, false, &into);
}
Status decode_into(compeg_batch &batch, const compeg_image *, const CallerDecode &into, const DecodeFacts &f, hipStream_t stream)
{
    return batch.decode_into(into, f.hs, f.components == 1 ? 0u : f.vs, stream);
}

// Output: the spec with what is its own -- the target laid out for the facts and the destination checked against it
// (target_for: 0, or the error recorded), and the runtime's description of the decode.  img: the decoder's.
// blocking: (decoders, hip_stream NULL: the gpu's own stream) the call waits for the stream.
template <class Owner, class Output>
int decode_to_caller(Owner *owner, const compeg_image *img, const Output &output, void *device_dst, size_t dst_bytes, void *hip_stream,
                     bool blocking = false)
{
    return guarded([&] {
        DecodeFacts facts;
        typename Output::Target target;
        int rc = decode_facts(owner, img, Output::kPrefix, output.spec, &facts);
        if (rc == COMPEG_OK)
            rc = output.target_for(facts, device_dst, dst_bytes, &target);
        if (rc != COMPEG_OK)
            return rc;
        const hipStream_t stream = stream_of(*owner, hip_stream);
        const Status s = decode_into(*owner, img, Output::decode(target), facts, stream);
        if (!s.ok())
            return fail(s);
        const hipError_t e = blocking ? hipStreamSynchronize(stream) : hipSuccess;
        return e == hipSuccess ? ok() : fail(hip_status(e, "hipStreamSynchronize"));
    });
}

// compeg_planes_spec as the header has it, laid out for a width x height image: 0 with *out filled in, or the error
// recorded.  (The texts name values, not the header's macros.)
int planes_layout(const compeg_planes_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hs, uint32_t vs,
                  compeg_planes_layout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (!out)
        return fail(COMPEG_E_INVALID_ARG, "layout is NULL");
    if (spec->format > COMPEG_PLANES_UYVY)
        return fail(COMPEG_E_INVALID_ARG, ("planes spec: format " + std::to_string(spec->format) + " is none of 0 (planar), 1 (semiplanar), 2 (yuyv), 3 (uyvy)").c_str());
    if (spec->chroma > COMPEG_CHROMA_420)
        return fail(COMPEG_E_INVALID_ARG, ("planes spec: chroma " + std::to_string(spec->chroma) + " is neither 0 (as coded) nor 1 (4:2:0)").c_str());
    for (int i = 0; i < 4; i++)
        if (spec->reserved[i] != 0u)
            return fail(COMPEG_E_INVALID_ARG, "planes spec: reserved must be 0");
    const bool gray = components == 1;
    if (components != 1 && components != 3)
        return fail(COMPEG_E_INVALID_ARG, ("planes: " + std::to_string(components) + " components, an image has 1 or 3").c_str());
    if (gray ? !(hs == 1 && vs == 1) : !((hs == 1 || hs == 2) && (vs == 1 || vs == 2)))
        return fail(COMPEG_E_INVALID_ARG, ("planes: luma sampling " + std::to_string(hs) + "x" + std::to_string(vs) +
                                           " is none of 2x1, 1x1, 1x2, 2x2 (1x1 for a grayscale image)").c_str());
    if (width == 0 || height == 0)
        return fail(COMPEG_E_INVALID_ARG, "planes: the image has no pixels");
    const bool packed = spec->format >= COMPEG_PLANES_YUYV, is422 = !gray && hs == 2 && vs == 1;
    const bool half = spec->chroma == COMPEG_CHROMA_420;
    if (half && packed)
        return fail(COMPEG_E_INVALID_ARG, "planes spec: chroma 1 (4:2:0) goes with the planar and semiplanar formats only, not with a packed one");
    if (packed && !is422)
        return fail(COMPEG_E_UNSUPPORTED, (std::string("planes: the packed formats yuyv and uyvy take 4:2:2 files only, this one is ") +
                                           sampling_name(components, hs, vs)).c_str());
    if (half && !is422)
        return fail(COMPEG_E_UNSUPPORTED, (std::string("planes: chroma 1 (4:2:0) is made from 4:2:2 files only, this one is ") +
                                           sampling_name(components, hs, vs)).c_str());
    compeg_planes_layout l;
    memset(&l, 0, sizeof l);
    const uint32_t cw = (width + hs - 1) / hs, ch = half ? (height + 1) / 2 : (height + vs - 1) / vs;
    if (packed) {
        l.planes = 1;
        l.width[0] = width;
        l.height[0] = height;
        l.row_bytes[0] = 4u * ((width + 1) / 2);
    } else {
        l.planes = gray ? 1u : (spec->format == COMPEG_PLANES_SEMIPLANAR ? 2u : 3u);
        l.width[0] = width;
        l.height[0] = height;
        l.row_bytes[0] = width;
        for (uint32_t p = 1; p < l.planes; p++) {
            l.width[p] = cw;
            l.height[p] = ch;
            l.row_bytes[p] = l.planes == 2 ? 2u * cw : cw;
        }
    }
    uint64_t at = 0;
    for (uint32_t p = 0; p < l.planes; p++) {
        const uint32_t given = p == 0 ? spec->luma_pitch : spec->chroma_pitch;
        if (given != 0u && given < l.row_bytes[p])
            return fail(COMPEG_E_INVALID_ARG, (std::string("planes spec: ") + (p == 0 ? "luma_pitch " : "chroma_pitch ") + std::to_string(given) +
                                               " is below the row's " + std::to_string(l.row_bytes[p]) + " bytes").c_str());
        l.pitch[p] = given ? given : l.row_bytes[p];
        l.offset[p] = at;
        at += uint64_t(l.pitch[p]) * l.height[p];
    }
    l.total_bytes = at;
    *out = l;
    return COMPEG_OK;
}

PlanesTarget planes_target(const compeg_planes_spec &spec, const compeg_planes_layout &l, void *device_dst)
{
    PlanesTarget t{};
    t.dst = static_cast<uint8_t *>(device_dst);
    t.image_stride = l.total_bytes;
    for (int p = 0; p < 3; p++) {
        t.offset[p] = l.offset[p];
        t.pitch[p] = l.pitch[p];
        t.row_bytes[p] = l.row_bytes[p];
        t.rows[p] = l.height[p];
    }
    t.format = spec.format;
    t.chroma420 = spec.chroma == COMPEG_CHROMA_420 ? 1u : 0u;
    return t;
}

struct PlanesOutput {
    using Target = PlanesTarget;
    static constexpr const char *kPrefix = "planes";
    const compeg_planes_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, PlanesTarget *target) const
    {
        compeg_planes_layout l;
        int rc = planes_layout(spec, f.width, f.height, f.components, f.hs, f.vs, &l);
        if (rc == COMPEG_OK)
            rc = check_destination(kPrefix, device_dst, dst_bytes, l.total_bytes, f.images);
        if (rc == COMPEG_OK)
            *target = planes_target(*spec, l, device_dst);
        return rc;
    }
    static CallerDecode decode(const PlanesTarget &target) { return planes_decode(target); }
};

} // namespace

extern "C" {

int compeg_image_sampling(const compeg_image *img, uint32_t *hsample, uint32_t *vsample)
{
    if (!img)
        return fail(COMPEG_E_INVALID_ARG, "img is NULL");
    if (hsample)
        *hsample = img->data->metadata.components[0].hsample;
    if (vsample)
        *vsample = img->data->metadata.components[0].vsample;
    return ok();
}

int compeg_planes_shape(const compeg_planes_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hsample,
                        uint32_t vsample, compeg_planes_layout *layout)
{
    return guarded([&] {
        const int rc = planes_layout(spec, width, height, components, hsample, vsample, layout);
        return rc == COMPEG_OK ? ok() : rc;
    });
}

int compeg_batch_decode_planes(compeg_batch *batch, const compeg_planes_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(batch, nullptr, PlanesOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_planes(compeg_decoder *dec, const compeg_image *img, const compeg_planes_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(dec, img, PlanesOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_planes_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_planes_spec *spec, void *device_dst,
                                          size_t dst_bytes)
{
    return decode_to_caller(dec, img, PlanesOutput{spec}, device_dst, dst_bytes, nullptr, true);
}

} // extern "C"

/* ---- Reduced-size decode ---------------------------------------------------- */

namespace {

struct ReducedLayout {
    uint32_t ow, oh, pitch;
    uint64_t total;
};

// compeg_reduced_spec as the header has it, laid out for a width x height image: 0 with *out filled in, or the error
// recorded.  (The texts name values, not the header's macros.)
int reduced_layout(const compeg_reduced_spec *spec, uint32_t width, uint32_t height, ReducedLayout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (spec->denominator != 8u)
        return fail(COMPEG_E_INVALID_ARG, ("reduced spec: denominator " + std::to_string(spec->denominator) +
                                           " is not 8: 1/8 is the DC-only decode and the only one built").c_str());
    if (spec->format > COMPEG_REDUCED_RGB_PLANAR)
        return fail(COMPEG_E_INVALID_ARG, ("reduced spec: format " + std::to_string(spec->format) + " is neither 0 (rgba) nor 1 (rgb planar)").c_str());
    if (width == 0 || height == 0)
        return fail(COMPEG_E_INVALID_ARG, "reduced: the image has no pixels");
    ReducedLayout l;
    l.ow = (width - 1u) / 8u + 1u;
    l.oh = (height - 1u) / 8u + 1u;
    if (spec->format == COMPEG_REDUCED_RGB_PLANAR) {
        if (spec->pitch != 0u)
            return fail(COMPEG_E_INVALID_ARG, ("reduced spec: pitch " + std::to_string(spec->pitch) + " with the planar format, whose rows are tight (pitch 0)").c_str());
        l.pitch = l.ow;
        l.total = 3ull * l.ow * l.oh;
    } else {
        const uint64_t row = 4ull * l.ow;
        if (spec->pitch != 0u && (spec->pitch < row || spec->pitch % 4u != 0u))
            return fail(COMPEG_E_INVALID_ARG, ("reduced spec: pitch " + std::to_string(spec->pitch) + " is not a multiple of 4 at or above the row's " +
                                               std::to_string(row) + " bytes").c_str());
        l.pitch = spec->pitch ? spec->pitch : uint32_t(row);
        l.total = uint64_t(l.pitch) * l.oh;
    }
    *out = l;
    return COMPEG_OK;
}

ReducedTarget reduced_target(const compeg_reduced_spec &spec, const ReducedLayout &l, void *device_dst)
{
    ReducedTarget t{};
    t.dst = static_cast<uint8_t *>(device_dst);
    t.image_stride = l.total;
    t.ow = l.ow;
    t.oh = l.oh;
    t.pitch = l.pitch;
    t.format = spec.format;
    return t;
}

struct ReducedOutput {
    using Target = ReducedTarget;
    static constexpr const char *kPrefix = "reduced";
    const compeg_reduced_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, ReducedTarget *target) const
    {
        ReducedLayout l;
        int rc = reduced_layout(spec, f.width, f.height, &l);
        if (rc == COMPEG_OK && spec->format == COMPEG_REDUCED_RGBA && reinterpret_cast<uintptr_t>(device_dst) % 4u != 0u)
            rc = fail(COMPEG_E_INVALID_ARG, "reduced: the rgba destination's address is not a multiple of 4");
        if (rc == COMPEG_OK)
            rc = check_destination(kPrefix, device_dst, dst_bytes, l.total, f.images);
        if (rc == COMPEG_OK)
            *target = reduced_target(*spec, l, device_dst);
        return rc;
    }
    static CallerDecode decode(const ReducedTarget &target) { return reduced_decode(target); }
};

} // namespace

extern "C" {

int compeg_reduced_shape(const compeg_reduced_spec *spec, uint32_t width, uint32_t height, uint32_t *out_width, uint32_t *out_height,
                         uint32_t *pitch, uint64_t *total_bytes)
{
    return guarded([&] {
        ReducedLayout l;
        const int rc = reduced_layout(spec, width, height, &l);
        if (rc != COMPEG_OK)
            return rc;
        if (out_width)
            *out_width = l.ow;
        if (out_height)
            *out_height = l.oh;
        if (pitch)
            *pitch = l.pitch;
        if (total_bytes)
            *total_bytes = l.total;
        return ok();
    });
}

int compeg_batch_decode_reduced(compeg_batch *batch, const compeg_reduced_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(batch, nullptr, ReducedOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_reduced(compeg_decoder *dec, const compeg_image *img, const compeg_reduced_spec *spec, void *device_dst,
                                  size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(dec, img, ReducedOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_reduced_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_reduced_spec *spec, void *device_dst,
                                           size_t dst_bytes)
{
    return decode_to_caller(dec, img, ReducedOutput{spec}, device_dst, dst_bytes, nullptr, true);
}

} // extern "C"

/* ---- Scaled decode ---------------------------------------------------------- */

namespace {

// compeg_scaled_spec as the header has it, laid out for a width x height image: 0 with *out filled in, or the error
// recorded.  (The texts name values, not the header's macros.)
int scaled_layout(const compeg_scaled_spec *spec, uint32_t width, uint32_t height, ReducedLayout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    const uint32_t den = spec->denominator;
    if (den != 2u && den != 4u && den != 8u)
        return fail(COMPEG_E_INVALID_ARG, ("scaled spec: denominator " + std::to_string(den) + " is none of 2, 4, 8: 1/2, 1/4 and 1/8 are the scales built").c_str());
    if (spec->format > COMPEG_SCALED_RGB_PLANAR)
        return fail(COMPEG_E_INVALID_ARG, ("scaled spec: format " + std::to_string(spec->format) + " is neither 0 (rgba) nor 1 (rgb planar)").c_str());
    if (width == 0 || height == 0)
        return fail(COMPEG_E_INVALID_ARG, "scaled: the image has no pixels");
    ReducedLayout l;
    l.ow = (width - 1u) / den + 1u;
    l.oh = (height - 1u) / den + 1u;
    if (spec->format == COMPEG_SCALED_RGB_PLANAR) {
        if (spec->pitch != 0u)
            return fail(COMPEG_E_INVALID_ARG, ("scaled spec: pitch " + std::to_string(spec->pitch) + " with the planar format, whose rows are tight (pitch 0)").c_str());
        l.pitch = l.ow;
        l.total = 3ull * l.ow * l.oh;
    } else {
        const uint64_t row = 4ull * l.ow;
        if (spec->pitch != 0u && (spec->pitch < row || spec->pitch % 4u != 0u))
            return fail(COMPEG_E_INVALID_ARG, ("scaled spec: pitch " + std::to_string(spec->pitch) + " is not a multiple of 4 at or above the row's " +
                                               std::to_string(row) + " bytes").c_str());
        l.pitch = spec->pitch ? spec->pitch : uint32_t(row);
        l.total = uint64_t(l.pitch) * l.oh;
    }
    *out = l;
    return COMPEG_OK;
}

// The layout and the destination's checks, shared by both outputs below.
int scaled_destination(const compeg_scaled_spec *spec, const DecodeFacts &f, void *device_dst, size_t dst_bytes, ReducedLayout *l)
{
    int rc = scaled_layout(spec, f.width, f.height, l);
    if (rc == COMPEG_OK && spec->format == COMPEG_SCALED_RGBA && reinterpret_cast<uintptr_t>(device_dst) % 4u != 0u)
        rc = fail(COMPEG_E_INVALID_ARG, "scaled: the rgba destination's address is not a multiple of 4");
    if (rc == COMPEG_OK)
        rc = check_destination("scaled", device_dst, dst_bytes, l->total, f.images);
    return rc;
}

// Denominators 2 and 4: the scaled kernels.
struct ScaledOutput {
    using Target = ScaledTarget;
    static constexpr const char *kPrefix = "scaled";
    const compeg_scaled_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, ScaledTarget *target) const
    {
        ReducedLayout l;
        const int rc = scaled_destination(spec, f, device_dst, dst_bytes, &l);
        if (rc == COMPEG_OK) {
            ScaledTarget t{};
            t.dst = static_cast<uint8_t *>(device_dst);
            t.image_stride = l.total;
            t.ow = l.ow;
            t.oh = l.oh;
            t.pitch = l.pitch;
            t.format = spec->format;
            t.n = 8u / spec->denominator;
            *target = t;
        }
        return rc;
    }
    static CallerDecode decode(const ScaledTarget &target) { return scaled_decode(target); }
};

// Denominator 8: the scaled spec's checks and words in front of the reduced decode's kernels (the formats' values are
// the same in both specs).
struct ScaledEighthOutput {
    using Target = ReducedTarget;
    static constexpr const char *kPrefix = "scaled";
    const compeg_scaled_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, ReducedTarget *target) const
    {
        ReducedLayout l;
        const int rc = scaled_destination(spec, f, device_dst, dst_bytes, &l);
        if (rc == COMPEG_OK)
            *target = reduced_target(compeg_reduced_spec{8u, spec->format, spec->pitch}, l, device_dst);
        return rc;
    }
    static CallerDecode decode(const ReducedTarget &target) { return reduced_decode(target); }
};
static_assert(COMPEG_SCALED_RGBA == COMPEG_REDUCED_RGBA && COMPEG_SCALED_RGB_PLANAR == COMPEG_REDUCED_RGB_PLANAR, "one numbering of the formats");

template <class Owner>
int decode_scaled(Owner *owner, const compeg_image *img, const compeg_scaled_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream,
                  bool blocking = false)
{
    if (spec && spec->denominator == 8u)
        return decode_to_caller(owner, img, ScaledEighthOutput{spec}, device_dst, dst_bytes, hip_stream, blocking);
    return decode_to_caller(owner, img, ScaledOutput{spec}, device_dst, dst_bytes, hip_stream, blocking);
}

} // namespace

extern "C" {

int compeg_scaled_shape(const compeg_scaled_spec *spec, uint32_t width, uint32_t height, uint32_t *out_width, uint32_t *out_height,
                        uint32_t *pitch, uint64_t *total_bytes)
{
    return guarded([&] {
        ReducedLayout l;
        const int rc = scaled_layout(spec, width, height, &l);
        if (rc != COMPEG_OK)
            return rc;
        if (out_width)
            *out_width = l.ow;
        if (out_height)
            *out_height = l.oh;
        if (pitch)
            *pitch = l.pitch;
        if (total_bytes)
            *total_bytes = l.total;
        return ok();
    });
}

int compeg_batch_decode_scaled(compeg_batch *batch, const compeg_scaled_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decode_scaled(batch, nullptr, spec, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_scaled(compeg_decoder *dec, const compeg_image *img, const compeg_scaled_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream)
{
    return decode_scaled(dec, img, spec, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_scaled_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_scaled_spec *spec, void *device_dst,
                                          size_t dst_bytes)
{
    return decode_scaled(dec, img, spec, device_dst, dst_bytes, nullptr, true);
}

} // extern "C"

/* ---- Levels decode ---------------------------------------------------------- */

namespace {

// natural (row-major) index -> zig-zag position: the table of kernels_body.h's zigzag_of
constexpr uint8_t kZigzagOf[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                   10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// compeg_levels_spec as the header has it, laid out for a width x height image: 0 with *out filled in, or the error
// recorded.  (The texts name values, not the header's macros.)
int levels_layout(const compeg_levels_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hs, uint32_t vs,
                  compeg_levels_layout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (!out)
        return fail(COMPEG_E_INVALID_ARG, "layout is NULL");
    if (spec->order > COMPEG_LEVELS_NATURAL)
        return fail(COMPEG_E_INVALID_ARG, ("levels spec: order " + std::to_string(spec->order) + " is neither 0 (zigzag) nor 1 (natural)").c_str());
    for (int i = 0; i < 3; i++)
        if (spec->reserved[i] != 0u)
            return fail(COMPEG_E_INVALID_ARG, "levels spec: reserved must be 0");
    const bool gray = components == 1;
    if (components != 1 && components != 3)
        return fail(COMPEG_E_INVALID_ARG, ("levels: " + std::to_string(components) + " components, an image has 1 or 3").c_str());
    if (gray ? !(hs == 1 && vs == 1) : !((hs == 1 || hs == 2) && (vs == 1 || vs == 2)))
        return fail(COMPEG_E_INVALID_ARG, ("levels: luma sampling " + std::to_string(hs) + "x" + std::to_string(vs) +
                                           " is none of 2x1, 1x1, 1x2, 2x2 (1x1 for a grayscale image)").c_str());
    if (width == 0 || height == 0)
        return fail(COMPEG_E_INVALID_ARG, "levels: the image has no pixels");
    compeg_levels_layout l;
    memset(&l, 0, sizeof l);
    l.components = components;
    const uint32_t width_mcus = (width - 1u) / (8u * hs) + 1u, height_mcus = (height - 1u) / (8u * vs) + 1u;
    uint64_t at = 0;
    for (uint32_t c = 0; c < components; c++) {
        const uint32_t hc = c == 0 ? hs : 1u, vc = c == 0 ? vs : 1u;
        l.blocks_w[c] = width_mcus * hc;
        l.blocks_h[c] = height_mcus * vc;
        // (the component's extent in samples: ceil(W hs_c / hs_0) x ceil(H vs_c / vs_0))
        const uint32_t cw = (width - 1u) / (hs / hc) + 1u, ch = (height - 1u) / (vs / vc) + 1u;
        l.width_in_blocks[c] = (cw - 1u) / 8u + 1u;
        l.height_in_blocks[c] = (ch - 1u) / 8u + 1u;
        l.offset[c] = at;
        const uint64_t blocks = uint64_t(l.blocks_w[c]) * l.blocks_h[c];
        if (blocks > (UINT64_MAX / 4u - at) / 128u)
            return fail(COMPEG_E_INVALID_ARG, ("levels: the blocks of a " + std::to_string(width) + "x" + std::to_string(height) +
                                               " image overflow the layout's 64-bit byte counts").c_str());
        at += blocks * 128u;
    }
    l.total_bytes = at;
    *out = l;
    return COMPEG_OK;
}

struct LevelsOutput {
    using Target = LevelsTarget;
    static constexpr const char *kPrefix = "levels";
    const compeg_levels_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, LevelsTarget *target) const
    {
        compeg_levels_layout l;
        int rc = levels_layout(spec, f.width, f.height, f.components, f.hs, f.vs, &l);
        if (rc == COMPEG_OK && reinterpret_cast<uintptr_t>(device_dst) % 16u != 0u)
            rc = fail(COMPEG_E_INVALID_ARG, "levels: the destination's address is not a multiple of 16");
        if (rc == COMPEG_OK)
            rc = check_destination(kPrefix, device_dst, dst_bytes, l.total_bytes, f.images);
        if (rc == COMPEG_OK) {
            LevelsTarget t{};
            t.dst = static_cast<uint8_t *>(device_dst);
            t.image_stride = l.total_bytes;
            for (int c = 0; c < 3; c++) {
                t.offset[c] = l.offset[c];
                t.blocks_w[c] = l.blocks_w[c];
                t.blocks_h[c] = l.blocks_h[c];
            }
            t.order = spec->order;
            *target = t;
        }
        return rc;
    }
    static CallerDecode decode(const LevelsTarget &target) { return levels_decode(target); }
};
static_assert(COMPEG_LEVELS_ZIGZAG == kLevelsZigzag && COMPEG_LEVELS_NATURAL == kLevelsNatural, "one numbering of the orders");

// 64 factors in zig-zag order -> out, in `order`
int quant_table_out(const uint16_t *zigzag, uint32_t components, uint32_t component, uint16_t *out, uint32_t order)
{
    if (!out)
        return fail(COMPEG_E_INVALID_ARG, "out is NULL");
    if (order > COMPEG_LEVELS_NATURAL)
        return fail(COMPEG_E_INVALID_ARG, ("quant table: order " + std::to_string(order) + " is neither 0 (zigzag) nor 1 (natural)").c_str());
    if (component >= components)
        return fail(COMPEG_E_INVALID_ARG, ("quant table: component " + std::to_string(component) + " of an image that has " +
                                           std::to_string(components)).c_str());
    for (int i = 0; i < 64; i++)
        out[i] = zigzag[order == COMPEG_LEVELS_NATURAL ? kZigzagOf[i] : i];
    return ok();
}

} // namespace

extern "C" {

int compeg_levels_shape(const compeg_levels_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hsample,
                        uint32_t vsample, compeg_levels_layout *layout)
{
    return guarded([&] {
        const int rc = levels_layout(spec, width, height, components, hsample, vsample, layout);
        return rc == COMPEG_OK ? ok() : rc;
    });
}

int compeg_batch_decode_levels(compeg_batch *batch, const compeg_levels_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(batch, nullptr, LevelsOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_levels(compeg_decoder *dec, const compeg_image *img, const compeg_levels_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(dec, img, LevelsOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_levels_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_levels_spec *spec, void *device_dst,
                                          size_t dst_bytes)
{
    return decode_to_caller(dec, img, LevelsOutput{spec}, device_dst, dst_bytes, nullptr, true);
}

int compeg_image_quant_table(const compeg_image *img, uint32_t component, uint16_t out[64], uint32_t order)
{
    return guarded([&] {
        if (!img)
            return fail(COMPEG_E_INVALID_ARG, "img is NULL");
        const ImageData &data = *img->data;
        uint16_t q[64] = {0};
        if (component < data.components)
            for (int z = 0; z < 64; z++)
                q[z] = uint16_t(data.metadata.qtables[data.metadata.components[component].qtable & 3][z]);
        return quant_table_out(q, data.components, component, out, order);
    });
}

int compeg_batch_quant_table(const compeg_batch *batch, size_t index, uint32_t component, uint16_t out[64], uint32_t order)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, "batch is NULL");
        if (index >= batch->count || index >= batch->quant_tables.size())
            return fail(COMPEG_E_INVALID_ARG, ("quant table: image " + std::to_string(index) + " is beyond the batch's " +
                                               std::to_string(batch->count) + " images").c_str());
        const compeg_batch::QuantTables &t = batch->quant_tables[index];
        return quant_table_out(t.q[component < 3u ? component : 0u], t.components, component, out, order);
    });
}

} // extern "C"

/* ---- Cropped decode --------------------------------------------------------- */

namespace {

struct CropLayout {
    uint32_t pitch;
    uint64_t total;
};

// compeg_crop_spec as the header has it, laid out against a width x height image: 0 with *out filled in, or the error
// recorded.  (The texts name values, not the header's macros.)
int crop_layout(const compeg_crop_spec *spec, uint32_t width, uint32_t height, CropLayout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (spec->format > COMPEG_CROP_RGB_PLANAR)
        return fail(COMPEG_E_INVALID_ARG, ("crop spec: format " + std::to_string(spec->format) + " is neither 0 (rgba) nor 1 (rgb planar)").c_str());
    if (spec->reserved[0] != 0u || spec->reserved[1] != 0u)
        return fail(COMPEG_E_INVALID_ARG, ("crop spec: reserved is " + std::to_string(spec->reserved[0]) + ", " + std::to_string(spec->reserved[1]) +
                                           ", it must be 0").c_str());
    if (width == 0 || height == 0)
        return fail(COMPEG_E_INVALID_ARG, "crop: the image has no pixels");
    const std::string rect = std::to_string(spec->width) + "x" + std::to_string(spec->height) + " at (" + std::to_string(spec->x) + ", " +
                             std::to_string(spec->y) + ")";
    if (spec->width == 0 || spec->height == 0)
        return fail(COMPEG_E_INVALID_ARG, ("crop spec: the rectangle " + rect + " is empty").c_str());
    if (uint64_t(spec->x) + spec->width > width || uint64_t(spec->y) + spec->height > height)
        return fail(COMPEG_E_INVALID_ARG, ("crop spec: the rectangle " + rect + " reaches beyond the image's " + std::to_string(width) + "x" +
                                           std::to_string(height)).c_str());
    CropLayout l;
    if (spec->format == COMPEG_CROP_RGB_PLANAR) {
        if (spec->pitch != 0u)
            return fail(COMPEG_E_INVALID_ARG, ("crop spec: pitch " + std::to_string(spec->pitch) + " with the planar format, whose rows are tight (pitch 0)").c_str());
        l.pitch = spec->width;
        l.total = 3ull * spec->width * spec->height;
    } else {
        const uint64_t row = 4ull * spec->width;
        if (spec->pitch != 0u && (spec->pitch < row || spec->pitch % 4u != 0u))
            return fail(COMPEG_E_INVALID_ARG, ("crop spec: pitch " + std::to_string(spec->pitch) + " is not a multiple of 4 at or above the row's " +
                                               std::to_string(row) + " bytes").c_str());
        l.pitch = spec->pitch ? spec->pitch : uint32_t(row);
        l.total = uint64_t(l.pitch) * spec->height;
    }
    *out = l;
    return COMPEG_OK;
}

// (mcu_w x mcu_h: the image's MCU in pixels.)  The rectangle in MCUs, once for the launch: the kernels' touch test and
// their per-MCU test read it.
CropTarget crop_target(const compeg_crop_spec &spec, const CropLayout &l, uint32_t mcu_w, uint32_t mcu_h, void *device_dst)
{
    CropTarget t{};
    t.dst = static_cast<uint8_t *>(device_dst);
    t.image_stride = l.total;
    t.x = spec.x;
    t.y = spec.y;
    t.width = spec.width;
    t.height = spec.height;
    t.pitch = l.pitch;
    t.format = spec.format;
    t.mx0 = spec.x / mcu_w;
    t.mx1 = (spec.x + spec.width - 1u) / mcu_w + 1u;
    t.my0 = spec.y / mcu_h;
    t.my1 = (spec.y + spec.height - 1u) / mcu_h + 1u;
    return t;
}

struct CroppedOutput {
    using Target = CropTarget;
    static constexpr const char *kPrefix = "crop";
    const compeg_crop_spec *spec;
    int target_for(const DecodeFacts &f, void *device_dst, size_t dst_bytes, CropTarget *target) const
    {
        CropLayout l;
        int rc = crop_layout(spec, f.width, f.height, &l);
        if (rc == COMPEG_OK && spec->format == COMPEG_CROP_RGBA && reinterpret_cast<uintptr_t>(device_dst) % 4u != 0u)
            rc = fail(COMPEG_E_INVALID_ARG, "crop: the rgba destination's address is not a multiple of 4");
        if (rc == COMPEG_OK)
            rc = check_destination(kPrefix, device_dst, dst_bytes, l.total, f.images);
        if (rc == COMPEG_OK) {
            const bool gray = f.components == 1;
            *target = crop_target(*spec, l, 8u * (gray ? 1u : f.hs), 8u * (gray ? 1u : f.vs), device_dst);
        }
        return rc;
    }
    static CallerDecode decode(const CropTarget &target) { return cropped_decode(target); }
};

} // namespace

extern "C" {

int compeg_crop_shape(const compeg_crop_spec *spec, uint32_t image_width, uint32_t image_height, uint32_t *pitch, uint64_t *total_bytes)
{
    return guarded([&] {
        CropLayout l;
        const int rc = crop_layout(spec, image_width, image_height, &l);
        if (rc != COMPEG_OK)
            return rc;
        if (pitch)
            *pitch = l.pitch;
        if (total_bytes)
            *total_bytes = l.total;
        return ok();
    });
}

int compeg_batch_decode_cropped(compeg_batch *batch, const compeg_crop_spec *spec, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(batch, nullptr, CroppedOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_cropped(compeg_decoder *dec, const compeg_image *img, const compeg_crop_spec *spec, void *device_dst,
                                  size_t dst_bytes, void *hip_stream)
{
    return decode_to_caller(dec, img, CroppedOutput{spec}, device_dst, dst_bytes, hip_stream);
}

int compeg_decoder_decode_cropped_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_crop_spec *spec, void *device_dst,
                                           size_t dst_bytes)
{
    return decode_to_caller(dec, img, CroppedOutput{spec}, device_dst, dst_bytes, nullptr, true);
}

} // extern "C"

/* ---- Cropped decode of a region list ------------------------------------------ */

namespace {

struct CropSlotLayout {
    uint32_t pitch;
    uint64_t slot_bytes;
};

// compeg_crop_regions_spec as the header has it: 0 with *out filled in, or the error recorded.
int crop_regions_layout(const compeg_crop_regions_spec *spec, CropSlotLayout *out)
{
    if (!spec)
        return fail(COMPEG_E_INVALID_ARG, "spec is NULL");
    if (spec->format > COMPEG_CROP_RGB_PLANAR)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: format " + std::to_string(spec->format) + " is neither 0 (rgba) nor 1 (rgb planar)").c_str());
    for (int i = 0; i < 4; i++)
        if (spec->reserved[i] != 0u)
            return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: reserved[" + std::to_string(i) + "] is " + std::to_string(spec->reserved[i]) +
                                               ", it must be 0").c_str());
    const std::string slot = std::to_string(spec->slot_width) + "x" + std::to_string(spec->slot_height);
    if (spec->slot_width == 0 || spec->slot_height == 0)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: the slot " + slot + " has no pixels").c_str());
    // (an image has at most 65535 pixels a side and a region lies inside its slot: nothing is lost, and no product below overflows)
    if (spec->slot_width > 65535u || spec->slot_height > 65535u)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: the slot " + slot + " is beyond 65535 pixels a side, which no image has").c_str());
    CropSlotLayout l;
    if (spec->format == COMPEG_CROP_RGB_PLANAR) {
        if (spec->pitch != 0u)
            return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: pitch " + std::to_string(spec->pitch) + " with the planar format, whose rows are tight (pitch 0)").c_str());
        l.pitch = spec->slot_width;
        l.slot_bytes = 3ull * spec->slot_width * spec->slot_height;
    } else {
        const uint32_t row = 4u * spec->slot_width;
        if (spec->pitch != 0u && (spec->pitch < row || spec->pitch % 4u != 0u))
            return fail(COMPEG_E_INVALID_ARG, ("crop regions spec: pitch " + std::to_string(spec->pitch) + " is not a multiple of 4 at or above the slot row's " +
                                               std::to_string(row) + " bytes").c_str());
        l.pitch = spec->pitch ? spec->pitch : row;
        l.slot_bytes = uint64_t(l.pitch) * spec->slot_height;
    }
    *out = l;
    return COMPEG_OK;
}

// One region against its width x height image and the (checked) spec's slot; which: "region 3: " or "".
int crop_region_fits(const compeg_crop_regions_spec &spec, uint32_t width, uint32_t height, const compeg_crop_region &r, const std::string &which)
{
    const std::string rect = std::to_string(r.width) + "x" + std::to_string(r.height) + " at (" + std::to_string(r.x) + ", " + std::to_string(r.y) + ")";
    if (r.reserved != 0u)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions: " + which + "reserved is " + std::to_string(r.reserved) + ", it must be 0").c_str());
    if (r.width == 0 || r.height == 0)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions: " + which + "the rectangle " + rect + " is empty").c_str());
    if (uint64_t(r.x) + r.width > width || uint64_t(r.y) + r.height > height)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions: " + which + "the rectangle " + rect + " reaches beyond image " + std::to_string(r.image) + "'s " +
                                           std::to_string(width) + "x" + std::to_string(height)).c_str());
    if (uint64_t(r.dst_x) + r.width > spec.slot_width || uint64_t(r.dst_y) + r.height > spec.slot_height)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions: " + which + "the rectangle " + rect + " placed at (" + std::to_string(r.dst_x) + ", " +
                                           std::to_string(r.dst_y) + ") reaches beyond the slot's " + std::to_string(spec.slot_width) + "x" +
                                           std::to_string(spec.slot_height)).c_str());
    return COMPEG_OK;
}

// What the checks and the records need of an image: its extent, its luma sampling as the kernels take it (1 x 0: a
// grayscale image) and its restart intervals.
struct RegionImage {
    uint32_t width, height, hs, vs, intervals;
};
RegionImage region_image(const ImageDesc &d)
{
    const bool gray = d.dus_per_mcu == 1;
    return RegionImage{d.out_w, d.out_h, gray ? 1u : d.hsample[0], gray ? 0u : d.vsample[0], d.total_intervals};
}
RegionImage region_image(const ImageData &data)
{
    const bool gray = data.components == 1;
    return RegionImage{data.width, data.height, gray ? 1u : data.metadata.components[0].hsample, gray ? 0u : data.metadata.components[0].vsample,
                       data.metadata.total_restart_intervals};
}

// The whole validation, once for both owners: 0 with *call made -- the records grouped by their image's sampling, a
// stable grouping, each with its own place in the destination -- or the error recorded.  images: the upload's count;
// image_of(i): image i.  Nothing of the caller's is kept: the records are copies.
template <class ImageOf>
int crop_regions_call(const compeg_crop_regions_spec *spec, const compeg_crop_region *regions, size_t count, size_t images, const ImageOf &image_of,
                      void *device_dst, size_t dst_bytes, CropRegionsCall *call)
{
    CropSlotLayout l;
    int rc = crop_regions_layout(spec, &l);
    if (rc != COMPEG_OK)
        return rc;
    if (!device_dst)
        return fail(COMPEG_E_INVALID_ARG, "device_dst is NULL");
    if (count != 0 && !regions)
        return fail(COMPEG_E_INVALID_ARG, "regions is NULL");
    if (spec->format == COMPEG_CROP_RGBA && reinterpret_cast<uintptr_t>(device_dst) % 4u != 0u)
        return fail(COMPEG_E_INVALID_ARG, "crop regions: the rgba destination's address is not a multiple of 4");
    if (uint64_t(dst_bytes) / l.slot_bytes < count)
        return fail(COMPEG_E_INVALID_ARG, ("crop regions: dst_bytes is " + std::to_string(dst_bytes) + ", " + std::to_string(count) + " slot(s) of " +
                                           std::to_string(l.slot_bytes) + " bytes need " + std::to_string(l.slot_bytes * count)).c_str());
    std::vector<CropRegionPlace> places(count);
    for (size_t k = 0; k < count; k++) {
        const compeg_crop_region &r = regions[k];
        const std::string which = "region " + std::to_string(k) + ": ";
        if (r.image >= images)
            return fail(COMPEG_E_INVALID_ARG, ("crop regions: " + which + "image " + std::to_string(r.image) + " is beyond the upload's " +
                                               std::to_string(images) + " image(s)").c_str());
        const RegionImage im = image_of(r.image);
        rc = crop_region_fits(*spec, im.width, im.height, r, which);
        if (rc != COMPEG_OK)
            return rc;
        if (crop_region_group(im.hs, im.vs) == kCropRegionGroups)
            return fail(COMPEG_E_UNSUPPORTED, ("crop regions: " + which + "image " + std::to_string(r.image) + "'s luma sampling " + std::to_string(im.hs) +
                                               "x" + std::to_string(im.vs) + " has no cropped kernel").c_str());
        places[k] = CropRegionPlace{r.image, r.x, r.y, r.width, r.height, r.dst_x, r.dst_y, im.hs, im.vs, im.intervals};
    }
    const CropRegionsTarget target{static_cast<uint8_t *>(device_dst), uint64_t(spec->slot_width) * spec->slot_height, l.pitch, spec->format};
    *call = make_crop_regions_call(target, l.slot_bytes, spec->format == COMPEG_CROP_RGBA ? 4u : 1u, places.data(), count);
    return COMPEG_OK;
}

int decoder_cropped_regions(compeg_decoder *dec, const compeg_image *img, const compeg_crop_regions_spec *spec, const compeg_crop_region *regions,
                            size_t count, void *device_dst, size_t dst_bytes, void *hip_stream, bool blocking)
{
    return guarded([&] {
        if (!dec || !img)
            return fail(COMPEG_E_INVALID_ARG, "NULL argument");
        const RegionImage im = region_image(*img->data);
        CropRegionsCall call;
        const int rc = crop_regions_call(spec, regions, count, 1, [&](uint32_t) { return im; }, device_dst, dst_bytes, &call);
        if (rc != COMPEG_OK)
            return rc;
        if (count == 0)
            return ok();
        const hipStream_t stream = stream_of(*dec, hip_stream);
        const Status s = dec->decode_cropped_regions(*img->data, call, stream);
        if (!s.ok())
            return fail(s);
        const hipError_t e = blocking ? hipStreamSynchronize(stream) : hipSuccess;
        return e == hipSuccess ? ok() : fail(hip_status(e, "hipStreamSynchronize"));
    });
}

} // namespace

extern "C" {

int compeg_crop_regions_shape(const compeg_crop_regions_spec *spec, uint32_t *pitch, uint64_t *slot_bytes)
{
    return guarded([&] {
        CropSlotLayout l;
        const int rc = crop_regions_layout(spec, &l);
        if (rc != COMPEG_OK)
            return rc;
        if (pitch)
            *pitch = l.pitch;
        if (slot_bytes)
            *slot_bytes = l.slot_bytes;
        return ok();
    });
}

int compeg_crop_region_check(const compeg_crop_regions_spec *spec, uint32_t image_width, uint32_t image_height, const compeg_crop_region *region)
{
    return guarded([&] {
        CropSlotLayout l;
        const int rc = crop_regions_layout(spec, &l);
        if (rc != COMPEG_OK)
            return rc;
        if (!region)
            return fail(COMPEG_E_INVALID_ARG, "region is NULL");
        if (image_width == 0 || image_height == 0)
            return fail(COMPEG_E_INVALID_ARG, "crop regions: the image has no pixels");
        return crop_region_fits(*spec, image_width, image_height, *region, "");
    });
}

int compeg_batch_decode_cropped_regions(compeg_batch *batch, const compeg_crop_regions_spec *spec, const compeg_crop_region *regions, size_t count,
                                        void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return guarded([&] {
        if (!batch)
            return fail(COMPEG_E_INVALID_ARG, null_text(batch));
        const Status up = batch->finish_upload(); // (the descriptors looked at below are the finished upload's)
        if (!up.ok())
            return fail(up);
        if (batch->count == 0 && count != 0)
            return fail(COMPEG_E_INVALID_ARG, "crop regions: nothing uploaded yet");
        CropRegionsCall call;
        const int rc = crop_regions_call(spec, regions, count, batch->count, [&](uint32_t i) { return region_image(batch->descs[i]); }, device_dst,
                                         dst_bytes, &call);
        if (rc != COMPEG_OK)
            return rc;
        if (count == 0)
            return ok();
        const Status s = batch->decode_cropped_regions(call, stream_of(*batch, hip_stream));
        return s.ok() ? ok() : fail(s);
    });
}

int compeg_decoder_decode_cropped_regions(compeg_decoder *dec, const compeg_image *img, const compeg_crop_regions_spec *spec,
                                          const compeg_crop_region *regions, size_t count, void *device_dst, size_t dst_bytes, void *hip_stream)
{
    return decoder_cropped_regions(dec, img, spec, regions, count, device_dst, dst_bytes, hip_stream, false);
}

int compeg_decoder_decode_cropped_regions_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_crop_regions_spec *spec,
                                                   const compeg_crop_region *regions, size_t count, void *device_dst, size_t dst_bytes)
{
    return decoder_cropped_regions(dec, img, spec, regions, count, device_dst, dst_bytes, nullptr, true);
}

} // extern "C"
