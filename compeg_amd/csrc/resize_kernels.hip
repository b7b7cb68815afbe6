// The resize_tensor_* kernels (resize_body.h): one kernel per filter, element type and downscale factor, a lane per
// 16-byte run of an output row; and the resize_tensor_antialias_* kernels (antialias_body.h), one per element type and
// downscale factor, a lane per output element.  No LDS, no lane exchange; compiled with the library's flags
// (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "antialias_body.h"
#include "kernels.h"
#include "resize_body.h"

namespace compeg {

// Grid: flat over (image, run) -- blocks_per_image workgroups for every image, one behind the other in x.
#define CG_RESIZE_KERNEL(fname, FILTER, name, DTYPE, K)                                                               \
    __global__ void __launch_bounds__(kTensorThreads) resize_tensor_##fname##_##name##_k##K##_kernel(ResizePack t)    \
    {                                                                                                                 \
        resize_tensor_block_lane<DTYPE, K, FILTER>(t, blockIdx.x, threadIdx.x);                                       \
    }
#define CG_RESIZE_KERNELS(fname, FILTER, name, DTYPE) \
    CG_RESIZE_KERNEL(fname, FILTER, name, DTYPE, 1)   \
    CG_RESIZE_KERNEL(fname, FILTER, name, DTYPE, 2)   \
    CG_RESIZE_KERNEL(fname, FILTER, name, DTYPE, 4)   \
    CG_RESIZE_KERNEL(fname, FILTER, name, DTYPE, 8)
#define CG_RESIZE_FILTER(fname, FILTER)                      \
    CG_RESIZE_KERNELS(fname, FILTER, u8, COMPEG_TENSOR_U8)   \
    CG_RESIZE_KERNELS(fname, FILTER, f16, COMPEG_TENSOR_F16) \
    CG_RESIZE_KERNELS(fname, FILTER, bf16, COMPEG_TENSOR_BF16) \
    CG_RESIZE_KERNELS(fname, FILTER, f32, COMPEG_TENSOR_F32)

CG_RESIZE_FILTER(nearest, COMPEG_RESIZE_NEAREST)
CG_RESIZE_FILTER(bilinear, COMPEG_RESIZE_BILINEAR)

using ResizeKernel = void (*)(ResizePack);

static_assert(sizeof(ResizeImage) == kResizeRecordBytes, "kernels.h states the record's size");

bool make_resize_record(void *record, const void *src, uint32_t pitch, const compeg_rect &crop, uint32_t k, uint32_t ow, uint32_t oh)
{
    ResizeImage im;
    if (!plan_resize_image(im, src, pitch, crop, k, ow, oh))
        return false;
    memcpy(record, &im, sizeof im);
    return true;
}

hipError_t launch_resize_tensor(const void *device_records, uint32_t images, const compeg_tensor_spec &spec,
                                const compeg_resize_spec &resize, void *dst, hipStream_t stream)
{
    static const ResizeKernel kernels[2][4][4] = {
#define CG_RESIZE_ROW(fname, name)                                                                        \
    {resize_tensor_##fname##_##name##_k1_kernel, resize_tensor_##fname##_##name##_k2_kernel,              \
     resize_tensor_##fname##_##name##_k4_kernel, resize_tensor_##fname##_##name##_k8_kernel}
        {CG_RESIZE_ROW(nearest, u8), CG_RESIZE_ROW(nearest, f16), CG_RESIZE_ROW(nearest, bf16), CG_RESIZE_ROW(nearest, f32)},
        {CG_RESIZE_ROW(bilinear, u8), CG_RESIZE_ROW(bilinear, f16), CG_RESIZE_ROW(bilinear, bf16), CG_RESIZE_ROW(bilinear, f32)}};
    ResizePack t;
    uint32_t blocks = 0;
    if (!device_records || !plan_resize_pack(t, blocks, images, spec, resize, dst))
        return hipErrorInvalidValue;
    t.images = static_cast<const ResizeImage *>(device_records);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[resize.filter][spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

// ---- antialiased bilinear ------------------------------------------------------------------------------------------

// Grid: flat over (image, element) -- blocks_per_image workgroups for every image, one behind the other in x.
#define CG_ANTIALIAS_KERNEL(name, DTYPE, K)                                                                           \
    __global__ void __launch_bounds__(kTensorThreads) resize_tensor_antialias_##name##_k##K##_kernel(AntialiasPack t) \
    {                                                                                                                 \
        antialias_tensor_block_lane<DTYPE, K>(t, blockIdx.x, threadIdx.x);                                            \
    }
#define CG_ANTIALIAS_KERNELS(name, DTYPE) \
    CG_ANTIALIAS_KERNEL(name, DTYPE, 1)   \
    CG_ANTIALIAS_KERNEL(name, DTYPE, 2)   \
    CG_ANTIALIAS_KERNEL(name, DTYPE, 4)   \
    CG_ANTIALIAS_KERNEL(name, DTYPE, 8)

CG_ANTIALIAS_KERNELS(u8, COMPEG_TENSOR_U8)
CG_ANTIALIAS_KERNELS(f16, COMPEG_TENSOR_F16)
CG_ANTIALIAS_KERNELS(bf16, COMPEG_TENSOR_BF16)
CG_ANTIALIAS_KERNELS(f32, COMPEG_TENSOR_F32)

using AntialiasKernel = void (*)(AntialiasPack);

static_assert(sizeof(AntialiasImage) == kResizeRecordBytes, "kernels.h states the record's size");

bool make_antialias_blob(std::vector<uint32_t> &blob, size_t &tables_at, const AntialiasSource *sources, uint32_t images, uint32_t k,
                         uint32_t ow, uint32_t oh)
{
    // (a record is 40 bytes, ten of the tables' words: the tables grow behind the records in the block that travels)
    constexpr size_t kRecordWords = sizeof(AntialiasImage) / 4u;
    AntialiasTables tables(size_t(images) * kRecordWords);
    for (uint32_t i = 0; i < images; i++) {
        AntialiasImage im;
        if (!plan_antialias_image(im, tables, sources[i].src, sources[i].pitch, sources[i].crop, k, ow, oh))
            return false;
        memcpy(tables.words.data() + i * kRecordWords, &im, sizeof im);
    }
    tables_at = size_t(images) * sizeof(AntialiasImage);
    blob.swap(tables.words);
    return true;
}

hipError_t launch_resize_tensor_antialias(const void *device_blob, size_t tables_at, uint32_t images, const compeg_tensor_spec &spec,
                                          const compeg_resize_spec &resize, void *dst, hipStream_t stream)
{
    static const AntialiasKernel kernels[4][4] = {
#define CG_ANTIALIAS_ROW(name)                                                                  \
    {resize_tensor_antialias_##name##_k1_kernel, resize_tensor_antialias_##name##_k2_kernel,    \
     resize_tensor_antialias_##name##_k4_kernel, resize_tensor_antialias_##name##_k8_kernel}
        CG_ANTIALIAS_ROW(u8), CG_ANTIALIAS_ROW(f16), CG_ANTIALIAS_ROW(bf16), CG_ANTIALIAS_ROW(f32)};
    AntialiasPack t;
    uint32_t blocks = 0;
    if (!device_blob || tables_at != size_t(images) * sizeof(AntialiasImage) || !plan_antialias_pack(t, blocks, images, spec, resize, dst))
        return hipErrorInvalidValue;
    t.images = static_cast<const AntialiasImage *>(device_blob);
    t.tables = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(device_blob) + tables_at);
    const uint32_t k = spec.downscale, ki = k == 1u ? 0u : k == 2u ? 1u : k == 4u ? 2u : 3u;
    hipLaunchKernelGGL(kernels[spec.dtype][ki], dim3(blocks), dim3(kTensorThreads), 0, stream, t);
    return hipGetLastError();
}

} // namespace compeg
