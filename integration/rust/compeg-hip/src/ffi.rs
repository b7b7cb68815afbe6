//! Raw declarations of `include/compeg_hip.h`, one group per reference type.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_double, c_float, c_int, c_uint, c_void};

macro_rules! opaque {
    ($($name:ident),*) => { $(#[repr(C)] pub struct $name { _private: [u8; 0] })* };
}
opaque!(compeg_gpu, compeg_decoder, compeg_image, compeg_scanbuffer, compeg_op, compeg_batch);

/// Host microseconds of a decode's stages (the reference's trace timers, src/lib.rs:391-396,452-475,516-522).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct compeg_stage_times {
    pub preprocess_us: c_double,
    pub enqueue_writes_us: c_double,
    pub poll_us: c_double,
}

/// What `compeg_*_pack_tensor` makes of the RGBA8 output (compeg_hip.h, "Tensor output").
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct compeg_tensor_spec {
    pub dtype: u32,
    pub order: u32,
    pub downscale: u32,
    pub reserved: u32,
    pub scale: [c_float; 3],
    pub bias: [c_float; 3],
}

/// The output extent and the filter of `compeg_*_pack_tensor_resized` (compeg_hip.h, "Resized tensor output").
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct compeg_resize_spec {
    pub out_width: u32,
    pub out_height: u32,
    pub filter: u32,
    pub reserved: u32,
}

/// A crop in pixels.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct compeg_rect {
    pub x: u32,
    pub y: u32,
    pub width: u32,
    pub height: u32,
}

/// C's `float` under its own name: the signatures below read like the header's, parameter by parameter.
#[allow(non_camel_case_types)]
pub type float = c_float;

/// One output slot of `compeg_*_pack_tensor_regions` (compeg_hip.h, "Region tensor output"): which crop of which
/// image fills which rectangle of the slot.  An all-zero `src` is the whole image, an all-zero `dst` the whole output.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct compeg_region {
    pub image: u32,
    pub reserved: u32,
    pub src: compeg_rect,
    pub dst: compeg_rect,
}

/// The output extent and the resampling kernel of `compeg_*_pack_tensor_filtered` (compeg_hip.h, "Filtered tensor
/// output").
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct compeg_filter_spec {
    pub out_width: u32,
    pub out_height: u32,
    pub kernel: u32,
    pub reserved: u32,
}

/// One output slot of `compeg_*_pack_tensor_oriented` (compeg_hip.h, "Oriented tensor output"): a region whose `dst`
/// lies in the upright slot, and the EXIF orientation (1..8; 0: the image's own tag) under which the slot is written.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct compeg_oriented_region {
    pub region: compeg_region,
    pub orientation: u32,
    pub reserved: u32,
}

/// The layout of `compeg_*_pack_tensor_nhwc` (compeg_hip.h, "Channels-last tensor output"): 3 or 4 channels a pixel,
/// and the value of the fourth.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct compeg_nhwc_spec {
    pub channels: u32,
    pub fill: float,
    pub reserved: [u32; 2],
}

/// The weights of `compeg_*_pack_tensor_luma` (compeg_hip.h, "Luma tensor output"): for R, G and B in 1/65536, their sum
/// exactly 65536.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct compeg_luma_spec {
    pub weights: [u32; 3],
    pub reserved: u32,
}

/// What a planes decode writes (compeg_hip.h, "Planar YCbCr output"): the format, the chroma option and the two pitches
/// in bytes (0 = tight).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_planes_spec {
    pub format: u32,
    pub chroma: u32,
    pub luma_pitch: u32,
    pub chroma_pitch: u32,
    pub reserved: [u32; 4],
}

/// Where one image's planes lie (`compeg_planes_shape`): offsets, pitches, row bytes and extents per plane.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_planes_layout {
    pub planes: u32,
    pub reserved: u32,
    pub total_bytes: u64,
    pub offset: [u64; 3],
    pub pitch: [u32; 3],
    pub row_bytes: [u32; 3],
    pub width: [u32; 3],
    pub height: [u32; 3],
}

/// What a reduced decode writes (compeg_hip.h, "Reduced-size decode"): the scale's denominator (8), the format and the
/// RGBA row pitch in bytes (0 = tight).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_reduced_spec {
    pub denominator: u32,
    pub format: u32,
    pub pitch: u32,
}

/// What a scaled decode writes (compeg_hip.h, "Scaled decode"): the scale's denominator (2, 4 or 8), the format and the
/// RGBA row pitch in bytes (0 = tight).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_scaled_spec {
    pub denominator: u32,
    pub format: u32,
    pub pitch: u32,
}

/// What a levels decode writes (compeg_hip.h, "Levels decode"): the order of a block's 64 values; `reserved` is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_levels_spec {
    pub order: u32,
    pub reserved: [u32; 3],
}

/// Where one image's blocks of quantised DCT coefficients lie (`compeg_levels_shape`): per component the offset, the
/// raster of blocks (whole MCUs) and libjpeg's `width_in_blocks` / `height_in_blocks`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_levels_layout {
    pub components: u32,
    pub reserved: u32,
    pub offset: [u64; 3],
    pub blocks_w: [u32; 3],
    pub blocks_h: [u32; 3],
    pub width_in_blocks: [u32; 3],
    pub height_in_blocks: [u32; 3],
    pub total_bytes: u64,
}

/// What a cropped decode writes (compeg_hip.h, "Cropped decode"): the rectangle in pixels of the image, the format and
/// the RGBA row pitch in bytes (0 = tight); `reserved` is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_crop_spec {
    pub x: u32,
    pub y: u32,
    pub width: u32,
    pub height: u32,
    pub format: u32,
    pub pitch: u32,
    pub reserved: [u32; 2],
}

/// One region of a cropped decode of a region list (compeg_hip.h, "Cropped decode of a region list"): the rectangle in
/// pixels of image `image` and where its top-left pixel lies in its slot; `reserved` is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_crop_region {
    pub image: u32,
    pub x: u32,
    pub y: u32,
    pub width: u32,
    pub height: u32,
    pub dst_x: u32,
    pub dst_y: u32,
    pub reserved: u32,
}

/// Every region's slot in pixels, the format and the RGBA row pitch in bytes (0 = tight); `reserved` is 0.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct compeg_crop_regions_spec {
    pub slot_width: u32,
    pub slot_height: u32,
    pub format: u32,
    pub pitch: u32,
    pub reserved: [u32; 4],
}

pub const COMPEG_OK: c_int = 0;
pub const COMPEG_E_INVALID_ARG: c_int = -1;
pub const COMPEG_E_UNSUPPORTED: c_int = -2;
pub const COMPEG_E_MALFORMED: c_int = -3;
pub const COMPEG_E_COUNT_MISMATCH: c_int = -4;
pub const COMPEG_E_HIP: c_int = -5;
pub const COMPEG_PARSE_ANY_LUMA_SAMPLING: c_uint = 1;
pub const COMPEG_PARSE_STANDARD_ENTROPY: c_uint = 2;
pub const COMPEG_PARSE_GRAYSCALE: c_uint = 4;
pub const COMPEG_KERNEL_NONE: c_int = 0;
pub const COMPEG_KERNEL_FUSED: c_int = 1;
pub const COMPEG_KERNEL_PAIR: c_int = 2;
pub const COMPEG_KERNEL_COOP_TEAM: c_int = 3;
pub const COMPEG_KERNEL_GENERIC: c_int = 4;
pub const COMPEG_KERNEL_SPLIT: c_int = 5;
pub const COMPEG_KERNEL_FUSED_LAYOUT: c_int = 6;
pub const COMPEG_KERNEL_FUSED_STREAM: c_int = 7;
pub const COMPEG_KERNEL_WALK_MCU: c_int = 8;
pub const COMPEG_KERNEL_PLANES: c_int = 9;
pub const COMPEG_KERNEL_REDUCED: c_int = 10;
pub const COMPEG_KERNEL_CROPPED: c_int = 11;
pub const COMPEG_KERNEL_SCALED: c_int = 12;
pub const COMPEG_KERNEL_LEVELS: c_int = 13;
pub const COMPEG_LEVELS_ZIGZAG: u32 = 0;
pub const COMPEG_LEVELS_NATURAL: u32 = 1;
pub const COMPEG_SCALED_RGBA: u32 = 0;
pub const COMPEG_SCALED_RGB_PLANAR: u32 = 1;
pub const COMPEG_CROP_RGBA: u32 = 0;
pub const COMPEG_CROP_RGB_PLANAR: u32 = 1;
pub const COMPEG_REDUCED_RGBA: u32 = 0;
pub const COMPEG_REDUCED_RGB_PLANAR: u32 = 1;
pub const COMPEG_PLANES_PLANAR: u32 = 0;
pub const COMPEG_PLANES_SEMIPLANAR: u32 = 1;
pub const COMPEG_PLANES_YUYV: u32 = 2;
pub const COMPEG_PLANES_UYVY: u32 = 3;
pub const COMPEG_CHROMA_AS_CODED: u32 = 0;
pub const COMPEG_CHROMA_420: u32 = 1;
pub const COMPEG_TENSOR_U8: u32 = 0;
pub const COMPEG_TENSOR_F16: u32 = 1;
pub const COMPEG_TENSOR_BF16: u32 = 2;
pub const COMPEG_TENSOR_F32: u32 = 3;
pub const COMPEG_TENSOR_RGB: u32 = 0;
pub const COMPEG_TENSOR_BGR: u32 = 1;
pub const COMPEG_RESIZE_NEAREST: u32 = 0;
pub const COMPEG_RESIZE_BILINEAR: u32 = 1;
/// A flag OR-ed into `compeg_resize_spec::filter`; only with `COMPEG_RESIZE_BILINEAR`.
pub const COMPEG_RESIZE_ANTIALIAS: u32 = 0x100;
pub const COMPEG_FIT_CENTER: c_uint = 0;
pub const COMPEG_FIT_TOP_LEFT: c_uint = 1;
pub const COMPEG_FILTER_BOX: u32 = 0;
pub const COMPEG_FILTER_TRIANGLE: u32 = 1;
pub const COMPEG_FILTER_BICUBIC: u32 = 2;
pub const COMPEG_FILTER_LANCZOS3: u32 = 3;
/// `compeg_oriented_region::orientation`: the image's own tag (`compeg_image_orientation`).
pub const COMPEG_ORIENT_FROM_IMAGE: u32 = 0;

extern "C" {
    pub fn compeg_last_error() -> *const c_char;
    pub fn compeg_version() -> *const c_char;

    // Gpu
    pub fn compeg_gpu_open(device: c_int, out: *mut *mut compeg_gpu) -> c_int;
    pub fn compeg_gpu_from_stream(device: c_int, hip_stream: *mut c_void, out: *mut *mut compeg_gpu) -> c_int;
    pub fn compeg_gpu_retain(gpu: *mut compeg_gpu);
    pub fn compeg_gpu_release(gpu: *mut compeg_gpu);
    pub fn compeg_gpu_device(gpu: *const compeg_gpu) -> c_int;
    pub fn compeg_gpu_name(gpu: *const compeg_gpu) -> *const c_char;

    // ImageData
    pub fn compeg_image_parse(jpeg: *const u8, len: usize, copy: c_int, out: *mut *mut compeg_image) -> c_int;
    pub fn compeg_image_parse_ext(jpeg: *const u8, len: usize, copy: c_int, flags: c_uint,
                                  out: *mut *mut compeg_image) -> c_int;
    pub fn compeg_image_free(img: *mut compeg_image);
    pub fn compeg_image_width(img: *const compeg_image) -> u32;
    pub fn compeg_image_height(img: *const compeg_image) -> u32;
    pub fn compeg_image_parallelism(img: *const compeg_image) -> u32;
    pub fn compeg_image_components(img: *const compeg_image) -> u32;
    pub fn compeg_image_sampling(img: *const compeg_image, hsample: *mut u32, vsample: *mut u32) -> c_int;
    pub fn compeg_image_metadata(img: *const compeg_image) -> *const u8;
    pub fn compeg_image_huffman_l1(img: *const compeg_image) -> *const u8;
    pub fn compeg_image_huffman_l2(img: *const compeg_image, nbytes: *mut usize) -> *const u8;
    pub fn compeg_image_scan_range(img: *const compeg_image, offset: *mut usize, len: *mut usize);

    // ScanBuffer
    pub fn compeg_scanbuffer_new() -> *mut compeg_scanbuffer;
    pub fn compeg_scanbuffer_free(sb: *mut compeg_scanbuffer);
    pub fn compeg_scanbuffer_process(sb: *mut compeg_scanbuffer, scan: *const u8, len: usize, expected: u32) -> c_int;
    pub fn compeg_scanbuffer_set_threads(sb: *mut compeg_scanbuffer, threads: c_uint) -> c_int;
    pub fn compeg_scanbuffer_process_on_gpu(sb: *mut compeg_scanbuffer, gpu: *mut compeg_gpu, scan: *const u8,
                                            len: usize, expected: u32) -> c_int;
    pub fn compeg_scanbuffer_data(sb: *const compeg_scanbuffer, nbytes: *mut usize) -> *const u8;
    pub fn compeg_scanbuffer_start_positions(sb: *const compeg_scanbuffer, nbytes: *mut usize) -> *const u8;

    // Decoder / DecodeOp
    pub fn compeg_decoder_new(gpu: *mut compeg_gpu, out: *mut *mut compeg_decoder) -> c_int;
    pub fn compeg_decoder_free(dec: *mut compeg_decoder);
    pub fn compeg_decoder_enqueue(dec: *mut compeg_decoder, img: *const compeg_image, hip_stream: *mut c_void,
                                  texture_changed: *mut c_int) -> c_int;
    pub fn compeg_decoder_start_decode(dec: *mut compeg_decoder, img: *const compeg_image,
                                       op: *mut *mut compeg_op) -> c_int;
    pub fn compeg_decoder_decode_blocking(dec: *mut compeg_decoder, img: *const compeg_image,
                                          op: *mut *mut compeg_op) -> c_int;
    pub fn compeg_decoder_last_warning(dec: *const compeg_decoder) -> *const c_char;
    pub fn compeg_decoder_last_stage_times(dec: *const compeg_decoder, out: *mut compeg_stage_times) -> c_int;
    pub fn compeg_decoder_last_kernel(dec: *const compeg_decoder) -> c_int;
    pub fn compeg_decoder_set_device_preprocess(dec: *mut compeg_decoder, on: c_int) -> c_int;
    pub fn compeg_decoder_set_scan_threads(dec: *mut compeg_decoder, threads: c_uint) -> c_int;
    pub fn compeg_op_wait(op: *mut compeg_op) -> c_int;
    pub fn compeg_op_texture_changed(op: *const compeg_op) -> c_int;
    pub fn compeg_op_free(op: *mut compeg_op);
    pub fn compeg_decoder_output(dec: *const compeg_decoder, device_ptr: *mut *mut c_void, width: *mut u32,
                                 height: *mut u32, pitch_bytes: *mut usize) -> c_int;
    pub fn compeg_decoder_take_output(dec: *mut compeg_decoder, device_ptr: *mut *mut c_void, width: *mut u32,
                                      height: *mut u32, pitch_bytes: *mut usize) -> c_int;
    pub fn compeg_device_free(device_ptr: *mut c_void);
    pub fn compeg_decoder_read_output(dec: *mut compeg_decoder, host_rgba: *mut u8, width: u32, height: u32) -> c_int;
    pub fn compeg_decoder_read_coefficients(dec: *mut compeg_decoder, host: *mut i32, count: usize) -> c_int;

    // Batch (extension)
    pub fn compeg_batch_new(gpu: *mut compeg_gpu, out: *mut *mut compeg_batch) -> c_int;
    pub fn compeg_batch_free(batch: *mut compeg_batch);
    pub fn compeg_batch_upload(batch: *mut compeg_batch, images: *const *const compeg_image, count: usize,
                               host_threads: c_int) -> c_int;
    pub fn compeg_batch_upload_jpegs(batch: *mut compeg_batch, jpegs: *const *const u8, lengths: *const usize,
                                     count: usize, host_threads: c_int, flags: c_uint) -> c_int;
    pub fn compeg_host_feed_work(jpegs: *const *const u8, lengths: *const usize, count: usize, host_threads: c_int,
                                 flags: c_uint, road: c_int, reps: c_int, seconds: *mut c_double) -> c_int;
    pub fn compeg_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn compeg_host_free(ptr: *mut c_void);
    pub fn compeg_host_register(ptr: *mut c_void, bytes: usize) -> c_int;
    pub fn compeg_host_unregister(ptr: *mut c_void) -> c_int;
    pub fn compeg_batch_upload_jpegs_begin(batch: *mut compeg_batch, jpegs: *const *const u8, lengths: *const usize,
                                           count: usize, host_threads: c_int, flags: c_uint) -> c_int;
    pub fn compeg_batch_upload_end(batch: *mut compeg_batch) -> c_int;
    pub fn compeg_batch_decode(batch: *mut compeg_batch, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_set_device_preprocess(batch: *mut compeg_batch, mode: c_int) -> c_int;
    pub fn compeg_batch_host_fallbacks(batch: *const compeg_batch) -> usize;
    pub fn compeg_batch_set_chunk(batch: *mut compeg_batch, images_per_launch: u32) -> c_int;
    pub fn compeg_batch_wait(batch: *mut compeg_batch) -> c_int;
    pub fn compeg_batch_count(batch: *const compeg_batch) -> usize;
    pub fn compeg_batch_output(batch: *const compeg_batch, index: usize, device_ptr: *mut *mut c_void,
                               width: *mut u32, height: *mut u32, pitch_bytes: *mut usize) -> c_int;
    pub fn compeg_batch_read_output(batch: *mut compeg_batch, index: usize, host_rgba: *mut u8) -> c_int;
    pub fn compeg_batch_algorithmic_bytes(batch: *const compeg_batch) -> u64;
    pub fn compeg_batch_pixels(batch: *const compeg_batch) -> u64;
    pub fn compeg_batch_set_timing(batch: *mut compeg_batch, on: c_int) -> c_int;
    pub fn compeg_batch_timing(batch: *mut compeg_batch, reset: c_int, decodes: *mut u32, total_ms: *mut c_double,
                               stage_ms: *mut c_double) -> c_int;
    pub fn compeg_batch_last_kernel(batch: *const compeg_batch) -> c_int;

    // Tensor output (extension)
    pub fn compeg_tensor_shape(spec: *const compeg_tensor_spec, width: u32, height: u32, out_width: *mut u32,
                               out_height: *mut u32, bytes_per_image: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec, device_dst: *mut c_void,
                                      dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor(batch: *mut compeg_batch, spec: *const compeg_tensor_spec, device_dst: *mut c_void,
                                    dst_bytes: usize, hip_stream: *mut c_void) -> c_int;

    // Resized tensor output (extension)
    pub fn compeg_resized_tensor_shape(spec: *const compeg_tensor_spec, resize: *const compeg_resize_spec, width: u32, height: u32,
                                       crop: *const compeg_rect, pre_width: *mut u32, pre_height: *mut u32,
                                       bytes_per_image: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_resized(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec,
                                              resize: *const compeg_resize_spec, crop: *const compeg_rect, device_dst: *mut c_void,
                                              dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_resized(batch: *mut compeg_batch, spec: *const compeg_tensor_spec,
                                            resize: *const compeg_resize_spec, crops: *const compeg_rect, device_dst: *mut c_void,
                                            dst_bytes: usize, hip_stream: *mut c_void) -> c_int;

    // Region tensor output (extension)
    pub fn compeg_region_fit(src_width: u32, src_height: u32, out_width: u32, out_height: u32, align: c_uint,
                             dst: *mut compeg_rect) -> c_int;
    pub fn compeg_region_tensor_shape(spec: *const compeg_tensor_spec, resize: *const compeg_resize_spec, width: u32, height: u32,
                                      region: *const compeg_region, pre_width: *mut u32, pre_height: *mut u32,
                                      bytes_per_slot: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_regions(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec,
                                              resize: *const compeg_resize_spec, regions: *const compeg_region, count: usize,
                                              pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                              hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_regions(batch: *mut compeg_batch, spec: *const compeg_tensor_spec,
                                            resize: *const compeg_resize_spec, regions: *const compeg_region, count: usize,
                                            pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                            hip_stream: *mut c_void) -> c_int;

    // Filtered tensor output (extension)
    pub fn compeg_filtered_tensor_shape(spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec, width: u32, height: u32,
                                        region: *const compeg_region, pre_width: *mut u32, pre_height: *mut u32,
                                        bytes_per_slot: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_filtered(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec,
                                               filter: *const compeg_filter_spec, regions: *const compeg_region, count: usize,
                                               pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                               hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_filtered(batch: *mut compeg_batch, spec: *const compeg_tensor_spec,
                                             filter: *const compeg_filter_spec, regions: *const compeg_region, count: usize,
                                             pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                             hip_stream: *mut c_void) -> c_int;

    // Oriented tensor output (extension)
    pub fn compeg_image_orientation(img: *const compeg_image) -> u32;
    pub fn compeg_batch_image_orientation(batch: *const compeg_batch, index: usize, out: *mut u32) -> c_int;
    pub fn compeg_orient_rect(upright_width: u32, upright_height: u32, orientation: u32, upright: *const compeg_rect,
                              stored: *mut compeg_rect) -> c_int;
    pub fn compeg_oriented_tensor_shape(spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec, width: u32, height: u32,
                                        region: *const compeg_oriented_region, pre_width: *mut u32, pre_height: *mut u32,
                                        bytes_per_slot: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_oriented(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec,
                                               filter: *const compeg_filter_spec, regions: *const compeg_oriented_region,
                                               count: usize, pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                               hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_oriented(batch: *mut compeg_batch, spec: *const compeg_tensor_spec,
                                             filter: *const compeg_filter_spec, regions: *const compeg_oriented_region,
                                             count: usize, pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                             hip_stream: *mut c_void) -> c_int;

    // Channels-last tensor output (extension)
    pub fn compeg_nhwc_tensor_shape(spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec, nhwc: *const compeg_nhwc_spec,
                                    width: u32, height: u32, region: *const compeg_oriented_region, pre_width: *mut u32,
                                    pre_height: *mut u32, bytes_per_slot: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_nhwc(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec,
                                           nhwc: *const compeg_nhwc_spec, regions: *const compeg_oriented_region, count: usize,
                                           pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                           hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_nhwc(batch: *mut compeg_batch, spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec,
                                         nhwc: *const compeg_nhwc_spec, regions: *const compeg_oriented_region, count: usize,
                                         pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                         hip_stream: *mut c_void) -> c_int;

    // Luma tensor output (extension)
    pub fn compeg_luma_tensor_shape(spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec, luma: *const compeg_luma_spec,
                                    width: u32, height: u32, region: *const compeg_oriented_region, pre_width: *mut u32,
                                    pre_height: *mut u32, bytes_per_slot: *mut usize) -> c_int;
    pub fn compeg_decoder_pack_tensor_luma(dec: *mut compeg_decoder, spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec,
                                           luma: *const compeg_luma_spec, regions: *const compeg_oriented_region, count: usize,
                                           pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                           hip_stream: *mut c_void) -> c_int;
    pub fn compeg_batch_pack_tensor_luma(batch: *mut compeg_batch, spec: *const compeg_tensor_spec, filter: *const compeg_filter_spec,
                                         luma: *const compeg_luma_spec, regions: *const compeg_oriented_region, count: usize,
                                         pad: *const float, device_dst: *mut c_void, dst_bytes: usize,
                                         hip_stream: *mut c_void) -> c_int;

    // Planar YCbCr output (extension)
    pub fn compeg_planes_shape(spec: *const compeg_planes_spec, width: u32, height: u32, components: u32, hsample: u32, vsample: u32,
                               layout: *mut compeg_planes_layout) -> c_int;
    pub fn compeg_batch_decode_planes(batch: *mut compeg_batch, spec: *const compeg_planes_spec, device_dst: *mut c_void,
                                      dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_planes(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_planes_spec,
                                        device_dst: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_planes_blocking(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_planes_spec,
                                                 device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_reduced_shape(spec: *const compeg_reduced_spec, width: u32, height: u32, out_width: *mut u32, out_height: *mut u32,
                                pitch: *mut u32, total_bytes: *mut u64) -> c_int;
    pub fn compeg_batch_decode_reduced(batch: *mut compeg_batch, spec: *const compeg_reduced_spec, device_dst: *mut c_void,
                                       dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_reduced(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_reduced_spec,
                                         device_dst: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_reduced_blocking(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_reduced_spec,
                                                  device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_crop_shape(spec: *const compeg_crop_spec, image_width: u32, image_height: u32, pitch: *mut u32,
                             total_bytes: *mut u64) -> c_int;
    pub fn compeg_batch_decode_cropped(batch: *mut compeg_batch, spec: *const compeg_crop_spec, device_dst: *mut c_void,
                                       dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_cropped(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_crop_spec,
                                         device_dst: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_cropped_blocking(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_crop_spec,
                                                  device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_crop_regions_shape(spec: *const compeg_crop_regions_spec, pitch: *mut u32, slot_bytes: *mut u64) -> c_int;
    pub fn compeg_crop_region_check(spec: *const compeg_crop_regions_spec, image_width: u32, image_height: u32,
                                    region: *const compeg_crop_region) -> c_int;
    pub fn compeg_batch_decode_cropped_regions(batch: *mut compeg_batch, spec: *const compeg_crop_regions_spec,
                                               regions: *const compeg_crop_region, count: usize, device_dst: *mut c_void,
                                               dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_cropped_regions(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_crop_regions_spec,
                                                 regions: *const compeg_crop_region, count: usize, device_dst: *mut c_void,
                                                 dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_cropped_regions_blocking(dec: *mut compeg_decoder, img: *const compeg_image,
                                                          spec: *const compeg_crop_regions_spec, regions: *const compeg_crop_region,
                                                          count: usize, device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_scaled_shape(spec: *const compeg_scaled_spec, width: u32, height: u32, out_width: *mut u32, out_height: *mut u32,
                               pitch: *mut u32, total_bytes: *mut u64) -> c_int;
    pub fn compeg_batch_decode_scaled(batch: *mut compeg_batch, spec: *const compeg_scaled_spec, device_dst: *mut c_void,
                                      dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_scaled(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_scaled_spec,
                                        device_dst: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_scaled_blocking(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_scaled_spec,
                                                 device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_levels_shape(spec: *const compeg_levels_spec, width: u32, height: u32, components: u32, hsample: u32, vsample: u32,
                               layout: *mut compeg_levels_layout) -> c_int;
    pub fn compeg_batch_decode_levels(batch: *mut compeg_batch, spec: *const compeg_levels_spec, device_dst: *mut c_void,
                                      dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_levels(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_levels_spec,
                                        device_dst: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> c_int;
    pub fn compeg_decoder_decode_levels_blocking(dec: *mut compeg_decoder, img: *const compeg_image, spec: *const compeg_levels_spec,
                                                 device_dst: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn compeg_image_quant_table(img: *const compeg_image, component: u32, out: *mut u16, order: u32) -> c_int;
    pub fn compeg_batch_quant_table(batch: *const compeg_batch, index: usize, component: u32, out: *mut u16, order: u32) -> c_int;
}
