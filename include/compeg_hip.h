/*
 * compeg_hip.h -- C ABI of libcompeg_hip.so: an MI355X-native (gfx950) decoder
 * for baseline 8-bit YCbCr 4:2:2 restart-interval JPEGs.
 *
 * The entry points are what a Rust `compeg`-shaped crate binds in place of the
 * reference's wgpu-backed implementation.  Each group cites the reference
 * interface it replaces (paths relative to SludgePhD/Compeg, v0.5.0).
 * INTEGRATION.md shows the Rust side.
 *
 * Conventions
 *   - every fallible call returns COMPEG_OK (0) or a negative COMPEG_E_* code;
 *     the message is available from compeg_last_error() (thread-local).  Texts
 *     equal the reference's error strings where it has one (src/lib.rs:622-793,
 *     src/file.rs:21-25,43-45,281-283,345-347, src/scan.rs:58-63).
 *   - nothing in this library aborts the process; inputs on which the
 *     reference panics (src/lib.rs:784-785 division by zero, src/huffman.rs
 *     asserts, src/file.rs:316,331-335 slicing) return COMPEG_E_MALFORMED.
 *   - objects are not internally synchronised: one thread at a time per
 *     decoder / scan buffer (the reference's `&mut self`), any number of
 *     decoders per compeg_gpu (the reference's `Arc<Gpu>`).
 *   - `hip_stream` arguments are `hipStream_t` passed as `void*` (NULL = the
 *     default stream) so that the header needs no HIP include.
 */
#ifndef COMPEG_HIP_H
#define COMPEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library itself is built -fvisibility=hidden */
#endif

#define COMPEG_OK 0
#define COMPEG_E_INVALID_ARG (-1) /* NULL handle, bad size ...                       */
#define COMPEG_E_UNSUPPORTED (-2) /* well-formed JPEG outside the supported subset   */
#define COMPEG_E_MALFORMED (-3)   /* broken stream (incl. inputs the reference panics on) */
#define COMPEG_E_COUNT_MISMATCH (-4) /* restart-interval count mismatch (scan.rs:58-63) */
#define COMPEG_E_HIP (-5)         /* HIP runtime failure, no usable gfx950 device    */

/* Size of the uniform block shared by all kernels (src/metadata.rs:21-41). */
#define COMPEG_METADATA_BYTES 1112
#define COMPEG_HUFFMAN_L1_BYTES 2048

typedef struct compeg_gpu compeg_gpu;
typedef struct compeg_decoder compeg_decoder;
typedef struct compeg_image compeg_image;
typedef struct compeg_scanbuffer compeg_scanbuffer;
typedef struct compeg_op compeg_op;
typedef struct compeg_batch compeg_batch;

/* Last error message of the calling thread ("" if none). */
const char *compeg_last_error(void);
/* Library version string, e.g. "compeg-hip 0.1.0 (gfx950)". */
const char *compeg_version(void);

/* ---- Gpu: src/lib.rs:64-270 (`Gpu::open`, `Gpu::from_wgpu`) -------------- */

/* Opens HIP device `device` (-1 = current device) and loads the gfx950 code
 * object.  The handle is reference-counted and immutable, i.e. shareable
 * between threads like `Arc<Gpu>`. */
int compeg_gpu_open(int device, compeg_gpu **out);
/* `from_wgpu` analogue: adopt a caller-owned stream as the queue that
 * start_decode / decode_blocking submit to. */
int compeg_gpu_from_stream(int device, void *hip_stream, compeg_gpu **out);
void compeg_gpu_retain(compeg_gpu *gpu);
void compeg_gpu_release(compeg_gpu *gpu);
int compeg_gpu_device(const compeg_gpu *gpu);
/* Human-readable device name ("AMD Instinct MI355X ..."), valid while gpu lives. */
const char *compeg_gpu_name(const compeg_gpu *gpu);

/* ---- ImageData: src/lib.rs:576-851 ---------------------------------------- */

/* Parses and validates a JPEG (`ImageData::new`).  copy != 0 keeps a private
 * copy of the bytes (Cow::Owned); copy == 0 borrows them (Cow::Borrowed): the
 * caller keeps `jpeg` alive and unchanged while the image is in use. */
int compeg_image_parse(const uint8_t *jpeg, size_t len, int copy, compeg_image **out);
/* Extension: flags widen the accepted subset.  With
 * COMPEG_PARSE_ANY_LUMA_SAMPLING the luma component may be sampled 1x1, 2x1,
 * 1x2 or 2x2 against 1x1 chroma (4:4:4, 4:2:2, 4:4:0, 4:2:0); the reference
 * rejects all but 2x1 (lib.rs:650-660).  4:4:4 decodes as the reference's
 * shaders would decode it if its front-end let it through; for the 16-row
 * MCUs of 4:4:0 / 4:2:0 the shaders' nearest-neighbour chroma rule is
 * continued vertically (oracle/compeg_oracle.c, orc_finalize_pass).  flags == 0
 * is compeg_image_parse. */
#define COMPEG_PARSE_ANY_LUMA_SAMPLING 1u
/* COMPEG_PARSE_STANDARD_ENTROPY: the image is entropy-decoded as ITU-T T.81 has
 * it in the two places where the reference deviates -- the bit reader is topped
 * up in front of DC codes as well (the reference does not, huffman.wgsl:157-160,
 * and loses the rest of a restart interval when a DC code needs more bits than
 * it has buffered), and ZRL skips 16 positions (the reference skips 17,
 * huffman.wgsl:176-179).  Everything else (32 retained coefficients, IDCT,
 * colour conversion) stays the reference's.  On valid streams the output then
 * no longer depends on the restart interval. */
#define COMPEG_PARSE_STANDARD_ENTROPY 2u
/* COMPEG_PARSE_GRAYSCALE: baseline frames with one component are accepted too
 * (the reference rejects them, lib.rs:640-672).  The lone component's sampling
 * factors (1..4 each) are ignored as T.81 A.2.2 has it: an MCU is one 8x8 data
 * unit, the image ceil(X/8) x ceil(Y/8) of them.  Such an image decodes to
 * what its 4:4:4 twin decodes to -- the same file with Cb = Cr = 128
 * throughout --: R = G = B = the luma sample, A = 255; retained coefficients,
 * entropy quirks and the transform are those of every other image.  Its
 * Metadata block describes component 0 as 1x1 and leaves components 1 and 2
 * zero, with max_hsample = max_vsample = dus_per_mcu = 1. */
#define COMPEG_PARSE_GRAYSCALE 4u
int compeg_image_parse_ext(const uint8_t *jpeg, size_t len, int copy, unsigned flags, compeg_image **out);
void compeg_image_free(compeg_image *img);
uint32_t compeg_image_width(const compeg_image *img);       /* lib.rs:828-831 */
uint32_t compeg_image_height(const compeg_image *img);      /* lib.rs:834-837 */
uint32_t compeg_image_parallelism(const compeg_image *img); /* lib.rs:838-846 */
/* Extension: components of the frame -- 3, or 1 for a grayscale image (COMPEG_PARSE_GRAYSCALE). */
uint32_t compeg_image_components(const compeg_image *img);
/* Extension: the luma component's sampling factors against chroma -- 2x1 (4:2:2), 1x1 (4:4:4), 1x2 (4:4:0), 2x2
 * (4:2:0); 1x1 for a grayscale image (compeg_image_components tells it from 4:4:4).  What a caller sizes the planes
 * of compeg_planes_shape with.  Either output may be NULL. */
int compeg_image_sampling(const compeg_image *img, uint32_t *hsample, uint32_t *vsample);
/* What the reference uploads per image (src/lib.rs:397-407), exposed so that a
 * binding's tests can compare them byte for byte: the 1112-byte Metadata
 * block, the 2048-byte L1 LUT, the L2 LUT, and the location of the
 * entropy-coded segment inside the JPEG. */
const uint8_t *compeg_image_metadata(const compeg_image *img);
const uint8_t *compeg_image_huffman_l1(const compeg_image *img);
const uint8_t *compeg_image_huffman_l2(const compeg_image *img, size_t *nbytes);
void compeg_image_scan_range(const compeg_image *img, size_t *offset, size_t *len);

/* ---- ScanBuffer: src/scan.rs:15-77 (doc-hidden re-export, lib.rs:44-46) ---- */

compeg_scanbuffer *compeg_scanbuffer_new(void);
void compeg_scanbuffer_free(compeg_scanbuffer *sb);
/* `ScanBuffer::process`.  On COMPEG_E_COUNT_MISMATCH the buffers still hold
 * the (truncated) result, as in the reference. */
int compeg_scanbuffer_process(compeg_scanbuffer *sb, const uint8_t *scan, size_t len,
                              uint32_t expected_restart_intervals);
/* Extension: `threads` threads (1..16, default 1) share the work of every following process() call on
 * segments of 64 KiB per thread and more; same output.  The helper threads live as long as the buffer. */
int compeg_scanbuffer_set_threads(compeg_scanbuffer *sb, unsigned threads);
/* Same result, computed by the device-side scan kernels: the
 * segment is copied to HBM, preprocessed there and the two buffers are copied
 * back.  Inputs the kernels hand back (FF runs longer than 512 bytes) are
 * processed on the host. */
int compeg_scanbuffer_process_on_gpu(compeg_scanbuffer *sb, compeg_gpu *gpu, const uint8_t *scan,
                                     size_t len, uint32_t expected_restart_intervals);
/* `processed_scan_data()` / `start_positions()`: valid until the next process(). */
const uint8_t *compeg_scanbuffer_data(const compeg_scanbuffer *sb, size_t *nbytes);
const uint8_t *compeg_scanbuffer_start_positions(const compeg_scanbuffer *sb, size_t *nbytes);

/* ---- Decoder / DecodeOp: src/lib.rs:273-574 ------------------------------- */

int compeg_decoder_new(compeg_gpu *gpu, compeg_decoder **out); /* Decoder::new */
void compeg_decoder_free(compeg_decoder *dec);

/* `Decoder::enqueue(&ImageData, &mut CommandEncoder) -> bool` (lib.rs:385):
 * preprocess on the host, upload, and record the decode on `hip_stream` (the
 * command-encoder analogue) without waiting.  *texture_changed (optional) is
 * set to 1 when the output buffer was reallocated (always on the first call).
 * Like the reference, a restart-interval count mismatch does not stop the
 * decode (lib.rs:391-394 drops that error); it is reported through
 * compeg_decoder_last_warning(). */
int compeg_decoder_enqueue(compeg_decoder *dec, const compeg_image *img, void *hip_stream,
                           int *texture_changed);
/* `start_decode` (lib.rs:483-499): enqueue on the gpu's own stream + submit. */
int compeg_decoder_start_decode(compeg_decoder *dec, const compeg_image *img, compeg_op **op);
/* `decode_blocking` (lib.rs:508-529): start_decode + wait.  (With device-side scan preprocessing the
 * blocking call does without the read-back between the scan kernels and the decode kernel: it looks at the
 * scan kernels' verdict after the decode and, for the rare segment they hand back, decodes again through
 * the host preprocessor before returning.) */
int compeg_decoder_decode_blocking(compeg_decoder *dec, const compeg_image *img, compeg_op **op);
const char *compeg_decoder_last_warning(const compeg_decoder *dec);
/* Host time of the stages of the decoder's last decode, in microseconds -- the three timers the reference
 * traces (`t_preprocess` lib.rs:391-396, `t_enqueue_writes` lib.rs:452-475, `t_poll` lib.rs:516-522):
 *   preprocess_us      scan preprocessing on the host (ScanBuffer::process), or staging the raw segment and
 *                      submitting the scan kernels when preprocessing runs on the device;
 *   enqueue_writes_us  everything else `enqueue` does: tables and descriptor, uploads, kernel launch;
 *   poll_us            the wait for the device in decode_blocking (0 after enqueue / start_decode).
 * Plain data, C layout; all zeros before the first decode. */
typedef struct compeg_stage_times {
    double preprocess_us;
    double enqueue_writes_us;
    double poll_us;
} compeg_stage_times;
int compeg_decoder_last_stage_times(const compeg_decoder *dec, compeg_stage_times *out);
/* Diagnostics: which decode kernel the decoder's last enqueue (compeg_batch_last_kernel: the first launch of the
 * batch's last decode) went to -- the dispatch is by launch size and restart interval, and tests pin a case to the
 * path it is meant to cover.  The reference has one pipeline (lib.rs:436-448) and no counterpart. */
#define COMPEG_KERNEL_NONE 0       /* nothing launched yet (or an image without a complete restart interval) */
#define COMPEG_KERNEL_FUSED 1      /* decode_fused_422_kernel: a lane per restart interval, launches that fill the chip */
#define COMPEG_KERNEL_PAIR 2       /* decode_pair_422_kernel: decoder wave + transformer wave per 64 intervals */
#define COMPEG_KERNEL_COOP_TEAM 3  /* decode_coop_team_422_kernel: the lanes of a team work inside the intervals */
#define COMPEG_KERNEL_GENERIC 4    /* entropy_samples_kernel + composite_generic_kernel (batches of mixed layouts) */
#define COMPEG_KERNEL_SPLIT 5      /* entropy_kernel + idct_composite_kernel (development pipeline) */
#define COMPEG_KERNEL_FUSED_LAYOUT 6 /* decode_fused_444 / _440 / _420 / _gray_kernel (one layout other than 4:2:2; grayscale images) */
#define COMPEG_KERNEL_FUSED_STREAM 7 /* decode_fused_422 / _444 / _440 / _420_stream_kernel: the batch kernels with streamed
                                       windows (long restart intervals, dense streams) */
#define COMPEG_KERNEL_WALK_MCU 8     /* walk_mcus_422_kernel + decode_fused_422_mcu_rec_kernel: a lane per restart interval
                                       finds where the MCUs begin, then a lane per MCU decodes (batches of few or long
                                       restart intervals; single images whose intervals the cooperative kernel does not
                                       take or takes less well: beyond 256 MCUs, no DRI at all, a 4K frame's 1080 teams) */
#define COMPEG_KERNEL_PLANES 9       /* decode_planes_422 / _444 / _440 / _420 / _gray_kernel: a planes decode
                                       (compeg_*_decode_planes), a lane per restart interval */
#define COMPEG_KERNEL_REDUCED 10     /* decode_reduced_422 / _444 / _440 / _420 / _gray_kernel: a reduced decode
                                       (compeg_*_decode_reduced), a lane per restart interval */
#define COMPEG_KERNEL_CROPPED 11     /* decode_cropped_422 / _444 / _440 / _420 / _gray_kernel: a cropped decode
                                       (compeg_*_decode_cropped), a lane per restart interval that touches the rectangle */
#define COMPEG_KERNEL_SCALED 12      /* decode_scaled_422 / _444 / _440 / _420 / _gray_kernel: a scaled decode at 1/2 or
                                       1/4 (compeg_*_decode_scaled), a lane per restart interval */
#define COMPEG_KERNEL_LEVELS 13      /* decode_levels_422 / _444 / _440 / _420 / _gray_kernel: a levels decode
                                       (compeg_*_decode_levels), a lane per restart interval */
int compeg_decoder_last_kernel(const compeg_decoder *dec);
/* Extension: on != 0 moves the scan preprocessing of every following decode
 * from the host (the reference's data flow, default) to the device-side scan
 * kernels; the raw entropy-coded segment is uploaded instead of the
 * preprocessed one.  Results are identical. */
int compeg_decoder_set_device_preprocess(compeg_decoder *dec, int on);
/* Extension: threads the host scan preprocessor of this decoder uses for one image (see
 * compeg_scanbuffer_set_threads).  Default: 8 on hosts with 32 hardware threads or more, 4 with 8 or more, else 1;
 * the environment variable COMPEG_SCAN_THREADS overrides the default.  The default (only) checks itself:
 * the first large segment is timed on one thread and on all, and the helpers are dropped if they lose. */
int compeg_decoder_set_scan_threads(compeg_decoder *dec, unsigned threads);

/* `DecodeOp` (lib.rs:541-574).  compeg_op_wait replaces polling the
 * SubmissionIndex.  Ops are freed by the caller. */
int compeg_op_wait(compeg_op *op);
int compeg_op_texture_changed(const compeg_op *op);
void compeg_op_free(compeg_op *op);

/* `Decoder::texture()` (lib.rs:372-374): the device-resident RGBA8 output,
 * row-major, bytes R,G,B,255, `pitch` bytes per row -- the width rounded up to
 * 16 pixels (rows begin on 64-byte boundaries; the allocation has whole MCU rows
 * too: what an MCU at the texture's edge holds beyond it lands in that padding,
 * which nobody should read).  Like the reference's
 * texture it never shrinks, so width/height may exceed the last image; only
 * the image's own WxH corner is defined.  The pointer stays valid until the
 * next decode that reallocates (texture_changed) or the decoder is freed. */
int compeg_decoder_output(const compeg_decoder *dec, void **device_ptr, uint32_t *width,
                          uint32_t *height, size_t *pitch_bytes);
/* `Decoder::into_texture()` (lib.rs:380-383): transfers ownership of the
 * output allocation to the caller (release it with compeg_device_free) and
 * frees the decoder. */
int compeg_decoder_take_output(compeg_decoder *dec, void **device_ptr, uint32_t *width,
                               uint32_t *height, size_t *pitch_bytes);
void compeg_device_free(void *device_ptr);
/* Test-harness helper (src/tests.rs:52-84 does copy_texture_to_buffer):
 * waits for the decoder's pending work and copies the WxH corner to host
 * memory, tightly packed (4*width bytes per row). */
int compeg_decoder_read_output(compeg_decoder *dec, uint8_t *host_rgba, uint32_t width,
                               uint32_t height);
/* Debug read-back (role of DownloadBuffer, src/dynamic.rs:81-163): the
 * coefficient buffer as the reference's huffman pass leaves it,
 * int32[total_dus*32] at du*32 + zigzag_pos, dequantised. */
int compeg_decoder_read_coefficients(compeg_decoder *dec, int32_t *host_coefficients,
                                     size_t count);

/* ---- Batch (extension; not in the reference) -------------------------------
 * Decodes many independent images with one launch sequence: the images'
 * preprocessed scans and tables are made resident in HBM once
 * (compeg_batch_upload), after which every compeg_batch_decode is pure device
 * work.  Outputs are RGBA8 images in one device allocation, each with rows
 * `pitch` bytes apart (compeg_batch_output: 4 x the width rounded up to 16
 * pixels -- rows on 64-byte boundaries; compeg_batch_read_output hands out a
 * tightly packed copy). */
int compeg_batch_new(compeg_gpu *gpu, compeg_batch **out);
void compeg_batch_free(compeg_batch *batch);
/* Host front-end for all images (preprocess or stage on `host_threads` threads,
 * 0 = one per core, at most 16) + upload, every image sent off as soon as it is
 * ready; replaces any previous content. */
int compeg_batch_upload(compeg_batch *batch, const compeg_image *const *images, size_t count,
                        int host_threads);
/* Records the decode of every uploaded image on hip_stream (NULL = the gpu's
 * stream) and returns without waiting.  Decodes of one batch recorded on different
 * streams are ordered one behind the other (the batch's device buffers are one set). */
/* The same from JPEG bytes (host-fed use): `ImageData::new` for every image -- on the worker threads, it walks the
 * whole entropy-coded segment -- then what compeg_batch_upload does.  flags: COMPEG_PARSE_*.  The bytes are
 * borrowed until the call returns.  An image the front-end rejects fails the whole call with its error text,
 * prefixed "image <index>: ".  Two batches on two compeg_gpu handles (two streams) pipeline a stream of frames:
 * the upload of one runs under the decode of the other (bench.py, "end_to_end"). */
int compeg_batch_upload_jpegs(compeg_batch *batch, const uint8_t *const *jpegs, const size_t *lengths, size_t count,
                              int host_threads, unsigned flags);
/* The copy-free road of compeg_batch_upload_jpegs.  `ImageData::new` borrows the caller's bytes (`Cow::Borrowed`,
 * lib.rs:577-595) and the reference uploads straight from them (lib.rs:397-407).  With device preprocessing
 * (compeg_batch_set_device_preprocess 1 or 2) and JPEG bytes in page-locked memory -- from compeg_host_alloc, or
 * any range made known with compeg_host_register (a capture driver's buffers, a receive ring) -- the host reads
 * the headers only: the entropy-coded segments are fetched by the card's DMA engines from where they lie and
 * preprocessed by the scan kernels, which also check what the skipped walk over the segment would have found (an
 * image with a marker other than RSTn inside its segment is parsed again in full on the host).  Pageable bytes
 * work too; the worker threads then copy them into the batch's own pinned arena first.  The bytes must stay
 * valid and unchanged until the call returns. */
/* Measurement aid (bench.py --host-feed-ranks; no device is touched): the host's share of feeding one batch,
 * `reps` times over on `host_threads` threads -- road 0: ImageData::new + ScanBuffer::process of every image into its
 * place in an arena (what compeg_batch_upload_jpegs does on the host with host preprocessing: every byte read once
 * and written once); road 1: the headers only (the copy-free road above); road 2: the headers, and every file copied
 * into its place in the arena (pageable bytes with device preprocessing: the default of compeg_batch_upload_jpegs
 * without compeg_host_register).  *seconds: wall time of all reps. */
int compeg_host_feed_work(const uint8_t *const *jpegs, const size_t *lengths, size_t count, int host_threads, unsigned flags,
                          int road, int reps, double *seconds);
/* compeg_batch_upload_jpegs in two steps, for a feeder that keeps the link busy.  _begin returns as soon as every
 * transfer is queued (copy-free road: after a peek at the headers; on every other road it does the whole upload);
 * _end waits for the transfers and the scan kernels and finishes the batch (compeg_batch_decode does it too if
 * nobody has).  In between, the feeder begins the next batch's upload: its transfers queue up behind these, and the
 * link does not idle while this batch's results are read and its descriptors made.  The bytes must stay valid
 * and unchanged until _end returns; the batch must not be touched otherwise between the two. */
int compeg_batch_upload_jpegs_begin(compeg_batch *batch, const uint8_t *const *jpegs, const size_t *lengths, size_t count,
                                    int host_threads, unsigned flags);
int compeg_batch_upload_end(compeg_batch *batch);
int compeg_host_alloc(size_t bytes, void **out);
void compeg_host_free(void *ptr);
int compeg_host_register(void *ptr, size_t bytes);
int compeg_host_unregister(void *ptr);
int compeg_batch_decode(compeg_batch *batch, void *hip_stream);
/* Where the scans are preprocessed.  0 (default): on the host during
 * compeg_batch_upload, like the reference.  1: raw entropy-coded segments are
 * uploaded and preprocessed once by the scan kernels.  2: like 1, and every
 * compeg_batch_decode re-runs the scan kernels first, i.e. a decode covers the
 * whole path from raw scan bytes in HBM to RGBA.  Set before upload.  Every layout
 * the front-end accepts (the extension layouts of COMPEG_PARSE_ANY_LUMA_SAMPLING too). */
int compeg_batch_set_device_preprocess(compeg_batch *batch, int mode);
/* Images of the last upload that the scan kernels handed back to the host. */
size_t compeg_batch_host_fallbacks(const compeg_batch *batch);
/* Images per kernel-launch pair (0 = the whole batch in one pair, the default).
 * Smaller chunks keep the coefficient intermediates cache-resident. */
int compeg_batch_set_chunk(compeg_batch *batch, uint32_t images_per_launch);
int compeg_batch_wait(compeg_batch *batch);
size_t compeg_batch_count(const compeg_batch *batch);
/* Device pointer / geometry of image `index`'s output. */
int compeg_batch_output(const compeg_batch *batch, size_t index, void **device_ptr,
                        uint32_t *width, uint32_t *height, size_t *pitch_bytes);
int compeg_batch_read_output(compeg_batch *batch, size_t index, uint8_t *host_rgba);
/* Algorithmic bytes of the uploaded batch as SURVEY.md 8(d) defines them:
 * 4*scan_words + 4*intervals + 1112 + 2048 + L2 bytes + 4*W*H per image. */
uint64_t compeg_batch_algorithmic_bytes(const compeg_batch *batch);
uint64_t compeg_batch_pixels(const compeg_batch *batch);
/* Kernel-level timing of every compeg_batch_decode since the last upload or
 * reset (at most 4096 are kept), measured with HIP events recorded on the
 * stream the kernels ran on: number of decodes, summed total milliseconds and
 * (for unchunked decodes) summed per-stage milliseconds
 * [huffman, idct+composite].  Waits for those decodes to finish; reset != 0
 * then starts a new measurement. */
int compeg_batch_timing(compeg_batch *batch, int reset, uint32_t *decodes, double *total_ms,
                        double stage_ms[2]);
/* on == 0: decodes record no timing events (compeg_batch_timing then reports none).  Every event is a packet the card
 * works through between two kernels: back-to-back decodes of a single frame run closer together without them.
 * Default: on. */
int compeg_batch_set_timing(compeg_batch *batch, int on);
int compeg_batch_last_kernel(const compeg_batch *batch); /* COMPEG_KERNEL_* */

/* ---- Tensor output (extension) -------------------------------
 * The RGBA8 output above is the reference's wgpu::Texture, made for a viewer.  These calls pack the last decode of
 * a decoder or a batch into what a model reads: planar, alpha dropped, optionally shrunk by an integer factor,
 * converted and normalised -- one hand-written kernel in place of a chain of framework operations.  Nothing else
 * changes: no existing call does, launches or reports anything different.
 *
 * Source: the object's RGBA8 output of its last decode; only the image's own WxH corner is used.
 * k = downscale (1, 2, 4 or 8); ow = W / k, oh = H / k (rounded down; both at least 1).
 * Plane c (0..2) takes source channel c (COMPEG_TENSOR_RGB) or 2 - c (COMPEG_TENSOR_BGR).  Output element (c, y, x):
 *   s = integer sum of that channel over the k x k pixels at rows k*y .., columns k*x ..
 *   m = float(s) * (1 / k^2)                 (exact in f32)
 *   v = (m * scale[c]) + bias[c]             (two f32 operations, each rounded; never fused)
 *   stored: v (F32); v rounded to nearest even (F16, BF16); rint(v), half to even, clamped to 0..255 (U8)
 * so that k = 1, scale 1, bias 0, U8 gives the R, G and B planes byte for byte.  (The sign of a zero is not defined.)
 * Destination: caller-owned device memory, contiguous, no padding: [3][oh][ow] for a decoder, [count][3][oh][ow]
 * for a batch, aligned to its element size. */
#define COMPEG_TENSOR_U8 0
#define COMPEG_TENSOR_F16 1
#define COMPEG_TENSOR_BF16 2
#define COMPEG_TENSOR_F32 3
#define COMPEG_TENSOR_RGB 0
#define COMPEG_TENSOR_BGR 1
typedef struct compeg_tensor_spec {
    uint32_t dtype, order, downscale, reserved; /* COMPEG_TENSOR_*; reserved = 0 */
    float scale[3];
    float bias[3];
} compeg_tensor_spec;
/* No device needed: the geometry (each output optional) and the byte count of one image's tensor for a WxH source.
 * COMPEG_E_INVALID_ARG for a spec the pack calls reject (values out of range, reserved != 0, a scale or bias that is not
 * finite) and for W < k or H < k. */
int compeg_tensor_shape(const compeg_tensor_spec *spec, uint32_t width, uint32_t height,
                        uint32_t *out_width, uint32_t *out_height, size_t *bytes_per_image);
/* Record the pack of the object's last decode on hip_stream (NULL = the gpu's stream) and return without waiting.
 * The pack runs behind that decode whatever stream it was recorded on, and the object's next decode, upload or
 * read-back runs behind the pack; compeg_batch_wait covers it.  It records none of the batch's timing events.  The
 * decoder's texture never shrinks: the last image's WxH is packed.  COMPEG_E_INVALID_ARG also for: dst_bytes smaller
 * than the tensor, device_dst not aligned to its element size, nothing decoded yet, a batch whose images are not
 * all of one size. */
int compeg_decoder_pack_tensor(compeg_decoder *dec, const compeg_tensor_spec *spec, void *device_dst,
                               size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor(compeg_batch *batch, const compeg_tensor_spec *spec, void *device_dst,
                             size_t dst_bytes, void *hip_stream);

/* ---- Resized tensor output (extension) --------------------------------------
 * compeg_*_pack_tensor above gives W/k x H/k, and a batch only if its images are all of one size.  These calls give
 * every image the same output extent whatever its size: a crop (optional) of the last decode is block-averaged as above,
 * resized with one of two filters and converted, in one hand-written kernel.  Nothing else changes.
 *
 * k = downscale, the crop (cx, cy, cw, ch) (NULL: the whole image), ow x oh the output extent:
 *   prefilter: pw = cw / k, ph = ch / k (rounded down; both at least 1);
 *     P[c][j][i] = float(s) * (1 / k^2), s the integer sum of the channel over the k x k pixels at rows cy + k*j ..,
 *     columns cx + k*i ..                                                        (exact in f32)
 *   ratios: rx = float(double(pw) / double(ow)), ry = float(double(ph) / double(oh))
 *   per axis (x shown): a = float(x) + 0.5f;  b = a * rx
 *     COMPEG_RESIZE_NEAREST:  i = min(int(floor(b)), pw - 1)
 *     COMPEG_RESIZE_BILINEAR: s = max(b - 0.5f, 0);  i0 = min(int(floor(s)), pw - 1);  i1 = min(i0 + 1, pw - 1);
 *                             w1 = s - float(i0);  w0 = 1.0f - w1      (half-pixel centres, no antialiasing)
 *   value: nearest m = P[c][j][i]; bilinear top = (P[j0][i0] * wx0) + (P[j0][i1] * wx1), bot likewise on row j1,
 *     m = (top * wy0) + (bot * wy1)
 *   v = (m * scale[c]) + bias[c], converted and stored as above.
 * Every operation is one rounded f32 operation, never fused.  With ow = pw and oh = ph both filters give
 * compeg_*_pack_tensor of the crop, element for element.  No pixel outside the crop is read.
 * Destination: [3][oh][ow] for a decoder, [count][3][oh][ow] for a batch, tight, aligned to its element size.  A
 * batch's images may differ in size; every image gets the same output extent.
 *
 * Antialiased bilinear: filter = COMPEG_RESIZE_BILINEAR | COMPEG_RESIZE_ANTIALIAS (a mode and a flag, as torch's
 * interpolate has them; the flag goes with no other filter).  Where an axis shrinks the triangle widens with the
 * reduction, as PIL and torchvision's Resize(antialias=True) have it; prefilter, crop, k, scale, bias, order and the
 * conversions are unchanged.  Each axis on its own, n its prefiltered extent (pw or ph), o its output extent, x the
 * output coordinate:
 *   n <= o (the axis does not shrink): first = i0, count = 2, (w_0, w_1) = (w0, w1) of COMPEG_RESIZE_BILINEAR above
 *   n > o, in double on the host:  s = double(n) / double(o);  c = s * (x + 0.5)
 *     lo = max(int64(c - s + 0.5), 0);  hi = min(int64(c + s + 0.5), n)          (conversions truncate toward zero)
 *     first = lo;  count = hi - lo                                                (at least 1)
 *     u_t = max(0, 1 - |(t + lo - c + 0.5) * (1.0 / s)|), t = 0 .. count - 1;  total = the sum of u_t in ascending t
 *     w_t = float(u_t / total)
 *   tap t reads index min(first + t, n - 1)                (the clamp binds only where the axis does not shrink)
 *   horizontal first, in f32:  h = P[j][i_0] * wx_0;  then h = h + (P[j][i_t] * wx_t), t = 1 ..
 *   then vertical over the rows j_t of the y taps in ascending order:  m = h[j_0] * wy_0;  then m = m + (h[j_t] * wy_t)
 *   v = (m * scale[c]) + bias[c], converted and stored as above.
 * Every f32 operation is rounded on its own, never fused.  With neither axis shrinking the result is
 * COMPEG_RESIZE_BILINEAR's, element for element; with ow = pw and oh = ph it is compeg_*_pack_tensor of the crop.
 * Ratio limit: the flag is rejected (COMPEG_E_INVALID_ARG) when pw > 64 * ow or ph > 64 * oh -- choose a larger
 * downscale; count is then 129 at the most. */
#define COMPEG_RESIZE_NEAREST 0
#define COMPEG_RESIZE_BILINEAR 1
#define COMPEG_RESIZE_ANTIALIAS 0x100u /* a flag OR-ed into filter; only with COMPEG_RESIZE_BILINEAR */
typedef struct compeg_resize_spec {
    uint32_t out_width, out_height, filter, reserved; /* 1..65535 each way; COMPEG_RESIZE_* (| the flag); reserved = 0 */
} compeg_resize_spec;
typedef struct compeg_rect {
    uint32_t x, y, width, height;
} compeg_rect;
/* No device needed: validates, and reports the prefiltered crop's extent (each output optional) and the byte count of
 * one image's tensor (3 * oh * ow * element size) for a WxH source.  COMPEG_E_INVALID_ARG for what compeg_tensor_shape
 * rejects and for: an output extent of 0 or above 65535, an unknown filter, reserved != 0, a crop with a side of 0 or
 * one that leaves the image, a crop (or image) smaller than downscale either way, COMPEG_RESIZE_ANTIALIAS with another
 * filter than bilinear or beyond its ratio limit. */
int compeg_resized_tensor_shape(const compeg_tensor_spec *spec, const compeg_resize_spec *resize, uint32_t width,
                                uint32_t height, const compeg_rect *crop, uint32_t *pre_width, uint32_t *pre_height,
                                size_t *bytes_per_image);
/* Like compeg_*_pack_tensor in everything they say about hip_stream, ordering, timing events and the decoder's texture.
 * crop / crops: NULL for whole images; one rectangle for a decoder, one per image for a batch (copied before the call
 * returns). */
int compeg_decoder_pack_tensor_resized(compeg_decoder *dec, const compeg_tensor_spec *spec,
                                       const compeg_resize_spec *resize, const compeg_rect *crop, void *device_dst,
                                       size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor_resized(compeg_batch *batch, const compeg_tensor_spec *spec,
                                     const compeg_resize_spec *resize, const compeg_rect *crops, void *device_dst,
                                     size_t dst_bytes, void *hip_stream);

/* ---- Region tensor output (extension) ----------------------------------------
 * compeg_*_pack_tensor_resized above takes one crop per image, gives slot i to image i and fills the whole ow x oh
 * output with the resized crop.  These calls take a list of regions instead.  A region says which image, which crop
 * of it, and which rectangle of its output slot the resized crop fills; everything outside that rectangle is a pad
 * value.  So M crops from whichever frames hold them become one [M][3][oh][ow] batch, and a frame is fitted into a
 * model's input with its aspect ratio kept (a letterbox), in one hand-written kernel.  Nothing else changes.
 *
 * Destination: [count][3][oh][ow], tight, aligned to its element size; count is the number of regions, not of images:
 * an image may appear any number of times, in any order, or not at all.
 * Inside the inner rectangle: slot r has the inner rectangle (dx, dy, dw, dh) = regions[r].dst.  Element (c, y, x)
 * with dx <= x < dx + dw and dy <= y < dy + dh equals element (c, y - dy, x - dx) of compeg_*_pack_tensor_resized of
 * image regions[r].image with the crop regions[r].src, the output extent dw x dh and the same spec, filter and flag,
 * bit for bit: the prefilter, ratios, taps, tables and summation order above apply with (ow, oh) := (dw, dh).  No pixel
 * outside the crop is read.
 * Outside the inner rectangle: every other element of plane c is
 *   v = (pad[ch] * scale[c]) + bias[c],  ch the source channel of plane c under order (c, or 2 - c)
 * two f32 operations, each rounded, never fused; converted and stored like every other element.  pad: three floats on
 * the 0..255 pixel scale, indexed by source channel (R, G, B); NULL: zeros; any finite value is allowed.
 * Writes: every element of every slot is written exactly once; no byte outside the tensor is written.
 * Antialiasing: COMPEG_RESIZE_ANTIALIAS keeps its ratio limit, against the inner extent: a region is rejected when
 * pw > 64 * dw or ph > 64 * dh.  Axis tables are built once per distinct (n, o) of the call. */
typedef struct compeg_region {
    uint32_t image;    /* index into the batch's last upload; 0 for a decoder */
    uint32_t reserved; /* 0 */
    compeg_rect src;   /* crop inside the image; all four fields 0: the whole image */
    compeg_rect dst;   /* rectangle inside ow x oh that the resized crop fills; all four 0: the whole output */
} compeg_region;       /* 40 bytes */
#define COMPEG_FIT_CENTER 0
#define COMPEG_FIT_TOP_LEFT 1
/* No device needed: the inner rectangle that fits a src_width x src_height crop (its pixel extent, before downscale)
 * into out_width x out_height with its aspect ratio kept, in 64-bit integers:
 *   out_width * src_height <= out_height * src_width:
 *     dw = out_width,  dh = (2 * src_height * out_width + src_width) / (2 * src_width), clamped to 1..out_height
 *   otherwise:
 *     dh = out_height, dw = (2 * src_width * out_height + src_height) / (2 * src_height), clamped to 1..out_width
 *   COMPEG_FIT_CENTER: dx = (out_width - dw) / 2, dy = (out_height - dh) / 2;  COMPEG_FIT_TOP_LEFT: dx = dy = 0
 * (3840x2160 into 640x640: (0, 140, 640, 360); 330x70 into 48x40: (0, 15, 48, 10)).  COMPEG_E_INVALID_ARG for a source
 * extent of 0, an output extent of 0 or above 65535, an unknown align, dst NULL. */
int compeg_region_fit(uint32_t src_width, uint32_t src_height, uint32_t out_width, uint32_t out_height,
                      unsigned align, compeg_rect *dst);
/* No device needed: validates one region (NULL: the whole image into the whole output) of a WxH image as the pack calls
 * do, all but its image index, and reports the prefiltered crop's extent (each output optional) and the byte count of
 * one slot (3 * oh * ow * element size).  COMPEG_E_INVALID_ARG for everything compeg_resized_tensor_shape rejects, the
 * antialias limit taken against the inner extent, and for: reserved != 0, a src or dst with a side of 0 that is not the
 * all-zero rectangle, a dst that leaves ow x oh. */
int compeg_region_tensor_shape(const compeg_tensor_spec *spec, const compeg_resize_spec *resize, uint32_t width,
                               uint32_t height, const compeg_region *region, uint32_t *pre_width,
                               uint32_t *pre_height, size_t *bytes_per_slot);
/* Like compeg_*_pack_tensor_resized in everything they say about hip_stream, ordering, timing events, the decoder's
 * texture and compeg_batch_wait.  regions (count of them) and pad are copied before the call returns.
 * COMPEG_E_INVALID_ARG, a message about a region naming its index ("region 3: ..."), for what
 * compeg_region_tensor_shape rejects and for: regions NULL or count 0, an image index beyond the batch (or not 0 on
 * a decoder), a pad value that is not finite, dst_bytes smaller than the tensor, device_dst not aligned to its element
 * size, a launch whose grid does not fit (2^31 workgroups of 256 lanes), nothing decoded yet. */
int compeg_decoder_pack_tensor_regions(compeg_decoder *dec, const compeg_tensor_spec *spec,
                                       const compeg_resize_spec *resize, const compeg_region *regions, size_t count,
                                       const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor_regions(compeg_batch *batch, const compeg_tensor_spec *spec,
                                     const compeg_resize_spec *resize, const compeg_region *regions, size_t count,
                                     const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);

/* ---- Filtered tensor output (extension) --------------------------------------
 * compeg_*_pack_tensor_regions with the separable resampling kernels of PIL's Image.resize, each widened with the
 * reduction: box (area averaging), triangle (PIL's BILINEAR), bicubic with a = -0.5 (PIL's BICUBIC, torch's
 * interpolate(mode="bicubic", antialias=True)) and Lanczos of support 3.  New entry points beside the old ones: no
 * existing call does anything different.
 *
 * Regions, crops, inner rectangles, pad, destination, writes: the region tensor output's, above.  The prefilter P (crop,
 * downscale k, block mean), scale, bias, order, the conversions and the u8 clamp: the resized tensor output's.
 * Each axis on its own: n its prefiltered extent (pw or ph), o the inner extent (dw or dh), S the kernel's support
 * (0.5, 1, 2, 3), x the output coordinate counted inside the inner rectangle.  On the host, in double:
 *   s = double(n) / double(o);  sc = max(s, 1.0);  sup = S * sc;  inv = 1.0 / sc;  c = s * (x + 0.5)
 *   lo = max(int64(c - sup + 0.5), 0);  hi = min(int64(c + sup + 0.5), n)      (truncated toward zero)
 *   first = lo;  count = hi - lo  (>= 1)
 *   u_t = f((t + lo - c + 0.5) * inv), t = 0 .. count - 1;  total = u_0 + u_1 + ..  (ascending t);  w_t = float(u_t / total)
 * with f(z):
 *   box:       1 for -0.5 < z <= 0.5, else 0
 *   triangle:  max(0, 1 - |z|)
 *   bicubic:   a = -0.5, q = |z|:  ((a + 2) q - (a + 3)) q q + 1 for q < 1;  (((q - 5) q + 8) q - 4) a for q < 2;  else 0
 *   lanczos3:  sinc(z) sinc(z / 3) for -3 <= z < 3, else 0;  sinc(0) = 1, sinc(z) = sin(pi z) / (pi z), sin the C library's
 * Weights may be negative.  Tap t reads index first + t, always inside the axis: no pixel outside the crop is read.
 * Then in f32, every operation rounded on its own, never fused:
 *   h(j) = P[j][i_0] * wx_0;  then h = h + (P[j][i_t] * wx_t) for the further x taps          (horizontal, row j)
 *   m = h(j_0) * wy_0;  then m = m + (h(j_t) * wy_t) over the y taps' rows in ascending order  (vertical)
 *   v = (m * scale[c]) + bias[c], converted and stored like every other tensor element (u8: rounded to even, clamped to
 *   0..255 -- bicubic and Lanczos overshoot at hard edges)
 * Tap limit: a region is rejected when n * 2S > 128 * o on either axis (2S = 1, 2, 4, 6: box reduces by 128 at the
 * most, triangle by 64, bicubic by 32, Lanczos by 21); count is then 129 at the most.  Choose a larger downscale.
 * What follows: triangle where both axes shrink is COMPEG_RESIZE_BILINEAR | COMPEG_RESIZE_ANTIALIAS of the same
 * regions, bit for bit; box at o = n / 2, n / 4, n / 8 (n divisible) is compeg_*_pack_tensor at that downscale; box,
 * triangle and bicubic at o = n are compeg_*_pack_tensor of the crop (Lanczos is not: sin(k pi) is not 0 in double). */
#define COMPEG_FILTER_BOX 0      /* support 0.5: area averaging */
#define COMPEG_FILTER_TRIANGLE 1 /* support 1: PIL's BILINEAR */
#define COMPEG_FILTER_BICUBIC 2  /* support 2, a = -0.5: PIL's BICUBIC, torch's bicubic with antialias=True */
#define COMPEG_FILTER_LANCZOS3 3 /* support 3: PIL's LANCZOS */
typedef struct compeg_filter_spec {
    uint32_t out_width, out_height; /* 1 .. 65535 */
    uint32_t kernel;                /* COMPEG_FILTER_* */
    uint32_t reserved;              /* 0 */
} compeg_filter_spec;               /* 16 bytes */
/* No device needed: compeg_region_tensor_shape for the filtered calls.  COMPEG_E_INVALID_ARG for what that rejects of
 * spec, the output extent and the region, and for: an unknown kernel, reserved != 0, an axis beyond the tap limit (the
 * message names both extents and advises a larger downscale). */
int compeg_filtered_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width,
                                 uint32_t height, const compeg_region *region, uint32_t *pre_width,
                                 uint32_t *pre_height, size_t *bytes_per_slot);
/* Like compeg_*_pack_tensor_regions in everything they say about hip_stream, ordering, timing events, the decoder's
 * texture, compeg_batch_wait, the copies made before the call returns, the messages and the rejections, with
 * compeg_filtered_tensor_shape's in place of compeg_region_tensor_shape's. */
int compeg_decoder_pack_tensor_filtered(compeg_decoder *dec, const compeg_tensor_spec *spec,
                                        const compeg_filter_spec *filter, const compeg_region *regions, size_t count,
                                        const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor_filtered(compeg_batch *batch, const compeg_tensor_spec *spec,
                                      const compeg_filter_spec *filter, const compeg_region *regions, size_t count,
                                      const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);

/* ---- Oriented tensor output (extension) --------------------------------------
 * compeg_*_pack_tensor_filtered with an orientation per region: the EXIF values 1..8 (tag 0x0112) -- so a frame whose
 * file says "rotate me" reaches the model upright, and a crop is mirrored where it is packed -- in the same one pass.
 * New entry points beside the old ones: no existing call does anything different.
 *
 * The tag.  compeg_image_orientation gives an image's: read from the first APP1 segment in front of SOS whose payload
 * begins "Exif\0\0" -- TIFF header "II*\0" or "MM\0*", IFD0 at the header's offset, entries of 12 bytes, the entry with
 * tag 0x0112, type 3 (SHORT) and count 1, its value in the file's byte order.  Every read is checked against the
 * segment's length; whatever does not fit (a short segment, an offset outside it, another type or count, a value
 * outside 1..8) gives 1, and so does a file without such a segment.  The tag never changes what compeg_image_parse*
 * accepts or rejects, nor any message.  compeg_batch_image_orientation: the same for image `index` of the last upload,
 * whichever way it was uploaded.  A decoder remembers the tag of the image it decoded last.
 *
 * Contract (exact).  Destination [count][3][oh][ow], tight, (ow, oh) = filter's out_width x out_height: the UPRIGHT
 * slot.  Let o be the region's orientation, COMPEG_ORIENT_FROM_IMAGE replaced by the image's tag.  Let the slot T have
 * the extent (ow', oh') = (ow, oh) for o in 1..4 and (oh, ow) for o in 5..8.  T is, bit for bit, what
 * compeg_*_pack_tensor_filtered stores for the region {image, src, dst'} at the output extent ow' x oh' with the same
 * spec, kernel and pad; src is in the coordinates of the stored raster (compeg_orient_rect maps an upright rectangle
 * there), dst = (dx, dy, dw, dh) in those of the upright slot.  The slot written is U = orient_o(T), every plane alike:
 *   o   U[y][x] =                dst' =                            PIL's Image.transpose
 *   1   T[y][x]                  (dx, dy, dw, dh)                  none
 *   2   T[y][ow-1-x]             (ow-dx-dw, dy, dw, dh)            FLIP_LEFT_RIGHT
 *   3   T[oh-1-y][ow-1-x]        (ow-dx-dw, oh-dy-dh, dw, dh)      ROTATE_180
 *   4   T[oh-1-y][x]             (dx, oh-dy-dh, dw, dh)            FLIP_TOP_BOTTOM
 *   5   T[x][y]                  (dy, dx, dh, dw)                  TRANSPOSE
 *   6   T[ow-1-x][y]             (dy, ow-dx-dw, dh, dw)            ROTATE_270
 *   7   T[ow-1-x][oh-1-y]        (oh-dy-dh, ow-dx-dw, dh, dw)      TRANSVERSE
 *   8   T[x][oh-1-y]             (oh-dy-dh, dx, dh, dw)            ROTATE_90
 * (what PIL's ImageOps.exif_transpose does for a file with that tag).  What follows: orientation 1 is the filtered pack,
 * bit for bit; every element of every slot is written exactly once and no byte outside the tensor is written; the pad
 * fills the image of what it fills in T; the resampling runs along the stored axes; the tap limit n * 2S <= 128 * o is
 * taken against T's axes -- for o in 5..8 pw against dh and ph against dw. */
#define COMPEG_ORIENT_FROM_IMAGE 0 /* the image's own tag (compeg_image_orientation) */
typedef struct compeg_oriented_region {
    compeg_region region;           /* image, src (stored coordinates), dst (in the upright slot) */
    uint32_t orientation, reserved; /* 0..8; reserved = 0 */
} compeg_oriented_region;           /* 48 bytes */
/* 1..8; 1 for NULL. */
uint32_t compeg_image_orientation(const compeg_image *img);
/* COMPEG_E_INVALID_ARG: batch or out NULL, index beyond the last upload. */
int compeg_batch_image_orientation(const compeg_batch *batch, size_t index, uint32_t *out);
/* No device needed: the rectangle of the stored raster that holds the pixels of `upright`, a rectangle of the upright
 * image of upright_width x upright_height: the map dst -> dst' of the table with the upright extents for (ow, oh), in
 * 64-bit integers.  COMPEG_E_INVALID_ARG for an orientation outside 1..8, a NULL pointer, a rectangle that leaves the
 * image. */
int compeg_orient_rect(uint32_t upright_width, uint32_t upright_height, uint32_t orientation, const compeg_rect *upright,
                       compeg_rect *stored);
/* No device needed: compeg_filtered_tensor_shape for the oriented calls; width x height: the stored raster.  There is no
 * image here, so COMPEG_ORIENT_FROM_IMAGE counts as 1.  COMPEG_E_INVALID_ARG for what compeg_filtered_tensor_shape
 * rejects of spec, filter and {src, dst'} at T's extent, and for: an orientation above 8, reserved != 0 (either one).
 * Beyond the tap limit under a transposing orientation the message says that the orientation transposes. */
int compeg_oriented_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, uint32_t width,
                                 uint32_t height, const compeg_oriented_region *region, uint32_t *pre_width,
                                 uint32_t *pre_height, size_t *bytes_per_slot);
/* Like compeg_*_pack_tensor_filtered in everything they say about hip_stream, ordering, timing events, the decoder's
 * texture, compeg_batch_wait, the copies made before the call returns, the messages and the rejections, with
 * compeg_oriented_tensor_shape's in place of compeg_filtered_tensor_shape's. */
int compeg_decoder_pack_tensor_oriented(compeg_decoder *dec, const compeg_tensor_spec *spec,
                                        const compeg_filter_spec *filter, const compeg_oriented_region *regions,
                                        size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                        void *hip_stream);
int compeg_batch_pack_tensor_oriented(compeg_batch *batch, const compeg_tensor_spec *spec,
                                      const compeg_filter_spec *filter, const compeg_oriented_region *regions,
                                      size_t count, const float *pad, void *device_dst, size_t dst_bytes,
                                      void *hip_stream);

/* ---- Channels-last tensor output (extension) ---------------------------------
 * compeg_*_pack_tensor_oriented into a channels-last destination of 3 or 4 channels: what torch.channels_last is for a
 * model, and what PIL, OpenCV, an encoder or a viewer call HWC -- RGB or BGR pixels, or RGBA / RGBX with a constant
 * fourth element -- without a second pass over the tensor.  New entry points beside the old ones: no existing call does
 * anything different.
 *
 * Contract (exact).  Destination [count][oh][ow][C], tight, C = nhwc's channels, (ow, oh) = filter's out_width x
 * out_height: the upright slot.  Element (s, y, x, c) for c < 3 is, bit for bit, element (s, c, y, x) of what
 * compeg_*_pack_tensor_oriented stores for the same spec, filter, regions and pad; spec's order decides what c means, as
 * it does for the planes.  For C = 4 element 3 of every pixel of every slot, the pad's pixels included, is `fill`
 * converted to the element type as any value is (u8: rint and clamp; f16 / bf16: round to nearest even), with neither
 * scale nor bias.  Every element of the tensor is written exactly once and no byte outside it is written.
 * bytes_per_slot = oh * ow * C * element size; device_dst needs the element type's alignment only. */
typedef struct compeg_nhwc_spec {
    uint32_t channels;    /* 3 or 4 */
    float fill;           /* channels == 4: the value of element 3 of every pixel (finite, whatever channels is) */
    uint32_t reserved[2]; /* 0 */
} compeg_nhwc_spec;       /* 16 bytes */
/* No device needed: compeg_oriented_tensor_shape for the channels-last calls.  COMPEG_E_INVALID_ARG for what that one
 * rejects, and for: nhwc NULL, channels other than 3 or 4, a fill that is not finite, a nonzero reserved word. */
int compeg_nhwc_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, const compeg_nhwc_spec *nhwc,
                             uint32_t width, uint32_t height, const compeg_oriented_region *region, uint32_t *pre_width,
                             uint32_t *pre_height, size_t *bytes_per_slot);
/* Like compeg_*_pack_tensor_oriented in everything they say about hip_stream, ordering, timing events, the decoder's
 * texture, compeg_batch_wait, the copies made before the call returns, the messages and the rejections, with
 * compeg_nhwc_tensor_shape's in place of compeg_oriented_tensor_shape's; nhwc is checked with the specs, before the
 * object is looked at.  dst_bytes below count * bytes_per_slot: the message names both numbers. */
int compeg_decoder_pack_tensor_nhwc(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                    const compeg_nhwc_spec *nhwc, const compeg_oriented_region *regions, size_t count,
                                    const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor_nhwc(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                  const compeg_nhwc_spec *nhwc, const compeg_oriented_region *regions, size_t count,
                                  const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);

/* ---- Luma tensor output (extension) ------------------------------------------
 * compeg_*_pack_tensor_oriented with one channel a slot: what a model whose first convolution takes [N, 1, H, W] reads
 * of a grayscale camera's frames, and the luma of a colour frame for OCR, optical flow or focus and exposure metrics --
 * without three identical planes and a slice.  New entry points beside the old ones: no existing call does anything
 * different.
 *
 * Contract (exact).  The source-pixel value: for a pixel (R, G, B, A) of the object's last decode,
 *   L = (wR * R + wG * G + wB * B + 32768) >> 16
 * in unsigned 32-bit arithmetic, (wR, wG, wB) = luma's weights, each 0..65536, their sum exactly 65536: L <= 255.  A
 * decoded grayscale frame has R = G = B = Y, so L = Y exactly, whatever the weights.  With the BT.601 weights L is PIL's
 * Image.convert("L"), byte for byte.  Presets:
 *   BT.601  {19595, 38470,  7471}   PIL's Image.convert("L")
 *   BT.709  {13933, 46871,  4732}
 *   R, G or B alone: {65536, 0, 0}, {0, 65536, 0}, {0, 0, 65536}
 * The tensor: destination [count][1][oh][ow], tight -- the same memory as [count][oh][ow] and [count][oh][ow][1] --
 * (ow, oh) = filter's out_width x out_height: the upright slot.  Element (s, 0, y, x) is, bit for bit, element
 * (s, 0, y, x) of what compeg_*_pack_tensor_oriented would store with order = RGB, the same dtype, downscale, scale[0],
 * bias[0], filter, regions and pad {p, p, p}, if every source pixel's R were replaced by its L.  So the prefilter is
 * P[j][i] = float(sum of L over the k x k block) * (1 / k^2): L is taken per pixel, before the block mean, as
 * convert("L") followed by a reduce is.  Axis tables, tap order, separately rounded f32 operations,
 * v = (m * scale[0]) + bias[0], the conversions, the u8 clamp, the orientation table and the tap limits are the oriented
 * pack's.  Every element of the tensor is written exactly once and no byte outside it is written.
 * bytes_per_slot = oh * ow * element size; device_dst needs the element type's alignment only.
 * Of spec, dtype, downscale, reserved, scale[0] and bias[0] are read; order, scale[1..2] and bias[1..2] are validated as
 * ever and have no effect.  pad points at ONE float on the 0..255 scale (NULL: 0); pad elements are
 * (pad * scale[0]) + bias[0]. */
typedef struct compeg_luma_spec {
    uint32_t weights[3]; /* for R, G, B: each 0..65536, their sum exactly 65536 */
    uint32_t reserved;   /* 0 */
} compeg_luma_spec;      /* 16 bytes */
/* No device needed: compeg_oriented_tensor_shape for the luma calls.  COMPEG_E_INVALID_ARG for what that one rejects, in
 * its words, and for: luma NULL, a weight above 65536 (the message names the weight), a sum other than 65536 (the
 * message names the sum), a nonzero reserved word. */
int compeg_luma_tensor_shape(const compeg_tensor_spec *spec, const compeg_filter_spec *filter, const compeg_luma_spec *luma,
                             uint32_t width, uint32_t height, const compeg_oriented_region *region, uint32_t *pre_width,
                             uint32_t *pre_height, size_t *bytes_per_slot);
/* Like compeg_*_pack_tensor_oriented in everything they say about hip_stream, ordering, timing events, the decoder's
 * texture, compeg_batch_wait, the copies made before the call returns, the messages and the rejections, with
 * compeg_luma_tensor_shape's in place of compeg_oriented_tensor_shape's; luma is checked with the specs, before the
 * object is looked at.  A pad that is not finite is rejected.  dst_bytes below count * bytes_per_slot: the message names
 * both numbers. */
int compeg_decoder_pack_tensor_luma(compeg_decoder *dec, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                    const compeg_luma_spec *luma, const compeg_oriented_region *regions, size_t count,
                                    const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);
int compeg_batch_pack_tensor_luma(compeg_batch *batch, const compeg_tensor_spec *spec, const compeg_filter_spec *filter,
                                  const compeg_luma_spec *luma, const compeg_oriented_region *regions, size_t count,
                                  const float *pad, void *device_dst, size_t dst_bytes, void *hip_stream);

/* ---- Planar YCbCr output (extension) -----------------------------------------
 * A second kind of decode: every component's 8-bit samples as the file codes them, at the component's own resolution,
 * written into caller-owned device memory -- no colour conversion, no chroma upsampling, no clamp beyond the
 * transform's own.  What a hardware video encoder (NV12 / NV16 / I420 / YUY2), a display path or a model trained on
 * YUV or luma reads, without a decode to RGBA and a conversion back.  New entry points beside the old ones: the RGBA
 * output, compeg_decoder_output / _read_output, and what the tensor packs see as "the last decode" are not touched by
 * a planes decode, and without these calls nothing behaves differently.
 *
 * Values.  The bytes written for a data unit are exactly the 64 samples the decoder holds in front of its colour
 * step: Y as decoded, Cb and Cr as decoded (0..255, 128 neutral).  The entropy decode and the transform are those of
 * every other decode (32 retained coefficients, the entropy quirks unless COMPEG_PARSE_STANDARD_ENTROPY, the wrapping
 * predictor, the f32 transform, truncation toward zero).  MCUs behind the last complete restart interval are not
 * decoded and their bytes in the destination are NOT WRITTEN: the memory is the caller's, its previous contents stay.
 *
 * Geometry.  Component c of a W x H image is ceil(W hs_c / hmax) x ceil(H vs_c / vmax) samples; a grayscale image has
 * the luma plane only.  Nothing outside these extents is ever written -- not the rest of a row inside its pitch, not
 * a row below the last; a data unit the extent cuts is stored in part.
 *
 * format:
 *   PLANAR      Y, then Cb, then Cr: I422 / I444 / I440 / I420 / Y800 by the file's sampling
 *   SEMIPLANAR  Y, then one plane of interleaved Cb Cr pairs: NV16 / NV24 / NV12 (no name for 4:4:0)
 *   YUYV, UYVY  one plane of Y0 Cb Y1 Cr (Cb Y0 Cr Y1) groups, 4:2:2 files only -- COMPEG_E_UNSUPPORTED otherwise.  A
 *               row is ceil(W / 2) groups: for an odd W the last group's second luma byte is the sample the file
 *               encodes to the right of the edge, not a replica.
 * chroma:
 *   AS_CODED    the default
 *   CHROMA_420  4:2:2 files only, PLANAR or SEMIPLANAR (I420 / NV12): chroma row r is (a + b + 1) >> 1 of rows 2 r and
 *               2 r + 1 of the coded chroma, sample by sample; the chroma planes are ceil(H / 2) rows.  For an odd H the
 *               last row's partner is the row the file encodes below the edge (MCUs are whole), not a replica.
 *               COMPEG_E_UNSUPPORTED for any other sampling, COMPEG_E_INVALID_ARG with a packed format.
 * luma_pitch / chroma_pitch: bytes from row to row of the first plane (Y, or the packed plane) and of the chroma
 *   planes (Cb and Cr, or CbCr); 0 = tight (the row's bytes), else any value >= the row's bytes.
 * Plane offsets are the library's: plane p + 1 begins at plane p's offset + pitch * height, the first at 0 -- no
 *   alignment is added (alignment 1), so tight planes are byte-compatible with what an encoder expects of
 *   I420 / NV12 / NV16 / YUY2 buffers.  Rows whose plane base and pitch are multiples of 16 bytes (8 for the 8-byte rows
 *   of Cb / Cr planes and of 4:4:4 / 4:4:0 / grayscale luma) take the vector-store path; any other destination is
 *   stored byte by byte and is not refused. */
#define COMPEG_PLANES_PLANAR 0
#define COMPEG_PLANES_SEMIPLANAR 1
#define COMPEG_PLANES_YUYV 2
#define COMPEG_PLANES_UYVY 3
#define COMPEG_CHROMA_AS_CODED 0
#define COMPEG_CHROMA_420 1
typedef struct compeg_planes_spec {
    uint32_t format, chroma;           /* COMPEG_PLANES_*, COMPEG_CHROMA_* */
    uint32_t luma_pitch, chroma_pitch; /* bytes; 0 = tight */
    uint32_t reserved[4];              /* 0 */
} compeg_planes_spec;                  /* 32 bytes */
typedef struct compeg_planes_layout {
    uint32_t planes;       /* 1, 2 or 3 */
    uint32_t reserved;     /* written as 0 */
    uint64_t total_bytes;  /* one image's planes, the last plane's last row at its full pitch */
    uint64_t offset[3];    /* per plane: its first byte ... */
    uint32_t pitch[3];     /* ... bytes from row to row ... */
    uint32_t row_bytes[3]; /* ... bytes of a row that are written ... */
    uint32_t width[3];     /* ... samples a row of each component it carries (packed: luma samples) ... */
    uint32_t height[3];    /* ... and rows; unused planes are all zero */
} compeg_planes_layout;    /* 88 bytes */
/* No device needed: one image's layout for a width x height image of `components` components (3, or 1: grayscale)
 * whose luma is sampled hsample x vsample (compeg_image_sampling).  COMPEG_E_INVALID_ARG for: NULL arguments, a
 * format or chroma value out of range, nonzero reserved words, CHROMA_420 with a packed format, a pitch below the
 * row's bytes (the message names both), a zero extent, a sampling that is none of the five;
 * COMPEG_E_UNSUPPORTED for a packed format or CHROMA_420 on anything but 4:2:2.  Nothing is written on failure. */
int compeg_planes_shape(const compeg_planes_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hsample,
                        uint32_t vsample, compeg_planes_layout *layout);
/* The images of the batch's last upload, image i to device_dst + i * total_bytes.  All images must have one size and one
 * sampling (COMPEG_E_INVALID_ARG with a message otherwise, as compeg_batch_pack_tensor asks for one size); dst_bytes
 * below count * total_bytes is refused before anything is launched (the message names both numbers).  Records on
 * hip_stream (NULL = the gpu's stream) and returns without waiting; compeg_batch_wait covers it.  compeg_batch_set_chunk
 * and the three preprocessing modes work as for compeg_batch_decode.  Any number of calls, with different specs, in any
 * order with compeg_batch_decode, after one upload.  It records none of the batch's timing events.  Ordering is the
 * tensor packs': a planes decode on another stream than the batch's previous work waits for that work, and what the
 * batch does next on another stream waits for it.  compeg_batch_last_kernel then says COMPEG_KERNEL_PLANES.
 * Known limits: a lane per restart interval on every launch (no cooperative, walk or streamed-window form: a single
 * frame or long intervals decode slowly); no mixed sizes or samplings; no resampling but CHROMA_420 from 4:2:2. */
int compeg_batch_decode_planes(compeg_batch *batch, const compeg_planes_spec *spec, void *device_dst, size_t dst_bytes,
                               void *hip_stream);
/* One image: uploads and preprocesses as compeg_decoder_enqueue does (host or device preprocessing), records the planes
 * decode on hip_stream (NULL = the gpu's stream) and returns without waiting.  The decoder's texture, its extent and
 * what the packs read stay those of the last RGBA decode; compeg_decoder_read_coefficients afterwards speaks of this
 * image.  To wait: synchronise hip_stream, or call compeg_decoder_decode_planes_blocking, which does.  The decoder's
 * next enqueue or pack on another stream waits for the planes decode, as this call waits for the decoder's previous
 * work.  compeg_decoder_last_kernel then says COMPEG_KERNEL_PLANES. */
int compeg_decoder_decode_planes(compeg_decoder *dec, const compeg_image *img, const compeg_planes_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream);
int compeg_decoder_decode_planes_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_planes_spec *spec,
                                          void *device_dst, size_t dst_bytes);

/* ---- Reduced-size decode (extension) ------------------------------------------
 * A third kind of decode: the image at 1/8 scale, one RGB pixel per 8 x 8 luma data unit, made from the DC terms alone
 * -- the entropy decode and nothing of the transform -- and written into caller-owned device memory.  What libjpeg
 * calls scale_denom = 8: thumbnails, motion grids, small model inputs, without a full-size image in between.  New
 * entry points beside the old ones: the RGBA output, compeg_decoder_output / _read_output, and what the tensor packs
 * see as "the last decode" are not touched by a reduced decode, and without these calls nothing behaves differently.
 *
 * Reduced extent: ow = ceil(W / 8), oh = ceil(H / 8).
 *
 * One sample per data unit.  dc is the data unit's prediction-summed, dequantised DC term with 32-bit wrap, exactly
 * what every other decode feeds its transform (the entropy quirks unless COMPEG_PARSE_STANDARD_ENTROPY, the wrapping
 * predictor, DC categories above 15 all act as they do there).  The sample is
 *     s = trunc(clamp((float(dc) * 0.125f) + 128.5f, 0, 255))
 * -- one f32 product, one f32 sum, a clamp to 0..255, a truncation.  This is what the decoder's transform leaves in all
 * 64 samples of a data unit whose AC coefficients are zero.
 *
 * Pixel (x, y) of the reduced image.  Y comes from luma data unit (x, y) of the luma grid, Cb and Cr from chroma data
 * unit (x / hs, y / vs) -- nearest neighbour, as the full decode replicates chroma -- and the colour step is the full
 * decode's integer YCbCr -> RGB with A = 255.  For grayscale files R = G = B = s.  Equivalently: pixel (8 x, 8 y) of
 * the full decode of the same file with every AC coefficient set to zero.  It is NOT the mean of the full decode's
 * 8 x 8 block: the colour step clamps per pixel, and the mean of clamped values is not the clamped mean.
 *
 * MCUs behind the last complete restart interval are not decoded and their bytes in the destination are NOT WRITTEN:
 * the memory is the caller's, its previous contents stay.  Nothing outside ow x oh is ever written -- not the rest of
 * a row inside its pitch, not a row below the last; an MCU the reduced extent cuts is stored in part.
 *
 * format:
 *   RGBA        interleaved R G B A, 4 bytes a pixel, A = 255.  pitch: bytes from row to row, 0 = tight (4 ow).  The
 *               destination's address and the pitch must be multiples of 4 (COMPEG_E_INVALID_ARG otherwise).
 *   RGB_PLANAR  [3, oh, ow] bytes, tight, any address: a CHW u8 tensor as it stands.  pitch must be 0.
 * denominator must be 8: 1/8 is the DC-only decode and the only one built (COMPEG_E_INVALID_ARG for any other value). */
#define COMPEG_REDUCED_RGBA 0
#define COMPEG_REDUCED_RGB_PLANAR 1
typedef struct compeg_reduced_spec {
    uint32_t denominator; /* 8 */
    uint32_t format;      /* COMPEG_REDUCED_* */
    uint32_t pitch;       /* RGBA: bytes from row to row, 0 = tight; RGB_PLANAR: 0 */
} compeg_reduced_spec;    /* 12 bytes */
/* No device needed: the reduced extent of a width x height image, the pitch that will be used (RGB_PLANAR: ow) and one
 * image's bytes (RGBA: pitch * oh, the last row at its full pitch; RGB_PLANAR: 3 * ow * oh).  Any output may be NULL.
 * COMPEG_E_INVALID_ARG for: a NULL spec, a denominator other than 8, a format out of range, RGB_PLANAR with a pitch,
 * an RGBA pitch below 4 * ow or not a multiple of 4 (the message names both), a zero extent.  Nothing is written on
 * failure. */
int compeg_reduced_shape(const compeg_reduced_spec *spec, uint32_t width, uint32_t height, uint32_t *out_width,
                         uint32_t *out_height, uint32_t *pitch, uint64_t *total_bytes);
/* The images of the batch's last upload, image i to device_dst + i * total_bytes.  All images must have one size and one
 * sampling (COMPEG_E_INVALID_ARG with a message otherwise, as compeg_batch_decode_planes asks); dst_bytes below
 * count * total_bytes is refused before anything is launched (the message names both numbers).  Records on hip_stream
 * (NULL = the gpu's stream) and returns without waiting; compeg_batch_wait covers it.  compeg_batch_set_chunk and the
 * three preprocessing modes work as for compeg_batch_decode.  Any number of calls, with different specs, in any order
 * with compeg_batch_decode and compeg_batch_decode_planes, after one upload.  It records none of the batch's timing
 * events.  Ordering is the tensor packs': a reduced decode on another stream than the batch's previous work waits for
 * that work, and what the batch does next on another stream waits for it.  compeg_batch_last_kernel then says
 * COMPEG_KERNEL_REDUCED.
 * Known limits: a lane per restart interval on every launch (no cooperative, walk or streamed-window form: a single
 * frame or long intervals decode slowly); no mixed sizes or samplings; 1/8 only; the tensor packs do not read a
 * caller's image. */
int compeg_batch_decode_reduced(compeg_batch *batch, const compeg_reduced_spec *spec, void *device_dst, size_t dst_bytes,
                                void *hip_stream);
/* One image: uploads and preprocesses as compeg_decoder_enqueue does (host or device preprocessing), records the
 * reduced decode on hip_stream (NULL = the gpu's stream) and returns without waiting.  The decoder's texture, its
 * extent and what the packs read stay those of the last RGBA decode.  To wait: synchronise hip_stream, or call
 * compeg_decoder_decode_reduced_blocking, which does.  The decoder's next enqueue or pack on another stream waits for
 * the reduced decode, as this call waits for the decoder's previous work.  compeg_decoder_last_kernel then says
 * COMPEG_KERNEL_REDUCED. */
int compeg_decoder_decode_reduced(compeg_decoder *dec, const compeg_image *img, const compeg_reduced_spec *spec, void *device_dst,
                                  size_t dst_bytes, void *hip_stream);
int compeg_decoder_decode_reduced_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_reduced_spec *spec,
                                           void *device_dst, size_t dst_bytes);

/* ---- Cropped decode (extension) -----------------------------------------------
 * A fourth kind of decode: one rectangle of the image, written into caller-owned device memory that holds the
 * rectangle and nothing else.  What nvJPEG calls a decode ROI and libjpeg-turbo jpeg_crop_scanline: a detector's box, a
 * fixed region of a fixed camera, without the full image in between.  A restart interval none of whose MCUs has a pixel
 * in the rectangle is not decoded, nor read: on restart-interval MJPEG a small rectangle costs a small part of the
 * decode.  New entry points beside the old ones: the RGBA output, compeg_decoder_output / _read_output, and what the
 * tensor packs see as "the last decode" are not touched by a cropped decode, and without these calls nothing behaves
 * differently.
 *
 * The rectangle (x, y, width, height) is in pixels of the W x H image.  It must be non-empty and lie wholly inside the
 * image: width >= 1, height >= 1, x + width <= W, y + height <= H.  x and y need not be aligned to anything.
 *
 * Output pixel (i, j), 0 <= i < width, 0 <= j < height, is pixel (x + i, y + j) of the RGBA decode of the same file
 * (compeg_decoder_decode / compeg_batch_decode), byte for byte, with A = 255: the same transform, chroma replicated to
 * the nearest neighbour, the same integer colour step.  Everything that shapes that decode acts here exactly as there:
 * the entropy quirks Q1, Q2, Q4 and Q5 unless COMPEG_PARSE_STANDARD_ENTROPY, the DC predictor's 32-bit wrap, an
 * interval beyond the scan's restart markers decoding from the scan's first word, grayscale files giving R = G = B.
 *
 * MCUs behind the last complete restart interval are not decoded and their bytes in the destination are NOT WRITTEN:
 * the memory is the caller's, its previous contents stay.  Nothing outside the rectangle's bytes is ever written -- not
 * the rest of a row inside its pitch, not a byte in front of an image or behind it.
 *
 * format:
 *   RGBA        interleaved R G B A, 4 bytes a pixel, A = 255.  pitch: bytes from row to row, 0 = tight (4 width).
 *               The destination's address and the pitch must be multiples of 4 (COMPEG_E_INVALID_ARG otherwise).
 *   RGB_PLANAR  [3, height, width] bytes, tight, any address: a CHW u8 tensor as it stands.  pitch must be 0.
 * reserved must be 0. */
#define COMPEG_CROP_RGBA 0
#define COMPEG_CROP_RGB_PLANAR 1
typedef struct compeg_crop_spec {
    uint32_t x, y, width, height; /* the rectangle, in pixels of the image */
    uint32_t format;              /* COMPEG_CROP_* */
    uint32_t pitch;               /* RGBA: bytes from row to row, 0 = tight; RGB_PLANAR: 0 */
    uint32_t reserved[2];         /* 0 */
} compeg_crop_spec;               /* 32 bytes */
/* No device needed: checks the spec against an image_width x image_height image and gives the pitch that will be used
 * (RGB_PLANAR: width) and one image's bytes (RGBA: pitch * height, the last row at its full pitch; RGB_PLANAR:
 * 3 * width * height).  Either output may be NULL.  COMPEG_E_INVALID_ARG, with a message that states the values, for: a
 * NULL spec, a format out of range, reserved not 0, an image without pixels, an empty rectangle, a rectangle that
 * reaches beyond the image, RGB_PLANAR with a pitch, an RGBA pitch below 4 * width or not a multiple of 4.  Nothing is
 * written on failure. */
int compeg_crop_shape(const compeg_crop_spec *spec, uint32_t image_width, uint32_t image_height, uint32_t *pitch,
                      uint64_t *total_bytes);
/* The images of the batch's last upload, image i to device_dst + i * total_bytes, one rectangle for all of them.  All
 * images must have one size and one sampling (COMPEG_E_INVALID_ARG with a message otherwise, as
 * compeg_batch_decode_planes asks); dst_bytes below count * total_bytes is refused before anything is launched (the
 * message names both numbers).  Records on hip_stream (NULL = the gpu's stream) and returns without waiting;
 * compeg_batch_wait covers it.  compeg_batch_set_chunk and the three preprocessing modes work as for
 * compeg_batch_decode.  Any number of calls, with different specs, in any order with the batch's other decodes, after
 * one upload.  It records none of the batch's timing events.  Ordering is the tensor packs': a cropped decode on another
 * stream than the batch's previous work waits for that work, and what the batch does next on another stream waits for
 * it.  compeg_batch_last_kernel then says COMPEG_KERNEL_CROPPED.
 * Known limits: the scan preprocessing still reads the whole entropy-coded segment, since every interval's start comes
 * from it -- the saving is in the decode kernel; a touched interval is walked from its start up to its last MCU in the
 * rectangle, so a file without DRI or with long intervals saves little; a lane per restart interval on every launch
 * (no cooperative, walk or streamed-window form); no cropped planes or reduced output; the tensor packs do not read a
 * caller's image.  (A rectangle per image, several per image, images of mixed sizes and samplings: "Cropped decode of a
 * region list" below.) */
int compeg_batch_decode_cropped(compeg_batch *batch, const compeg_crop_spec *spec, void *device_dst, size_t dst_bytes,
                                void *hip_stream);
/* One image: uploads and preprocesses as compeg_decoder_enqueue does (host or device preprocessing), records the
 * cropped decode on hip_stream (NULL = the gpu's stream) and returns without waiting.  The decoder's texture, its
 * extent and what the packs read stay those of the last RGBA decode.  To wait: synchronise hip_stream, or call
 * compeg_decoder_decode_cropped_blocking, which does.  The decoder's next enqueue or pack on another stream waits for
 * the cropped decode, as this call waits for the decoder's previous work.  compeg_decoder_last_kernel then says
 * COMPEG_KERNEL_CROPPED. */
int compeg_decoder_decode_cropped(compeg_decoder *dec, const compeg_image *img, const compeg_crop_spec *spec, void *device_dst,
                                  size_t dst_bytes, void *hip_stream);
int compeg_decoder_decode_cropped_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_crop_spec *spec,
                                           void *device_dst, size_t dst_bytes);

/* ---- Cropped decode of a region list (extension) -------------------------------
 * The cropped decode with a rectangle per region: each region names its image and its rectangle and gets a slot of its
 * own in the destination.  A loader's random crop per image, a detector's M boxes out of whichever frames hold them, a
 * dataset of photographs of many sizes with 4:2:0, 4:4:4 and grayscale files side by side.  New entry points beside the
 * old ones: without these calls nothing behaves differently.
 *
 * Destination.  Region k owns slot k, at device_dst + k * slot_bytes; every slot is slot_width x slot_height pixels.
 *   RGBA        slot_height rows of 4 * slot_width bytes at pitch (0 = tight); slot_bytes = pitch * slot_height.
 *               device_dst and pitch must be multiples of 4 and pitch >= 4 * slot_width.
 *   RGB_PLANAR  a tight [3, slot_height, slot_width] u8 block at any address; slot_bytes = 3 * slot_width *
 *               slot_height.  pitch must be 0.
 * So [count, slot_height, slot_width, 4] or [count, 3, slot_height, slot_width] is a tensor as it stands.
 *
 * Pixels.  Pixel (dst_x + i, dst_y + j) of slot k, 0 <= i < width, 0 <= j < height, is pixel (x + i, y + j) of the RGBA
 * decode of image regions[k].image, byte for byte, A = 255.  Everything "Cropped decode" says about the entropy quirks,
 * the DC predictor's wrap, intervals beyond the scan's restart markers and grayscale files applies unchanged.
 *
 * Rectangles.  Each is non-empty and lies inside its image; dst_x + width <= slot_width and dst_y + height <=
 * slot_height.  Any number of regions may name the same image, in any order; an image may be named by none.  x, y,
 * dst_x and dst_y need not be aligned to anything.
 *
 * NOT WRITTEN: everything in a slot outside its region's rectangle -- the rest of the slot (a pad colour the caller put
 * there stays), the rest of a row inside its pitch -- and anything in front of or behind the destination; and the
 * pixels of MCUs behind the image's last complete restart interval.
 *
 * The images may differ in size, sampling (4:2:2, 4:4:4, 4:4:0, 4:2:0, grayscale), entropy mode and tables. */
typedef struct compeg_crop_region {
    uint32_t image;               /* index into the batch's last upload (decoder: 0) */
    uint32_t x, y, width, height; /* the rectangle, in pixels of that image */
    uint32_t dst_x, dst_y;        /* where its top-left pixel lies in its slot */
    uint32_t reserved;            /* 0 */
} compeg_crop_region;             /* 32 bytes */
typedef struct compeg_crop_regions_spec {
    uint32_t slot_width, slot_height; /* every region's slot, in pixels (1 .. 65535) */
    uint32_t format;                  /* COMPEG_CROP_RGBA / COMPEG_CROP_RGB_PLANAR */
    uint32_t pitch;                   /* RGBA: bytes from row to row of a slot, 0 = tight; RGB_PLANAR: 0 */
    uint32_t reserved[4];             /* 0 */
} compeg_crop_regions_spec;           /* 32 bytes */
/* No device needed: checks the spec and gives the pitch that will be used (RGB_PLANAR: slot_width) and one slot's
 * bytes.  Either output may be NULL.  COMPEG_E_INVALID_ARG, with a message that states the values, for: a NULL spec, a
 * format out of range, reserved not 0, a slot extent of 0 or above 65535 (no image has more pixels a side), RGB_PLANAR
 * with a pitch, an RGBA pitch below 4 * slot_width or not a multiple of 4.  Nothing is written on failure. */
int compeg_crop_regions_shape(const compeg_crop_regions_spec *spec, uint32_t *pitch, uint64_t *slot_bytes);
/* No device needed: the spec as above, then one region against an image_width x image_height image and the slot.
 * COMPEG_E_INVALID_ARG with a message that states the values for: a NULL region, an image without pixels, reserved not
 * 0, an empty rectangle, a rectangle that reaches beyond the image, a rectangle that placed at (dst_x, dst_y) reaches
 * beyond the slot.  region->image is not looked at. */
int compeg_crop_region_check(const compeg_crop_regions_spec *spec, uint32_t image_width, uint32_t image_height,
                             const compeg_crop_region *region);
/* `count` regions of the images of the batch's last upload, region k into slot k.  Refused with COMPEG_E_INVALID_ARG
 * and a message that states the values -- nothing is launched or written, whichever region is the bad one, and a
 * refusal that concerns one region names its index: what the two functions above refuse; a NULL batch, device_dst, or
 * regions with count > 0; an RGBA device_dst that is not a multiple of 4; a region whose image is at or beyond the
 * upload's count; dst_bytes below count * slot_bytes (the message names both numbers); nothing uploaded yet.
 * count == 0 succeeds and launches nothing.  The regions are copied during the call: the caller may free them on return.
 * Records on hip_stream (NULL = the gpu's stream) and returns without waiting; compeg_batch_wait covers it.  One launch
 * per sampling present among the images the regions name, at most five; compeg_batch_set_chunk(n) bounds the REGIONS
 * per launch for this call; the three preprocessing modes work as for compeg_batch_decode.  Ordering is the tensor
 * packs', both ways, as for compeg_batch_decode_cropped; no timing events are recorded; the RGBA output and what the
 * packs see as the last decode are left alone.  compeg_batch_last_kernel then says COMPEG_KERNEL_CROPPED.
 * Known limits: one region a slot (no mosaics of several regions in one slot); no scale per region (crop x
 * decode_scaled); no cropped planes or levels; the planes, reduced, scaled and levels decodes still want batches of one
 * size and sampling; regions of the same image share nothing -- each walks its touched intervals itself; a lane per
 * restart interval on every launch (no cooperative, walk or streamed form), so a file without DRI or with long
 * intervals saves little, as for the one-rectangle decode; the tensor packs do not read a caller's image. */
int compeg_batch_decode_cropped_regions(compeg_batch *batch, const compeg_crop_regions_spec *spec, const compeg_crop_region *regions,
                                        size_t count, void *device_dst, size_t dst_bytes, void *hip_stream);
/* One image, M boxes of it: every region's image must be 0.  Uploads and preprocesses as compeg_decoder_decode_cropped
 * does and records the decode on hip_stream; the _blocking form records on the gpu's stream and waits.  The texture, its
 * extent and what the packs read stay those of the last RGBA decode; ordering as for compeg_decoder_decode_cropped.
 * compeg_decoder_last_kernel then says COMPEG_KERNEL_CROPPED. */
int compeg_decoder_decode_cropped_regions(compeg_decoder *dec, const compeg_image *img, const compeg_crop_regions_spec *spec,
                                          const compeg_crop_region *regions, size_t count, void *device_dst, size_t dst_bytes,
                                          void *hip_stream);
int compeg_decoder_decode_cropped_regions_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_crop_regions_spec *spec,
                                                   const compeg_crop_region *regions, size_t count, void *device_dst, size_t dst_bytes);

/* ---- Scaled decode (extension) ------------------------------------------------
 * A fifth kind of decode: the image at 1/2, 1/4 or 1/8 scale, written into caller-owned device memory.  What libjpeg
 * calls scale_denom = 2, 4, 8 and PIL draft(): the size a resize to a model input should start from, without a full-size
 * image in between.  New entry points beside the old ones: the RGBA output, compeg_decoder_output / _read_output, and
 * what the tensor packs see as "the last decode" are not touched by a scaled decode, compeg_*_decode_reduced stays as it
 * is, and without these calls nothing behaves differently.
 *
 * Extent.  denominator den is 2, 4 or 8, N = 8 / den.  ow = ceil(W / den), oh = ceil(H / den).
 *
 * Samples.  Every data unit gives N x N samples, made from the N x N lowest-frequency corner of its dequantised
 * coefficients: F[v][u] with v, u < N, v the vertical frequency, natural index v * 8 + u (zig-zag positions 24 and
 * below: all inside what the decoder retains).  The transform is the separable N-point inverse DCT
 *     f(x, y) = 1/4 sum_u sum_v C(u) C(v) F[v][u] cos((2x + 1) u pi / 2N) cos((2y + 1) v pi / 2N) + 128.5
 * with C(0) = 1 / sqrt(2), C(k) = 1 otherwise, and the sample is trunc(clamp(f, 0, 255)).  This is IJG libjpeg's scaled
 * IDCT (jidctint.c's reduced-size outputs), NOT libjpeg-turbo's jidctred, and NOT the N x N block means of the full
 * decode: the high frequencies are dropped before the transform, not averaged away after it, and the colour step clamps
 * per pixel.
 *
 * Pinned arithmetic.  f32 throughout, every step one IEEE operation, nothing contracted into a fused multiply-add.
 *   inputs      in = float(dc) * 0.125f for the DC term (dc: the prediction-summed, dequantised DC term with 32-bit
 *               wrap, as every other decode takes it); in = (float(level) * quant[z]) * 0.125f for an AC term at zig-zag
 *               position z.
 *   order       the column pass (over v, for each u) first, then the row pass (over u, for each y), which adds 128.5f to
 *               its first input before anything else.
 *   N = 4 pass  A = (float)1.306562965 (sqrt2 cos(pi/8)), B = (float)0.541196100 (sqrt2 cos(3 pi/8)):
 *               e0 = in0 + in2; e1 = in0 - in2; o0 = (in1 * A) + (in3 * B); o1 = (in1 * B) - (in3 * A);
 *               out0 = e0 + o0; out1 = e1 + o1; out2 = e1 - o1; out3 = e0 - o0.
 *   N = 2 pass  out0 = in0 + in1; out1 = in0 - in1.
 *   N = 1       the reduced decode's sample, trunc(clamp((float(dc) * 0.125f) + 128.5f, 0, 255)).
 * With every AC term zero each of the N x N samples equals the reduced decode's sample bit for bit.
 *
 * Pixel (x, y) of the scaled image.  Y comes from the scaled luma plane at (x, y), Cb and Cr from the scaled chroma
 * planes at (x / hs, y / vs) -- nearest neighbour, as the full decode replicates chroma (quirk Q4) -- and the colour step
 * is the full decode's integer YCbCr -> RGB with A = 255.  For grayscale files R = G = B = s.
 *
 * MCUs behind the last complete restart interval are not decoded and their bytes in the destination are NOT WRITTEN:
 * the memory is the caller's, its previous contents stay.  Nothing outside ow x oh is ever written -- not the rest of
 * a row inside its pitch, not a row below the last; an MCU the scaled extent cuts is stored in part.
 *
 * format:
 *   RGBA        interleaved R G B A, 4 bytes a pixel, A = 255.  pitch: bytes from row to row, 0 = tight (4 ow).  The
 *               destination's address and the pitch must be multiples of 4 (COMPEG_E_INVALID_ARG otherwise).
 *   RGB_PLANAR  [3, oh, ow] bytes, tight, any address: a CHW u8 tensor as it stands.  pitch must be 0.
 * denominator must be 2, 4 or 8 (COMPEG_E_INVALID_ARG for any other value).  Denominator 8 runs the reduced decode's
 * kernels: its bytes are compeg_*_decode_reduced's and the last kernel is then COMPEG_KERNEL_REDUCED. */
#define COMPEG_SCALED_RGBA 0
#define COMPEG_SCALED_RGB_PLANAR 1
typedef struct compeg_scaled_spec {
    uint32_t denominator; /* 2, 4 or 8 */
    uint32_t format;      /* COMPEG_SCALED_* */
    uint32_t pitch;       /* RGBA: bytes from row to row, 0 = tight; RGB_PLANAR: 0 */
} compeg_scaled_spec;     /* 12 bytes */
/* No device needed: the scaled extent of a width x height image, the pitch that will be used (RGB_PLANAR: ow) and one
 * image's bytes (RGBA: pitch * oh, the last row at its full pitch; RGB_PLANAR: 3 * ow * oh).  Any output may be NULL.
 * COMPEG_E_INVALID_ARG for: a NULL spec, a denominator other than 2, 4 or 8 (the message says which are built), a format
 * out of range, RGB_PLANAR with a pitch, an RGBA pitch below 4 * ow or not a multiple of 4 (the message names both), a
 * zero extent.  Nothing is written on failure. */
int compeg_scaled_shape(const compeg_scaled_spec *spec, uint32_t width, uint32_t height, uint32_t *out_width,
                        uint32_t *out_height, uint32_t *pitch, uint64_t *total_bytes);
/* The images of the batch's last upload, image i to device_dst + i * total_bytes.  All images must have one size and one
 * sampling (COMPEG_E_INVALID_ARG with a message otherwise, as compeg_batch_decode_planes asks); dst_bytes below
 * count * total_bytes is refused before anything is launched (the message names both numbers).  Records on hip_stream
 * (NULL = the gpu's stream) and returns without waiting; compeg_batch_wait covers it.  compeg_batch_set_chunk and the
 * three preprocessing modes work as for compeg_batch_decode.  Any number of calls, with different specs, in any order
 * with the batch's other decodes, after one upload.  It records none of the batch's timing events.  Ordering is the
 * tensor packs': a scaled decode on another stream than the batch's previous work waits for that work, and what the
 * batch does next on another stream waits for it.  compeg_batch_last_kernel then says COMPEG_KERNEL_SCALED
 * (denominator 8: COMPEG_KERNEL_REDUCED).
 * Known limits: a lane per restart interval on every launch (no cooperative, walk or streamed-window form: a single
 * frame or long intervals decode slowly); no mixed sizes or samplings; no scales above 1 and no other denominators; no
 * planes (YCbCr) output at reduced size; the tensor packs do not read a caller's image. */
int compeg_batch_decode_scaled(compeg_batch *batch, const compeg_scaled_spec *spec, void *device_dst, size_t dst_bytes,
                               void *hip_stream);
/* One image: uploads and preprocesses as compeg_decoder_enqueue does (host or device preprocessing), records the
 * scaled decode on hip_stream (NULL = the gpu's stream) and returns without waiting.  The decoder's texture, its
 * extent and what the packs read stay those of the last RGBA decode.  To wait: synchronise hip_stream, or call
 * compeg_decoder_decode_scaled_blocking, which does.  The decoder's next enqueue or pack on another stream waits for
 * the scaled decode, as this call waits for the decoder's previous work.  compeg_decoder_last_kernel then says
 * COMPEG_KERNEL_SCALED (denominator 8: COMPEG_KERNEL_REDUCED). */
int compeg_decoder_decode_scaled(compeg_decoder *dec, const compeg_image *img, const compeg_scaled_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream);
int compeg_decoder_decode_scaled_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_scaled_spec *spec,
                                          void *device_dst, size_t dst_bytes);

/* ---- Levels decode: quantised DCT coefficients (extension) ----------------------
 * A sixth kind of decode: the file's own quantised DCT coefficients (levels), written into caller-owned device memory
 * as int16 blocks with nothing of the transform applied -- what libjpeg calls jpeg_read_coefficients.  For DCT-domain
 * models, transcoders and forensic tools.  New entry points beside the old ones: the RGBA output, compeg_decoder_output
 * / _read_output, last_w / last_h and what the tensor packs see as "the last decode" are not touched by a levels decode,
 * compeg_decoder_read_coefficients (the debug read-back of 32 dequantised positions) stays as it is, and without these
 * calls nothing behaves differently.
 *
 * Layout.  Component c of a W x H image has blocks_w[c] = width_mcus * hs_c and blocks_h[c] = height_mcus * vs_c blocks
 * (hs_c x vs_c: the component's sampling factors; chroma 1 x 1; width_mcus = ceil(W / (8 hs_0)), height_mcus =
 * ceil(H / (8 vs_0))): whole MCUs, so every decoded data unit has a home and nothing is masked at the image's edge.  The
 * destination holds, component after component, int16[blocks_h[c]][blocks_w[c]][64], tight; component 0 at offset 0;
 * a grayscale image has one component.  The block of data unit (h, v) of component c in MCU (mx, my) is at
 * offset[c] + ((by * blocks_w[c] + bx) * 64) * 2 bytes with bx = mx * hs_c + h, by = my * vs_c + v.  Image i of a batch
 * is at i * total_bytes.  width_in_blocks[c] = ceil(comp_w / 8) and height_in_blocks[c] = ceil(comp_h / 8) with comp_w =
 * ceil(W * hs_c / hs_0), comp_h = ceil(H * vs_c / vs_0) are libjpeg's counts of the blocks that carry image samples:
 * the top-left width_in_blocks x height_in_blocks corner of each raster.
 *
 * Values.  Each value is the level as the entropy decode yields it, NOT multiplied by the quantiser.
 *   position 0      the component's DC predictor after this unit's difference.  The predictor is a 32-bit integer that
 *                   wraps, as on every decode route; its LOW 16 BITS are stored (two's complement).  A conforming file
 *                   keeps it inside 16 bits; a hostile one (DC categories above 11, long runs of large differences) does
 *                   not, and then only the low half is seen here.
 *   positions 1..63 int16(val) of the decoded value, as the decoder's coefficient slot holds it on every route.
 * Quirks Q1 (the reference's reader underflow) and Q2 (a ZRL advances 17 positions), COMPEG_PARSE_STANDARD_ENTROPY and
 * DC categories above 15 act as on every other route.  Quirk Q3 does NOT act: positions 32..63 are kept.  A position
 * beyond 63 -- a corrupt stream reaches one, and so does Q2's 17-step ZRL -- is dropped.
 *
 * order:
 *   ZIGZAG   the file's order: index z of a block is zig-zag position z.
 *   NATURAL  row-major 8 x 8 with the horizontal frequency fastest (libjpeg's JBLOCK): index v * 8 + u holds zig-zag
 *            position ZIGZAG[v * 8 + u], the table every JPEG text prints (0 1 5 6 14 15 27 28 / 2 4 7 13 ...).
 *
 * MCUs behind the last complete restart interval are not decoded and their bytes in the destination are NOT WRITTEN:
 * the memory is the caller's, its previous contents stay.  Nothing outside total_bytes per image is ever written.  The
 * destination's address must be a multiple of 16 (every block is then a 128-byte line); a misaligned address and a
 * dst_bytes too small are refused with COMPEG_E_INVALID_ARG and a message before anything is launched.
 *
 * Not built: dequantised or float output (compeg_image_quant_table gives the factors: one broadcast multiply);
 * batches of mixed size or sampling; the cooperative, walk and streamed-window routes; tensor packs reading a caller's
 * blocks. */
#define COMPEG_LEVELS_ZIGZAG 0
#define COMPEG_LEVELS_NATURAL 1
typedef struct compeg_levels_spec {
    uint32_t order;       /* COMPEG_LEVELS_* */
    uint32_t reserved[3]; /* 0 */
} compeg_levels_spec;     /* 16 bytes */
typedef struct compeg_levels_layout {
    uint32_t components;          /* 1 or 3 */
    uint32_t reserved;            /* written as 0 */
    uint64_t offset[3];           /* per component: its first byte (a multiple of 128) ... */
    uint32_t blocks_w[3];         /* ... blocks a row of its raster ... */
    uint32_t blocks_h[3];         /* ... and rows of blocks: whole MCUs ... */
    uint32_t width_in_blocks[3];  /* ... of which ceil(comp_w / 8) ... */
    uint32_t height_in_blocks[3]; /* ... by ceil(comp_h / 8) carry samples of the image; unused components are all zero */
    uint64_t total_bytes;         /* one image's blocks */
} compeg_levels_layout;           /* 88 bytes */
/* No device needed: one image's layout for a width x height image of `components` components (3, or 1: grayscale)
 * whose luma is sampled hsample x vsample (compeg_image_sampling).  COMPEG_E_INVALID_ARG for: NULL arguments, an order
 * out of range, nonzero reserved words, a zero extent, a sampling that is none of the five, an extent whose blocks
 * overflow the layout's 64-bit byte counts (far beyond what a JPEG header can state).  Nothing is written on failure. */
int compeg_levels_shape(const compeg_levels_spec *spec, uint32_t width, uint32_t height, uint32_t components, uint32_t hsample,
                        uint32_t vsample, compeg_levels_layout *layout);
/* The images of the batch's last upload, image i to device_dst + i * total_bytes.  All images must have one size and one
 * sampling (COMPEG_E_INVALID_ARG with a message otherwise, as compeg_batch_decode_planes asks); dst_bytes below
 * count * total_bytes and an address that is no multiple of 16 are refused before anything is launched.  Records on
 * hip_stream (NULL = the gpu's stream) and returns without waiting; compeg_batch_wait covers it.  compeg_batch_set_chunk
 * and the three preprocessing modes work as for compeg_batch_decode.  Any number of calls, with different specs, in any
 * order with the batch's other decodes, after one upload.  It records none of the batch's timing events.  Ordering is
 * the tensor packs': a levels decode on another stream than the batch's previous work waits for that work, and what the
 * batch does next on another stream waits for it.  compeg_batch_last_kernel then says COMPEG_KERNEL_LEVELS.
 * Known limits: a lane per restart interval on every launch (no cooperative, walk or streamed-window form: a single
 * frame or long intervals decode slowly); no mixed sizes or samplings; no dequantised or float output; the tensor packs
 * do not read a caller's blocks. */
int compeg_batch_decode_levels(compeg_batch *batch, const compeg_levels_spec *spec, void *device_dst, size_t dst_bytes,
                               void *hip_stream);
/* One image: uploads and preprocesses as compeg_decoder_enqueue does (host or device preprocessing), records the
 * levels decode on hip_stream (NULL = the gpu's stream) and returns without waiting.  The decoder's texture, its
 * extent and what the packs read stay those of the last RGBA decode.  To wait: synchronise hip_stream, or call
 * compeg_decoder_decode_levels_blocking, which does.  The decoder's next enqueue or pack on another stream waits for
 * the levels decode, as this call waits for the decoder's previous work.  compeg_decoder_last_kernel then says
 * COMPEG_KERNEL_LEVELS. */
int compeg_decoder_decode_levels(compeg_decoder *dec, const compeg_image *img, const compeg_levels_spec *spec, void *device_dst,
                                 size_t dst_bytes, void *hip_stream);
int compeg_decoder_decode_levels_blocking(compeg_decoder *dec, const compeg_image *img, const compeg_levels_spec *spec,
                                          void *device_dst, size_t dst_bytes);
/* The quantisation table of component `component` (0 .. components - 1) of a parsed image, 64 factors in `order`
 * (COMPEG_LEVELS_*): level * factor, position by position, is the dequantised coefficient -- no second parse of the
 * file.  COMPEG_E_INVALID_ARG for NULL arguments, a component the image does not have, an order out of range.
 * compeg_batch_quant_table: the same for image `index` of the batch's last upload (batches take JPEG bytes without a
 * compeg_image). */
int compeg_image_quant_table(const compeg_image *img, uint32_t component, uint16_t out[64], uint32_t order);
int compeg_batch_quant_table(const compeg_batch *batch, size_t index, uint32_t component, uint16_t out[64], uint32_t order);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* COMPEG_HIP_H */
