"""Loader of the in-tree native library (compeg_amd/libcompeg_hip.so).

There is no Python or CPU fallback: if the library is missing the import fails
loudly, and opening a Gpu without a gfx950 device raises Error."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# COMPEG_LIB: developer override for A/B runs of two builds of the same library (tools/ab_bench.sh)
LIB_PATH = os.environ.get("COMPEG_LIB") or os.path.join(_HERE, "libcompeg_hip.so")

OK, E_INVALID_ARG, E_UNSUPPORTED, E_MALFORMED, E_COUNT_MISMATCH, E_HIP = 0, -1, -2, -3, -4, -5
METADATA_BYTES = 1112
L1_BYTES = 2048


class Error(Exception):
    """String-only error like compeg::Error (src/error.rs:5-46); .code carries the C status."""

    def __init__(self, message, code=E_INVALID_ARG):
        super().__init__(message)
        self.code = code


class TensorSpec(C.Structure):
    """compeg_tensor_spec (include/compeg_hip.h, "Tensor output")."""
    _fields_ = [("dtype", C.c_uint32), ("order", C.c_uint32), ("downscale", C.c_uint32), ("reserved", C.c_uint32),
                ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class ResizeSpec(C.Structure):
    """compeg_resize_spec (include/compeg_hip.h, "Resized tensor output")."""
    _fields_ = [("out_width", C.c_uint32), ("out_height", C.c_uint32), ("filter", C.c_uint32), ("reserved", C.c_uint32)]


class Rect(C.Structure):
    """compeg_rect: a crop in pixels."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class Region(C.Structure):
    """compeg_region (include/compeg_hip.h, "Region tensor output"): which crop of which image fills which rectangle of
    its output slot; an all-zero src is the whole image, an all-zero dst the whole output."""
    _fields_ = [("image", C.c_uint32), ("reserved", C.c_uint32), ("src", Rect), ("dst", Rect)]


class FilterSpec(C.Structure):
    """compeg_filter_spec (include/compeg_hip.h, "Filtered tensor output")."""
    _fields_ = [("out_width", C.c_uint32), ("out_height", C.c_uint32), ("kernel", C.c_uint32), ("reserved", C.c_uint32)]


class OrientedRegion(C.Structure):
    """compeg_oriented_region (include/compeg_hip.h, "Oriented tensor output"): a Region whose dst lies in the upright
    slot, and the orientation (0: the image's own EXIF tag; 1..8: the EXIF values) under which its slot is written."""
    _fields_ = [("region", Region), ("orientation", C.c_uint32), ("reserved", C.c_uint32)]


class NhwcSpec(C.Structure):
    """compeg_nhwc_spec (include/compeg_hip.h, "Channels-last tensor output"): 3 or 4 channels a pixel, and the value of
    the fourth."""
    _fields_ = [("channels", C.c_uint32), ("fill", C.c_float), ("reserved", C.c_uint32 * 2)]


class LumaSpec(C.Structure):
    """compeg_luma_spec (include/compeg_hip.h, "Luma tensor output"): the weights of R, G and B in 1/65536, their sum 65536."""
    _fields_ = [("weights", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class PlanesSpec(C.Structure):
    """compeg_planes_spec (include/compeg_hip.h, "Planar YCbCr output"): format, chroma option and the two pitches."""
    _fields_ = [("format", C.c_uint32), ("chroma", C.c_uint32), ("luma_pitch", C.c_uint32), ("chroma_pitch", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class PlanesLayout(C.Structure):
    """compeg_planes_layout: where one image's planes lie and how large they are."""
    _fields_ = [("planes", C.c_uint32), ("reserved", C.c_uint32), ("total_bytes", C.c_uint64), ("offset", C.c_uint64 * 3),
                ("pitch", C.c_uint32 * 3), ("row_bytes", C.c_uint32 * 3), ("width", C.c_uint32 * 3), ("height", C.c_uint32 * 3)]


class ReducedSpec(C.Structure):
    """compeg_reduced_spec (include/compeg_hip.h, "Reduced-size decode"): the scale's denominator (8), format, RGBA pitch."""
    _fields_ = [("denominator", C.c_uint32), ("format", C.c_uint32), ("pitch", C.c_uint32)]


class ScaledSpec(C.Structure):
    """compeg_scaled_spec (include/compeg_hip.h, "Scaled decode"): the scale's denominator (2, 4 or 8), format, RGBA pitch."""
    _fields_ = [("denominator", C.c_uint32), ("format", C.c_uint32), ("pitch", C.c_uint32)]


class LevelsSpec(C.Structure):
    """compeg_levels_spec (include/compeg_hip.h, "Levels decode"): the order of a block's 64 values."""
    _fields_ = [("order", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class LevelsLayout(C.Structure):
    """compeg_levels_layout: where one image's blocks of quantised DCT coefficients (levels) lie, component by component."""
    _fields_ = [("components", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64 * 3), ("blocks_w", C.c_uint32 * 3),
                ("blocks_h", C.c_uint32 * 3), ("width_in_blocks", C.c_uint32 * 3), ("height_in_blocks", C.c_uint32 * 3),
                ("total_bytes", C.c_uint64)]


class CropSpec(C.Structure):
    """compeg_crop_spec (include/compeg_hip.h, "Cropped decode"): the rectangle in pixels of the image, format, RGBA pitch."""
    _fields_ = [("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32),
                ("pitch", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CropRegion(C.Structure):
    """compeg_crop_region (include/compeg_hip.h, "Cropped decode of a region list"): which rectangle of which image lies
    where in its slot."""
    _fields_ = [("image", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("dst_x", C.c_uint32), ("dst_y", C.c_uint32), ("reserved", C.c_uint32)]


class CropRegionsSpec(C.Structure):
    """compeg_crop_regions_spec: every region's slot in pixels, the format and the RGBA pitch."""
    _fields_ = [("slot_width", C.c_uint32), ("slot_height", C.c_uint32), ("format", C.c_uint32), ("pitch", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C compeg_amd/csrc` (hipcc --offload-arch=gfx950). compeg_amd has no fallback path.")
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, i = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    pvp, psz, pu32, pi = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    sig = {
        "compeg_last_error": (C.c_char_p, []),
        "compeg_version": (C.c_char_p, []),
        "compeg_gpu_open": (i, [i, pvp]),
        "compeg_gpu_from_stream": (i, [i, vp, pvp]),
        "compeg_gpu_retain": (None, [vp]),
        "compeg_gpu_release": (None, [vp]),
        "compeg_gpu_device": (i, [vp]),
        "compeg_gpu_name": (C.c_char_p, [vp]),
        "compeg_image_parse": (i, [vp, sz, i, pvp]),
        "compeg_image_parse_ext": (i, [vp, sz, i, C.c_uint, pvp]),
        "compeg_image_free": (None, [vp]),
        "compeg_image_width": (u32, [vp]),
        "compeg_image_height": (u32, [vp]),
        "compeg_image_parallelism": (u32, [vp]),
        "compeg_image_components": (u32, [vp]),
        "compeg_image_sampling": (i, [vp, pu32, pu32]),
        "compeg_image_metadata": (vp, [vp]),
        "compeg_image_huffman_l1": (vp, [vp]),
        "compeg_image_huffman_l2": (vp, [vp, psz]),
        "compeg_image_scan_range": (None, [vp, psz, psz]),
        "compeg_scanbuffer_new": (vp, []),
        "compeg_scanbuffer_free": (None, [vp]),
        "compeg_scanbuffer_process": (i, [vp, vp, sz, u32]),
        "compeg_scanbuffer_process_on_gpu": (i, [vp, vp, vp, sz, u32]),
        "compeg_scanbuffer_set_threads": (i, [vp, C.c_uint]),
        "compeg_scanbuffer_data": (vp, [vp, psz]),
        "compeg_scanbuffer_start_positions": (vp, [vp, psz]),
        "compeg_decoder_new": (i, [vp, pvp]),
        "compeg_decoder_free": (None, [vp]),
        "compeg_decoder_enqueue": (i, [vp, vp, vp, pi]),
        "compeg_decoder_start_decode": (i, [vp, vp, pvp]),
        "compeg_decoder_decode_blocking": (i, [vp, vp, pvp]),
        "compeg_decoder_last_warning": (C.c_char_p, [vp]),
        "compeg_decoder_last_stage_times": (C.c_int, [vp, vp]),
        "compeg_decoder_set_device_preprocess": (i, [vp, i]),
        "compeg_decoder_set_scan_threads": (i, [vp, C.c_uint]),
        "compeg_op_wait": (i, [vp]),
        "compeg_op_texture_changed": (i, [vp]),
        "compeg_op_free": (None, [vp]),
        "compeg_decoder_output": (i, [vp, pvp, pu32, pu32, psz]),
        "compeg_decoder_take_output": (i, [vp, pvp, pu32, pu32, psz]),
        "compeg_device_free": (None, [vp]),
        "compeg_decoder_read_output": (i, [vp, vp, u32, u32]),
        "compeg_decoder_read_coefficients": (i, [vp, vp, sz]),
        "compeg_batch_new": (i, [vp, pvp]),
        "compeg_batch_free": (None, [vp]),
        "compeg_batch_upload": (i, [vp, pvp, sz, i]),
        "compeg_batch_upload_jpegs": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_int, C.c_uint]),
        "compeg_batch_upload_jpegs_begin": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_int, C.c_uint]),
        "compeg_batch_upload_end": (i, [vp]),
        "compeg_batch_decode": (i, [vp, vp]),
        "compeg_batch_set_chunk": (i, [vp, u32]),
        "compeg_batch_set_device_preprocess": (i, [vp, i]),
        "compeg_batch_host_fallbacks": (sz, [vp]),
        "compeg_batch_wait": (i, [vp]),
        "compeg_batch_count": (sz, [vp]),
        "compeg_batch_output": (i, [vp, sz, pvp, pu32, pu32, psz]),
        "compeg_batch_read_output": (i, [vp, sz, vp]),
        "compeg_batch_algorithmic_bytes": (C.c_uint64, [vp]),
        "compeg_batch_pixels": (C.c_uint64, [vp]),
        "compeg_batch_timing": (i, [vp, i, pu32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "compeg_batch_set_timing": (i, [vp, i]),
        "compeg_batch_last_kernel": (i, [vp]),
        "compeg_host_feed_work": (i, [vp, vp, C.c_size_t, i, C.c_uint, i, i, C.POINTER(C.c_double)]),
        "compeg_host_alloc": (i, [C.c_size_t, C.POINTER(C.c_void_p)]),
        "compeg_host_free": (None, [vp]),
        "compeg_host_register": (i, [vp, C.c_size_t]),
        "compeg_host_unregister": (i, [vp]),
        "compeg_decoder_last_kernel": (i, [vp]),
        "compeg_tensor_shape": (i, [C.POINTER(TensorSpec), u32, u32, pu32, pu32, psz]),
        "compeg_decoder_pack_tensor": (i, [vp, C.POINTER(TensorSpec), vp, sz, vp]),
        "compeg_batch_pack_tensor": (i, [vp, C.POINTER(TensorSpec), vp, sz, vp]),
        "compeg_resized_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(ResizeSpec), u32, u32, C.POINTER(Rect), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_resized": (i, [vp, C.POINTER(TensorSpec), C.POINTER(ResizeSpec), C.POINTER(Rect), vp, sz, vp]),
        "compeg_batch_pack_tensor_resized": (i, [vp, C.POINTER(TensorSpec), C.POINTER(ResizeSpec), C.POINTER(Rect), vp, sz, vp]),
        "compeg_region_fit": (i, [u32, u32, u32, u32, C.c_uint, C.POINTER(Rect)]),
        "compeg_region_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(ResizeSpec), u32, u32, C.POINTER(Region), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_regions": (i, [vp, C.POINTER(TensorSpec), C.POINTER(ResizeSpec), C.POINTER(Region), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_batch_pack_tensor_regions": (i, [vp, C.POINTER(TensorSpec), C.POINTER(ResizeSpec), C.POINTER(Region), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_filtered_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(FilterSpec), u32, u32, C.POINTER(Region), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_filtered": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(Region), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_batch_pack_tensor_filtered": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(Region), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_image_orientation": (u32, [vp]),
        "compeg_batch_image_orientation": (i, [vp, sz, pu32]),
        "compeg_orient_rect": (i, [u32, u32, u32, C.POINTER(Rect), C.POINTER(Rect)]),
        "compeg_oriented_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(FilterSpec), u32, u32, C.POINTER(OrientedRegion), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_oriented": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_batch_pack_tensor_oriented": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_nhwc_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(NhwcSpec), u32, u32, C.POINTER(OrientedRegion), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_nhwc": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(NhwcSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_batch_pack_tensor_nhwc": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(NhwcSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_luma_tensor_shape": (i, [C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(LumaSpec), u32, u32, C.POINTER(OrientedRegion), pu32, pu32, psz]),
        "compeg_decoder_pack_tensor_luma": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(LumaSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_batch_pack_tensor_luma": (i, [vp, C.POINTER(TensorSpec), C.POINTER(FilterSpec), C.POINTER(LumaSpec), C.POINTER(OrientedRegion), sz, C.POINTER(C.c_float), vp, sz, vp]),
        "compeg_planes_shape": (i, [C.POINTER(PlanesSpec), u32, u32, u32, u32, u32, C.POINTER(PlanesLayout)]),
        "compeg_batch_decode_planes": (i, [vp, C.POINTER(PlanesSpec), vp, sz, vp]),
        "compeg_decoder_decode_planes": (i, [vp, vp, C.POINTER(PlanesSpec), vp, sz, vp]),
        "compeg_decoder_decode_planes_blocking": (i, [vp, vp, C.POINTER(PlanesSpec), vp, sz]),
        "compeg_reduced_shape": (i, [C.POINTER(ReducedSpec), u32, u32, pu32, pu32, pu32, C.POINTER(C.c_uint64)]),
        "compeg_batch_decode_reduced": (i, [vp, C.POINTER(ReducedSpec), vp, sz, vp]),
        "compeg_decoder_decode_reduced": (i, [vp, vp, C.POINTER(ReducedSpec), vp, sz, vp]),
        "compeg_decoder_decode_reduced_blocking": (i, [vp, vp, C.POINTER(ReducedSpec), vp, sz]),
        "compeg_scaled_shape": (i, [C.POINTER(ScaledSpec), u32, u32, pu32, pu32, pu32, C.POINTER(C.c_uint64)]),
        "compeg_batch_decode_scaled": (i, [vp, C.POINTER(ScaledSpec), vp, sz, vp]),
        "compeg_decoder_decode_scaled": (i, [vp, vp, C.POINTER(ScaledSpec), vp, sz, vp]),
        "compeg_decoder_decode_scaled_blocking": (i, [vp, vp, C.POINTER(ScaledSpec), vp, sz]),
        "compeg_levels_shape": (i, [C.POINTER(LevelsSpec), u32, u32, u32, u32, u32, C.POINTER(LevelsLayout)]),
        "compeg_batch_decode_levels": (i, [vp, C.POINTER(LevelsSpec), vp, sz, vp]),
        "compeg_decoder_decode_levels": (i, [vp, vp, C.POINTER(LevelsSpec), vp, sz, vp]),
        "compeg_decoder_decode_levels_blocking": (i, [vp, vp, C.POINTER(LevelsSpec), vp, sz]),
        "compeg_image_quant_table": (i, [vp, u32, C.POINTER(C.c_uint16), u32]),
        "compeg_batch_quant_table": (i, [vp, sz, u32, C.POINTER(C.c_uint16), u32]),
        "compeg_crop_shape": (i, [C.POINTER(CropSpec), u32, u32, pu32, C.POINTER(C.c_uint64)]),
        "compeg_batch_decode_cropped": (i, [vp, C.POINTER(CropSpec), vp, sz, vp]),
        "compeg_decoder_decode_cropped": (i, [vp, vp, C.POINTER(CropSpec), vp, sz, vp]),
        "compeg_decoder_decode_cropped_blocking": (i, [vp, vp, C.POINTER(CropSpec), vp, sz]),
        "compeg_crop_regions_shape": (i, [C.POINTER(CropRegionsSpec), pu32, C.POINTER(C.c_uint64)]),
        "compeg_crop_region_check": (i, [C.POINTER(CropRegionsSpec), u32, u32, C.POINTER(CropRegion)]),
        "compeg_batch_decode_cropped_regions": (i, [vp, C.POINTER(CropRegionsSpec), C.POINTER(CropRegion), sz, vp, sz, vp]),
        "compeg_decoder_decode_cropped_regions": (i, [vp, vp, C.POINTER(CropRegionsSpec), C.POINTER(CropRegion), sz, vp, sz, vp]),
        "compeg_decoder_decode_cropped_regions_blocking": (i, [vp, vp, C.POINTER(CropRegionsSpec), C.POINTER(CropRegion), sz, vp, sz]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("COMPEG_LIB") and not hasattr(L, name):
            continue           # (A/B runs against an older build: it may lack the newest entry points)
        fn = getattr(L, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype, fn.argtypes = res, args
    L._signatures = sig
    return L


lib = _load()


def check(rc):
    if rc != OK:
        raise Error(lib.compeg_last_error().decode("utf-8", "replace"), rc)
