"""compeg_amd -- host-side mirror of the reference's public API over the C ABI of
libcompeg_hip.so (hand-written gfx950 kernels).

Same names, argument meaning and error behaviour as SludgePhD/Compeg's Rust
crate (src/lib.rs), so tests read like the reference's own:

    gpu = Gpu.open()
    decoder = Decoder(gpu)
    data = ImageData(jpeg_bytes)          # raises compeg_amd.Error like ImageData::new -> Err
    op = decoder.decode_blocking(data)
    rgba = decoder.read_texture(data.width(), data.height())

Everything that computes runs in the native library; this package only moves
handles around.  There is no CPU fallback.
"""
import ctypes as C

import numpy as np

from ._lib import (CropRegion, CropRegionsSpec, CropSpec, E_COUNT_MISMATCH, E_HIP, E_INVALID_ARG, E_MALFORMED, E_UNSUPPORTED, L1_BYTES,
                   LIB_PATH, METADATA_BYTES, Error, FilterSpec, LumaSpec, NhwcSpec, OrientedRegion, PlanesLayout, PlanesSpec, Rect, ReducedSpec, Region, ResizeSpec,
                   LevelsLayout, LevelsSpec, ScaledSpec, TensorSpec, check,
                   lib)

__all__ = ["Gpu", "Decoder", "DecodeOp", "ImageData", "ScanBuffer", "Batch", "Texture", "Error", "HostBuffer", "JpegList",
           "host_register", "host_unregister", "version", "LIB_PATH", "tensor_shape", "TENSOR_DTYPES", "TENSOR_ORDERS",
           "resized_tensor_shape", "RESIZE_FILTERS", "ResizeSpec", "Rect", "Region", "FIT_ALIGNS", "region_fit",
           "region_tensor_shape", "FILTER_KERNELS", "FilterSpec", "filtered_tensor_shape", "ORIENTATIONS", "OrientedRegion",
           "orient_rect", "oriented_tensor_shape", "NhwcSpec", "nhwc_tensor_shape", "LumaSpec", "LUMA_WEIGHTS",
           "luma_tensor_shape", "PlanesSpec", "PlanesLayout", "PLANES_FORMATS", "PLANES_CHROMA", "planes_shape",
           "ReducedSpec", "REDUCED_FORMATS", "reduced_shape", "CropSpec", "CROP_FORMATS", "crop_shape",
           "ScaledSpec", "SCALED_FORMATS", "scaled_shape", "DECODE_KERNEL_NAMES",
           "LevelsSpec", "LevelsLayout", "LEVELS_ORDERS", "levels_shape", "LAST_KERNEL_NAMES",
           "CropRegion", "CropRegionsSpec", "crop_regions_shape"]


# compeg_decoder_last_kernel / compeg_batch_last_kernel (include/compeg_hip.h: COMPEG_KERNEL_*).  KERNEL_NAMES: the RGBA
# routes and the planes decode, ten names (tests/test_planes_stream.py pins the count); ALL_KERNEL_NAMES: every value
# last_kernel() can give, the reduced decode's (COMPEG_KERNEL_REDUCED = 10) and the cropped decode's
# (COMPEG_KERNEL_CROPPED = 11) behind them, twelve names (tests/test_crop_stream.py pins the count); DECODE_KERNEL_NAMES:
# those and the scaled decode's (COMPEG_KERNEL_SCALED = 12), thirteen names (tests/test_scaled_stream.py pins the count);
# LAST_KERNEL_NAMES: those and the levels decode's (COMPEG_KERNEL_LEVELS = 13), what both last_kernel() methods index.
KERNEL_NAMES = ("none", "fused", "pair", "coop_team", "generic", "split", "fused_layout", "fused_stream", "walk_mcu", "planes")
ALL_KERNEL_NAMES = KERNEL_NAMES + ("reduced", "cropped")
DECODE_KERNEL_NAMES = ALL_KERNEL_NAMES + ("scaled",)
LAST_KERNEL_NAMES = DECODE_KERNEL_NAMES + ("levels",)


def version():
    return lib.compeg_version().decode()


# Tensor output (include/compeg_hip.h: COMPEG_TENSOR_*): element types and plane orders by name
TENSOR_DTYPES = {"u8": 0, "f16": 1, "bf16": 2, "f32": 3}
TENSOR_ORDERS = {"rgb": 0, "bgr": 1}


def _tensor_spec(dtype, downscale, scale, bias, order):
    """compeg_tensor_spec from names (or the header's numbers, which the library checks)."""
    spec = TensorSpec()
    if isinstance(dtype, str) and dtype not in TENSOR_DTYPES:
        raise Error(f"unknown tensor dtype {dtype!r} (one of {', '.join(TENSOR_DTYPES)})")
    if isinstance(order, str) and order not in TENSOR_ORDERS:
        raise Error(f"unknown tensor order {order!r} (one of {', '.join(TENSOR_ORDERS)})")
    spec.dtype = TENSOR_DTYPES[dtype] if isinstance(dtype, str) else dtype
    spec.order = TENSOR_ORDERS[order] if isinstance(order, str) else order
    spec.downscale, spec.reserved = downscale, 0
    spec.scale[:] = [float(x) for x in scale]
    spec.bias[:] = [float(x) for x in bias]
    return spec


def tensor_shape(width, height, dtype="f16", downscale=1):
    """((3, oh, ow), bytes) of one WxH image's tensor (compeg_tensor_shape; no device needed)."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    ow, oh, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_tensor_shape(C.byref(spec), width, height, C.byref(ow), C.byref(oh), C.byref(nbytes)))
    return (3, oh.value, ow.value), nbytes.value


# Resized tensor output (include/compeg_hip.h: COMPEG_RESIZE_*): filters by name
RESIZE_FILTERS = {"nearest": 0, "bilinear": 1}


RESIZE_ANTIALIAS = 0x100   # COMPEG_RESIZE_ANTIALIAS: a flag beside the filter, for "bilinear" only (the library checks)


def _resize_spec(size, filter, antialias=False):
    """compeg_resize_spec from size = (ow, oh), a filter's name (or the header's number, which the library checks) and the
    antialias flag."""
    if isinstance(filter, str) and filter not in RESIZE_FILTERS:
        raise Error(f"unknown resize filter {filter!r} (one of {', '.join(RESIZE_FILTERS)})")
    ow, oh = size
    spec = ResizeSpec()
    spec.out_width, spec.out_height = ow, oh
    spec.filter = (RESIZE_FILTERS[filter] if isinstance(filter, str) else filter) | (RESIZE_ANTIALIAS if antialias else 0)
    spec.reserved = 0
    return spec


def _rect(crop):
    x, y, w, h = crop
    return Rect(x, y, w, h)


def resized_tensor_shape(width, height, size, dtype="f16", downscale=1, filter="bilinear", crop=None, antialias=False):
    """((3, oh, ow), bytes, (ph, pw)) of one WxH image's resized tensor: size = (ow, oh), crop = (x, y, w, h) or None for
    the whole image, (ph, pw) the extent of the block-averaged crop that the filter reads (compeg_resized_tensor_shape;
    no device needed).  antialias: as in pack_tensor_resized; its ratio limit (64 either way) is checked here too."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    resize = _resize_spec(size, filter, antialias)
    rect = _rect(crop) if crop is not None else None
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_resized_tensor_shape(C.byref(spec), C.byref(resize), width, height, C.byref(rect) if rect is not None else None,
                                          C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (3, resize.out_height, resize.out_width), nbytes.value, (ph.value, pw.value)


# Region tensor output (include/compeg_hip.h: COMPEG_FIT_*): placements by name
FIT_ALIGNS = {"center": 0, "top_left": 1}


def _region(region):
    """compeg_region from (image, src or None, dst or None), rectangles as (x, y, w, h); or a Region as it is."""
    if isinstance(region, Region):
        return region
    image, src, dst = region
    r = Region()
    r.image, r.reserved = image, 0
    r.src = src if isinstance(src, Rect) else (_rect(src) if src is not None else Rect(0, 0, 0, 0))
    r.dst = dst if isinstance(dst, Rect) else (_rect(dst) if dst is not None else Rect(0, 0, 0, 0))
    return r


def _regions(regions):
    regions = list(regions)
    return (Region * max(len(regions), 1))(*[_region(r) for r in regions]), len(regions)


def _pad(pad):
    return (C.c_float * 3)(*[float(x) for x in pad]) if pad is not None else None


def region_fit(src_size, out_size, align="center"):
    """(dx, dy, dw, dh): the rectangle of out_size = (ow, oh) that a crop of src_size = (w, h) pixels fills when it is
    fitted with its aspect ratio kept, centred or ("top_left") at the origin (compeg_region_fit; no device needed)."""
    if isinstance(align, str) and align not in FIT_ALIGNS:
        raise Error(f"unknown fit align {align!r} (one of {', '.join(FIT_ALIGNS)})")
    rect = Rect()
    check(lib.compeg_region_fit(src_size[0], src_size[1], out_size[0], out_size[1], FIT_ALIGNS[align] if isinstance(align, str) else align,
                                C.byref(rect)))
    return rect.x, rect.y, rect.width, rect.height


def region_tensor_shape(width, height, size, region=None, dtype="f16", downscale=1, filter="bilinear", antialias=False):
    """((3, oh, ow), bytes, (ph, pw)) of one slot of a region pack: region = (image, src or None, dst or None) of a WxH
    image (None: the whole image into the whole output), checked as the pack calls check it, all but the image index
    (compeg_region_tensor_shape; no device needed).  The antialias limit is taken against dst's extent."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    resize = _resize_spec(size, filter, antialias)
    r = _region(region) if region is not None else None
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_region_tensor_shape(C.byref(spec), C.byref(resize), width, height, C.byref(r) if r is not None else None,
                                         C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (3, resize.out_height, resize.out_width), nbytes.value, (ph.value, pw.value)


# Filtered tensor output (include/compeg_hip.h: COMPEG_FILTER_*): resampling kernels by name
FILTER_KERNELS = {"box": 0, "triangle": 1, "bicubic": 2, "lanczos3": 3}


def _filter_spec(size, kernel):
    """compeg_filter_spec from size = (ow, oh) and a kernel's name (or the header's number, which the library checks)."""
    if isinstance(kernel, str) and kernel not in FILTER_KERNELS:
        raise Error(f"unknown filter kernel {kernel!r} (one of {', '.join(FILTER_KERNELS)})")
    spec = FilterSpec()
    spec.out_width, spec.out_height = size
    spec.kernel, spec.reserved = FILTER_KERNELS[kernel] if isinstance(kernel, str) else kernel, 0
    return spec


def filtered_tensor_shape(width, height, size, region=None, kernel="bicubic", dtype="f16", downscale=1):
    """((3, oh, ow), bytes, (ph, pw)) of one slot of a filtered pack: region_tensor_shape for pack_tensor_filtered, the
    kernel's tap limit (box reduces by 128 at the most, triangle 64, bicubic 32, lanczos3 21) taken against dst's extent
    (compeg_filtered_tensor_shape; no device needed)."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    filter = _filter_spec(size, kernel)
    r = _region(region) if region is not None else None
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_filtered_tensor_shape(C.byref(spec), C.byref(filter), width, height, C.byref(r) if r is not None else None,
                                           C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (3, filter.out_height, filter.out_width), nbytes.value, (ph.value, pw.value)


# Oriented tensor output (include/compeg_hip.h): the EXIF orientation values by name -- what has to be done to the stored
# raster to see it upright
ORIENTATIONS = {"normal": 1, "mirror": 2, "rotate180": 3, "flip": 4, "transpose": 5, "rotate90": 6, "transverse": 7, "rotate270": 8}


def _orientation(orientation):
    """0..8 from a name of ORIENTATIONS, "exif" (0: the image's own tag) or the number itself (which the library checks)."""
    if isinstance(orientation, str):
        if orientation == "exif":
            return 0
        if orientation not in ORIENTATIONS:
            raise Error(f"unknown orientation {orientation!r} (\"exif\" or one of {', '.join(ORIENTATIONS)})")
        return ORIENTATIONS[orientation]
    return orientation


def _oriented_regions(regions, orientation):
    """compeg_oriented_region list from (image, src, dst) or (image, src, dst, orientation) tuples (or OrientedRegions as they
    are); `orientation` is for the regions that carry none."""
    out = []
    for region in regions:
        if not isinstance(region, OrientedRegion):
            r = OrientedRegion()
            r.region = _region(tuple(region)[:3])
            r.orientation, r.reserved = _orientation(region[3] if len(region) > 3 else orientation), 0
            region = r
        out.append(region)
    return (OrientedRegion * max(len(out), 1))(*out), len(out)


def orient_rect(upright_size, orientation, rect):
    """(x, y, w, h) in the stored raster of rect = (x, y, w, h) of the upright image of upright_size = (w, h): what goes
    into a region's src when the crop was chosen on the upright image (compeg_orient_rect; no device needed)."""
    stored = Rect()
    check(lib.compeg_orient_rect(upright_size[0], upright_size[1], _orientation(orientation), C.byref(_rect(rect)), C.byref(stored)))
    return stored.x, stored.y, stored.width, stored.height


def oriented_tensor_shape(width, height, size, region=None, orientation=1, kernel="bicubic", dtype="f16", downscale=1):
    """((3, oh, ow), bytes, (ph, pw)) of one slot of an oriented pack: filtered_tensor_shape for pack_tensor_oriented --
    width x height the stored raster, size = (ow, oh) the upright slot, region = (image, src, dst[, orientation]); the
    tap limit is taken along the stored axes (compeg_oriented_tensor_shape; no device needed; "exif" counts as 1)."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    filter = _filter_spec(size, kernel)
    list_, _ = _oriented_regions([region if region is not None else (0, None, None)], orientation)
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_oriented_tensor_shape(C.byref(spec), C.byref(filter), width, height, list_, C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (3, filter.out_height, filter.out_width), nbytes.value, (ph.value, pw.value)


def _device_range(dst):
    """(address, bytes) of a pack destination: such a pair; a tensor-like object (data_ptr / numel / element_size);
    or anything with __cuda_array_interface__ (contiguous).  No framework is imported for it."""
    if isinstance(dst, tuple) and len(dst) == 2:
        return int(dst[0]), int(dst[1])
    if hasattr(dst, "data_ptr") and hasattr(dst, "numel") and hasattr(dst, "element_size"):
        if hasattr(dst, "is_contiguous") and not dst.is_contiguous():
            raise Error("pack_tensor: the destination must be contiguous")
        return int(dst.data_ptr()), int(dst.numel()) * int(dst.element_size())
    cai = getattr(dst, "__cuda_array_interface__", None)
    if cai is not None:
        itemsize = np.dtype(cai["typestr"]).itemsize
        shape = tuple(cai["shape"])
        strides = cai.get("strides")
        tight = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) * itemsize for i in range(len(shape)))
        if strides is not None and tuple(strides) != tight:
            raise Error("pack_tensor: the destination must be contiguous")
        return int(cai["data"][0]), int(np.prod(shape, dtype=np.int64)) * itemsize
    raise Error("pack_tensor: dst is neither (address, nbytes), a tensor, nor a __cuda_array_interface__ object")


def _nhwc_spec(channels, fill):
    """compeg_nhwc_spec; the library checks the values."""
    spec = NhwcSpec()
    spec.channels, spec.fill = channels, float(fill)
    spec.reserved[0] = spec.reserved[1] = 0
    return spec


def nhwc_tensor_shape(width, height, size, region=None, orientation=1, channels=3, fill=0.0, kernel="bicubic", dtype="f16", downscale=1):
    """((oh, ow, C), bytes, (ph, pw)) of one slot of a channels-last pack: oriented_tensor_shape for pack_tensor_nhwc, with
    C = channels, 3 or 4 (compeg_nhwc_tensor_shape; no device needed)."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    filter = _filter_spec(size, kernel)
    nhwc = _nhwc_spec(channels, fill)
    list_, _ = _oriented_regions([region if region is not None else (0, None, None)], orientation)
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_nhwc_tensor_shape(C.byref(spec), C.byref(filter), C.byref(nhwc), width, height, list_, C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (filter.out_height, filter.out_width, nhwc.channels), nbytes.value, (ph.value, pw.value)


def _nhwc_device_range(dst, size, channels):
    """(address, bytes) of a channels-last pack destination of size = (ow, oh) and `channels`: _device_range's forms, with a
    tensor taken by its shape and strides instead of is_contiguous() -- it must cover its memory densely, without overlap,
    and be [.., oh, ow, C] row-major or [.., C, oh, ow] with channels-last strides (what torch.channels_last gives).  A
    planar tensor is an error here, not a scrambled image.  No framework is imported for it."""
    if isinstance(dst, tuple) and len(dst) == 2:
        return int(dst[0]), int(dst[1])
    if hasattr(dst, "data_ptr") and hasattr(dst, "stride") and hasattr(dst, "shape") and hasattr(dst, "element_size"):
        address, itemsize = int(dst.data_ptr()), int(dst.element_size())
        shape, strides = tuple(int(n) for n in dst.shape), tuple(int(n) for n in dst.stride())
    else:
        cai = getattr(dst, "__cuda_array_interface__", None)
        if cai is None:
            raise Error("pack_tensor_nhwc: dst is neither (address, nbytes), a tensor, nor a __cuda_array_interface__ object")
        address, itemsize = int(cai["data"][0]), np.dtype(cai["typestr"]).itemsize
        shape = tuple(int(n) for n in cai["shape"])
        if cai.get("strides") is None:
            strides = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(len(shape)))
        else:
            if any(int(b) % itemsize for b in cai["strides"]):
                raise Error("pack_tensor_nhwc: the destination's strides are no multiples of its element size")
            strides = tuple(int(b) // itemsize for b in cai["strides"])
    ow, oh = size
    what = f"shape {shape} with strides {strides}"
    if len(shape) < 3 or any(n < 1 for n in shape):
        raise Error(f"pack_tensor_nhwc: the destination has {what}, neither [.., {oh}, {ow}, {channels}] nor [.., {channels}, {oh}, {ow}]")
    # dense and without overlap: by ascending stride, each one is the extent of what lies below it (an axis of 1: any stride)
    below = 1
    for stride, n in sorted((s, n) for s, n in zip(strides, shape) if n != 1):
        if stride != below:
            raise Error(f"pack_tensor_nhwc: the destination ({what}) does not cover its memory densely (a slice, an expanded or an overlapping view)")
        below *= n
    lead = shape[:-3]
    outer = [int(np.prod(lead[i + 1:], dtype=np.int64)) * oh * ow * channels for i in range(len(lead))]

    def laid(inner):
        return all(n == 1 or s == want for n, s, want in zip(shape, strides, outer + inner))
    last = shape[-3:] == (oh, ow, channels) and laid([ow * channels, channels, 1])
    first = shape[-3:] == (channels, oh, ow) and laid([1, ow * channels, channels])
    if not (last or first):
        planar = shape[-3:] == (channels, oh, ow)
        raise Error(f"pack_tensor_nhwc: the destination has {what}: " +
                    ("planar memory -- give it channels-last strides (torch: memory_format=torch.channels_last)" if planar else
                     f"neither [.., {oh}, {ow}, {channels}] row-major nor [.., {channels}, {oh}, {ow}] with channels-last strides"))
    return address, below * itemsize


# Luma tensor output (include/compeg_hip.h: compeg_luma_spec): the weights of R, G and B by name, in 1/65536
LUMA_WEIGHTS = {"bt601": (19595, 38470, 7471), "bt709": (13933, 46871, 4732), "r": (65536, 0, 0), "g": (0, 65536, 0), "b": (0, 0, 65536)}


def _luma_spec(weights):
    """compeg_luma_spec from a name of LUMA_WEIGHTS or three integers (which the library checks)."""
    if isinstance(weights, LumaSpec):
        return weights
    if isinstance(weights, str):
        if weights not in LUMA_WEIGHTS:
            raise Error(f"unknown luma weights {weights!r} (one of {', '.join(LUMA_WEIGHTS)}, or three integers with a sum of 65536)")
        weights = LUMA_WEIGHTS[weights]
    weights = tuple(weights)
    if len(weights) != 3 or any(int(w) != w or not 0 <= w <= 0xffffffff for w in weights):
        raise Error(f"luma weights {weights!r} are not three integers (each 0..65536, their sum 65536)")
    spec = LumaSpec()
    spec.weights[:] = [int(w) for w in weights]
    spec.reserved = 0
    return spec


def _luma_pad(pad):
    return C.pointer(C.c_float(float(pad))) if pad is not None else None


def luma_tensor_shape(width, height, size, region=None, orientation=1, weights="bt601", kernel="bicubic", dtype="f16", downscale=1):
    """((1, oh, ow), bytes, (ph, pw)) of one slot of a luma pack: oriented_tensor_shape for pack_tensor_luma, one channel
    a slot (compeg_luma_tensor_shape; no device needed)."""
    spec = _tensor_spec(dtype, downscale, (1, 1, 1), (0, 0, 0), "rgb")
    filter = _filter_spec(size, kernel)
    luma = _luma_spec(weights)
    list_, _ = _oriented_regions([region if region is not None else (0, None, None)], orientation)
    pw, ph, nbytes = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(lib.compeg_luma_tensor_shape(C.byref(spec), C.byref(filter), C.byref(luma), width, height, list_, C.byref(pw), C.byref(ph), C.byref(nbytes)))
    return (1, filter.out_height, filter.out_width), nbytes.value, (ph.value, pw.value)


def _luma_device_range(dst, size, count):
    """(address, bytes) of a luma pack destination of `count` slots of size = (ow, oh): _device_range's forms, with a tensor
    taken by its shape and strides -- it must cover its memory densely, in row-major order, be [.., 1, oh, ow],
    [.., oh, ow, 1] or [.., oh, ow], and hold `count` slots: [N, 3, oh, ow] is 3 N slots, so a three-channel tensor, like a
    slice or another extent, is an error here, not a scrambled image.  No framework is imported for it."""
    if isinstance(dst, tuple) and len(dst) == 2:
        return int(dst[0]), int(dst[1])
    if hasattr(dst, "data_ptr") and hasattr(dst, "stride") and hasattr(dst, "shape") and hasattr(dst, "element_size"):
        address, itemsize = int(dst.data_ptr()), int(dst.element_size())
        shape, strides = tuple(int(n) for n in dst.shape), tuple(int(n) for n in dst.stride())
    else:
        cai = getattr(dst, "__cuda_array_interface__", None)
        if cai is None:
            raise Error("pack_tensor_luma: dst is neither (address, nbytes), a tensor, nor a __cuda_array_interface__ object")
        address, itemsize = int(cai["data"][0]), np.dtype(cai["typestr"]).itemsize
        shape = tuple(int(n) for n in cai["shape"])
        if cai.get("strides") is None:
            strides = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) for i in range(len(shape)))
        else:
            if any(int(b) % itemsize for b in cai["strides"]):
                raise Error("pack_tensor_luma: the destination's strides are no multiples of its element size")
            strides = tuple(int(b) // itemsize for b in cai["strides"])
    ow, oh = size
    what = f"shape {shape} with strides {strides}"
    forms = f"[.., 1, {oh}, {ow}], [.., {oh}, {ow}, 1] or [.., {oh}, {ow}]"
    if any(n < 1 for n in shape):
        raise Error(f"pack_tensor_luma: the destination has {what}, none of {forms}")
    # the slot's axes, whichever form names them; what is in front of them counts slots
    if len(shape) >= 3 and shape[-3:] == (1, oh, ow):
        lead = shape[:-3]
    elif len(shape) >= 3 and shape[-3:] == (oh, ow, 1):
        lead = shape[:-3]
    elif len(shape) >= 2 and shape[-2:] == (oh, ow):
        lead = shape[:-2]
    else:
        raise Error(f"pack_tensor_luma: the destination has {what}, none of {forms} (one channel a slot)")
    # row-major and dense: an axis's stride is the extent of the axes behind it (an axis of 1: any stride)
    below = 1
    for n, stride in zip(reversed(shape), reversed(strides)):
        if n != 1 and stride != below:
            raise Error(f"pack_tensor_luma: the destination ({what}) does not cover its memory densely in row-major order "
                        "(a slice, an expanded or a permuted view)")
        below *= n
    slots = int(np.prod(lead, dtype=np.int64))
    if slots != count:
        raise Error(f"pack_tensor_luma: the destination ({what}) holds {slots} slots of one channel, the call packs {count} "
                    "(a luma pack writes one channel a slot: no three-channel tensor)")
    return address, slots * oh * ow * itemsize


# Planar YCbCr output (include/compeg_hip.h: COMPEG_PLANES_*, COMPEG_CHROMA_*): formats and chroma options by name
PLANES_FORMATS = {"planar": 0, "semiplanar": 1, "yuyv": 2, "uyvy": 3}
PLANES_CHROMA = {"coded": 0, "420": 1}


def _planes_spec(format, chroma, pitch):
    """compeg_planes_spec from names (or the header's numbers, which the library checks); pitch: None (tight), one
    number (the luma pitch) or (luma_pitch, chroma_pitch), 0 = tight."""
    if isinstance(format, str) and format not in PLANES_FORMATS:
        raise Error(f"unknown planes format {format!r} (one of {', '.join(PLANES_FORMATS)})")
    if isinstance(chroma, str) and chroma not in PLANES_CHROMA:
        raise Error(f"unknown planes chroma option {chroma!r} (one of {', '.join(PLANES_CHROMA)})")
    spec = PlanesSpec()
    spec.format = PLANES_FORMATS[format] if isinstance(format, str) else format
    spec.chroma = PLANES_CHROMA[chroma] if isinstance(chroma, str) else chroma
    if pitch is None:
        pitch = (0, 0)
    elif not isinstance(pitch, (tuple, list)):
        pitch = (pitch, 0)
    spec.luma_pitch, spec.chroma_pitch = int(pitch[0]), int(pitch[1])
    return spec


def planes_shape(width, height, sampling=(2, 1), components=3, format="planar", chroma="coded", pitch=None):
    """(planes, total_bytes) of one width x height image whose luma is sampled `sampling` (ImageData.sampling()) --
    compeg_planes_shape; no device needed.  planes: a tuple of dicts offset / pitch / row_bytes / width / height, one per
    plane, in the order they lie; the caller makes its views of a u8 destination from them."""
    spec = _planes_spec(format, chroma, pitch)
    lay = PlanesLayout()
    check(lib.compeg_planes_shape(C.byref(spec), width, height, components, sampling[0], sampling[1], C.byref(lay)))
    planes = tuple({"offset": lay.offset[p], "pitch": lay.pitch[p], "row_bytes": lay.row_bytes[p], "width": lay.width[p],
                    "height": lay.height[p]} for p in range(lay.planes))
    return planes, lay.total_bytes


# Reduced-size decode (include/compeg_hip.h: COMPEG_REDUCED_*): formats by name
REDUCED_FORMATS = {"rgba": 0, "rgb_planar": 1}


def _reduced_spec(format, pitch, denominator=8):
    """compeg_reduced_spec from a name (or the header's number, which the library checks); pitch: None or 0 = tight."""
    if isinstance(format, str) and format not in REDUCED_FORMATS:
        raise Error(f"unknown reduced format {format!r} (one of {', '.join(REDUCED_FORMATS)})")
    spec = ReducedSpec()
    spec.denominator = denominator
    spec.format = REDUCED_FORMATS[format] if isinstance(format, str) else format
    spec.pitch = int(pitch or 0)
    return spec


def reduced_shape(width, height, format="rgba", pitch=None):
    """(ow, oh, pitch, total_bytes) of the 1/8-scale decode of one width x height image -- compeg_reduced_shape; no
    device needed.  ow x oh = ceil(width / 8) x ceil(height / 8); "rgba": rows of 4 ow bytes at `pitch` (a multiple of 4,
    None = tight); "rgb_planar": a tight [3, oh, ow] u8 block."""
    spec = _reduced_spec(format, pitch)
    ow, oh, pt, total = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    check(lib.compeg_reduced_shape(C.byref(spec), width, height, C.byref(ow), C.byref(oh), C.byref(pt), C.byref(total)))
    return ow.value, oh.value, pt.value, total.value


# Scaled decode (include/compeg_hip.h: COMPEG_SCALED_*): formats by name
SCALED_FORMATS = {"rgba": 0, "rgb_planar": 1}


def _scaled_spec(denominator, format, pitch):
    """compeg_scaled_spec from a name (or the header's number, which the library checks, as it checks the denominator);
    pitch: None or 0 = tight."""
    if isinstance(format, str) and format not in SCALED_FORMATS:
        raise Error(f"unknown scaled format {format!r} (one of {', '.join(SCALED_FORMATS)})")
    spec = ScaledSpec()
    spec.denominator = denominator
    spec.format = SCALED_FORMATS[format] if isinstance(format, str) else format
    spec.pitch = int(pitch or 0)
    return spec


def scaled_shape(width, height, denominator, format="rgba", pitch=None):
    """(ow, oh, pitch, total_bytes) of the decode of one width x height image at 1 / denominator (2, 4 or 8) --
    compeg_scaled_shape; no device needed.  ow x oh = ceil(width / denominator) x ceil(height / denominator); "rgba": rows
    of 4 ow bytes at `pitch` (a multiple of 4, None = tight); "rgb_planar": a tight [3, oh, ow] u8 block."""
    spec = _scaled_spec(denominator, format, pitch)
    ow, oh, pt, total = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    check(lib.compeg_scaled_shape(C.byref(spec), width, height, C.byref(ow), C.byref(oh), C.byref(pt), C.byref(total)))
    return ow.value, oh.value, pt.value, total.value


# Levels decode: quantised DCT coefficients (include/compeg_hip.h: COMPEG_LEVELS_*): orders by name
LEVELS_ORDERS = {"zigzag": 0, "natural": 1}


def _levels_order(order):
    if isinstance(order, str) and order not in LEVELS_ORDERS:
        raise Error(f"unknown levels order {order!r} (one of {', '.join(LEVELS_ORDERS)})")
    return LEVELS_ORDERS[order] if isinstance(order, str) else order


def _levels_spec(order):
    """compeg_levels_spec from a name (or the header's number, which the library checks)."""
    spec = LevelsSpec()
    spec.order = _levels_order(order)
    return spec


def levels_shape(width, height, sampling=(2, 1), components=3, order="zigzag"):
    """(components, total_bytes) of the quantised DCT coefficients (levels) of one width x height image whose luma is
    sampled `sampling` (ImageData.sampling()) -- compeg_levels_shape; no device needed.  components: a tuple of dicts
    offset / blocks_w / blocks_h / width_in_blocks / height_in_blocks, one per component: int16[blocks_h][blocks_w][64]
    from `offset` bytes on, whole MCUs, of which the top-left width_in_blocks x height_in_blocks carry image samples."""
    spec = _levels_spec(order)
    lay = LevelsLayout()
    check(lib.compeg_levels_shape(C.byref(spec), width, height, components, sampling[0], sampling[1], C.byref(lay)))
    comps = tuple({"offset": lay.offset[c], "blocks_w": lay.blocks_w[c], "blocks_h": lay.blocks_h[c],
                   "width_in_blocks": lay.width_in_blocks[c], "height_in_blocks": lay.height_in_blocks[c]}
                  for c in range(lay.components))
    return comps, lay.total_bytes


# Cropped decode (include/compeg_hip.h: COMPEG_CROP_*): formats by name
CROP_FORMATS = {"rgba": 0, "rgb_planar": 1}


def _crop_spec(rect, format, pitch):
    """compeg_crop_spec from a rectangle (x, y, width, height) in pixels of the image and a format's name (or the header's
    number, which the library checks); pitch: None or 0 = tight."""
    if isinstance(format, str) and format not in CROP_FORMATS:
        raise Error(f"unknown crop format {format!r} (one of {', '.join(CROP_FORMATS)})")
    spec = CropSpec()
    spec.x, spec.y, spec.width, spec.height = (int(v) for v in rect)
    spec.format = CROP_FORMATS[format] if isinstance(format, str) else format
    spec.pitch = int(pitch or 0)
    return spec


def crop_shape(width, height, rect, format="rgba", pitch=None):
    """(pitch, total_bytes) of the cropped decode of rect = (x, y, w, h) out of one width x height image --
    compeg_crop_shape; no device needed.  The rectangle must be non-empty and inside the image.  "rgba": rows of 4 w bytes
    at `pitch` (a multiple of 4, None = tight); "rgb_planar": a tight [3, h, w] u8 block."""
    spec = _crop_spec(rect, format, pitch)
    pt, total = C.c_uint32(), C.c_uint64()
    check(lib.compeg_crop_shape(C.byref(spec), width, height, C.byref(pt), C.byref(total)))
    return pt.value, total.value


def _crop_region(region):
    """compeg_crop_region from (image, (x, y, w, h)), (image, (x, y, w, h), (dst_x, dst_y)) or a CropRegion as it is."""
    if isinstance(region, CropRegion):
        return region
    if not isinstance(region, (tuple, list)) or len(region) not in (2, 3) or len(region[1]) != 4 or (len(region) == 3 and len(region[2]) != 2):
        raise Error(f"crop regions: {region!r} is neither (image, (x, y, w, h)), (image, (x, y, w, h), (dst_x, dst_y)) nor a CropRegion")
    r = CropRegion()
    r.image = int(region[0])
    r.x, r.y, r.width, r.height = (int(v) for v in region[1])
    r.dst_x, r.dst_y = (int(v) for v in region[2]) if len(region) == 3 else (0, 0)
    r.reserved = 0
    return r


def _crop_regions_spec(slot, format, pitch):
    """compeg_crop_regions_spec from the slot (width, height) in pixels and a format's name (or the header's number, which
    the library checks); pitch: None or 0 = tight."""
    if isinstance(format, str) and format not in CROP_FORMATS:
        raise Error(f"unknown crop format {format!r} (one of {', '.join(CROP_FORMATS)})")
    spec = CropRegionsSpec()
    spec.slot_width, spec.slot_height = (int(v) for v in slot)
    spec.format = CROP_FORMATS[format] if isinstance(format, str) else format
    spec.pitch = int(pitch or 0)
    return spec


def _crop_regions_args(regions, slot, format, pitch):
    """(spec, array of CropRegion, count) of a region list; slot None: the largest dst_x + w and dst_y + h of the list."""
    items = [_crop_region(r) for r in regions]
    if slot is None:
        slot = (max(r.dst_x + r.width for r in items), max(r.dst_y + r.height for r in items)) if items else (1, 1)  # (no region: nothing is written)
    array = (CropRegion * max(len(items), 1))(*items)
    return _crop_regions_spec(slot, format, pitch), array, len(items)


def crop_regions_shape(slot, format="rgba", pitch=None):
    """(pitch, slot_bytes) of the cropped decode of a region list into slots of slot = (width, height) pixels --
    compeg_crop_regions_shape; no device needed.  "rgba": slot rows of 4 width bytes at `pitch` (a multiple of 4, None =
    tight); "rgb_planar": a tight [3, height, width] u8 block a slot.  Region k's slot lies at k * slot_bytes."""
    spec = _crop_regions_spec(slot, format, pitch)
    pt, total = C.c_uint32(), C.c_uint64()
    check(lib.compeg_crop_regions_shape(C.byref(spec), C.byref(pt), C.byref(total)))
    return pt.value, total.value


def _host_view(data):
    a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(a)


class HostBuffer:
    """Page-locked host memory (compeg_host_alloc).  JPEG bytes that lie here -- `place()` packs a list of them -- go
    to the card without being touched on the host when a Batch with device preprocessing uploads them: the
    `Cow::Borrowed` road of ImageData::new + the uploads straight from the borrowed bytes (src/lib.rs:577-595,397-407)."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib.compeg_host_alloc(nbytes, C.byref(p)))
        self._p, self.nbytes = p, nbytes
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(nbytes, 1)).from_address(p.value))[:nbytes]

    def place(self, jpegs, align=64):
        """Copies the byte strings in, one behind the other; returns views of them (to hand to Batch.upload_jpegs)."""
        views, at = [], 0
        for j in jpegs:
            a = _host_view(j)
            if at + a.nbytes > self.nbytes:
                raise ValueError("HostBuffer too small")
            self.array[at:at + a.nbytes] = a
            views.append(self.array[at:at + a.nbytes])
            at = (at + a.nbytes + align - 1) // align * align
        return views

    def close(self):
        if self._p:
            self.array = None
            lib.compeg_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_feed_work(jpegs, host_threads, road, reps=1):
    """Seconds the host's share of feeding this batch takes, `reps` times over (compeg_host_feed_work: no device)."""
    jl = jpegs if isinstance(jpegs, JpegList) else JpegList(jpegs)
    sec = C.c_double()
    check(lib.compeg_host_feed_work(jl.ptrs, jl.lens, jl.count, host_threads, 0, road, reps, C.byref(sec)))
    return sec.value


def host_register(array):
    """Page-locks a caller-owned buffer (numpy array) in place: compeg_host_register."""
    check(lib.compeg_host_register(C.c_void_p(array.ctypes.data), array.nbytes))


def host_unregister(array):
    check(lib.compeg_host_unregister(C.c_void_p(array.ctypes.data)))


class JpegList:
    """The (pointer, length) arrays compeg_batch_upload_jpegs takes, gathered once from bytes-like objects (which this
    object keeps alive)."""

    def __init__(self, jpegs):
        self.views = [_host_view(j) for j in jpegs]
        self.count = len(self.views)
        self.ptrs = (C.c_void_p * self.count)(*[v.__array_interface__["data"][0] for v in self.views])
        self.lens = (C.c_size_t * self.count)(*[v.nbytes for v in self.views])


class Gpu:
    """An open handle to one MI355X (ref: `Gpu`, src/lib.rs:64-270)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, device=-1):
        """ref: Gpu::open (src/lib.rs:78-102)."""
        h = C.c_void_p()
        check(lib.compeg_gpu_open(device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_stream(cls, device, hip_stream):
        """`Gpu::from_wgpu` analogue (src/lib.rs:105): adopt a caller-owned HIP stream
        (an int / pointer value, e.g. torch.cuda.current_stream().cuda_stream)."""
        h = C.c_void_p()
        check(lib.compeg_gpu_from_stream(device, C.c_void_p(hip_stream), C.byref(h)))
        return cls(h)

    def device(self):
        return lib.compeg_gpu_device(self._h)

    def name(self):
        return lib.compeg_gpu_name(self._h).decode()

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_gpu_release(self._h)
            self._h = None


class ImageData:
    """A parsed JPEG (ref: `ImageData`, src/lib.rs:576-851)."""

    def __init__(self, jpeg, copy=True, allow_sampling=False, standard_entropy=False, allow_grayscale=False):
        """Extensions beyond the reference (compeg_image_parse_ext): allow_sampling -- 4:4:4, 4:4:0 and
        4:2:0 are accepted as well as 4:2:2; standard_entropy -- the bit reader is topped up in front of
        DC codes and ZRL skips 16 positions, as ITU-T T.81 has it (the reference deviates in both);
        allow_grayscale -- frames with one component are accepted and decode to R = G = B = luma."""
        self._h = None
        self._keep = _host_view(jpeg)
        h = C.c_void_p()
        flags = (1 if allow_sampling else 0) | (2 if standard_entropy else 0) | (4 if allow_grayscale else 0)
        if flags:
            check(lib.compeg_image_parse_ext(self._keep.ctypes.data, self._keep.nbytes, 1 if copy else 0, flags,
                                             C.byref(h)))
        else:
            check(lib.compeg_image_parse(self._keep.ctypes.data, self._keep.nbytes, 1 if copy else 0, C.byref(h)))
        self._h = h
        if copy:
            self._keep = None

    new = classmethod(lambda cls, jpeg: cls(jpeg))

    def width(self):
        return lib.compeg_image_width(self._h)

    def height(self):
        return lib.compeg_image_height(self._h)

    def parallelism(self):
        return lib.compeg_image_parallelism(self._h)

    def components(self):
        """Extension (compeg_image_components): 3, or 1 for a grayscale image (allow_grayscale)."""
        return lib.compeg_image_components(self._h)

    def sampling(self):
        """Extension (compeg_image_sampling): the luma component's sampling factors (h, v) -- (2, 1) for 4:2:2, (1, 1)
        for 4:4:4 and grayscale, (1, 2) for 4:4:0, (2, 2) for 4:2:0."""
        hs, vs = C.c_uint32(), C.c_uint32()
        check(lib.compeg_image_sampling(self._h, C.byref(hs), C.byref(vs)))
        return hs.value, vs.value

    def quant_table(self, component, order="zigzag"):
        """Extension (compeg_image_quant_table): the 64 quantisation factors of component `component` as np.uint16, in
        `order` ("zigzag" or "natural") -- what a level of decode_levels is multiplied by to give the coefficient."""
        out = (C.c_uint16 * 64)()
        check(lib.compeg_image_quant_table(self._h, component, out, _levels_order(order)))
        return np.frombuffer(out, dtype=np.uint16).copy()

    @property
    def orientation(self):
        """Extension (compeg_image_orientation): the file's EXIF orientation tag, 1..8; 1 where it has no usable one."""
        return lib.compeg_image_orientation(self._h)

    # what the reference uploads for this image (src/lib.rs:397-407)
    def metadata(self):
        return C.string_at(lib.compeg_image_metadata(self._h), METADATA_BYTES)

    def huffman_l1(self):
        return C.string_at(lib.compeg_image_huffman_l1(self._h), L1_BYTES)

    def huffman_l2(self):
        n = C.c_size_t()
        p = lib.compeg_image_huffman_l2(self._h, C.byref(n))
        return C.string_at(p, n.value) if n.value else b""

    def scan_range(self):
        o, n = C.c_size_t(), C.c_size_t()
        lib.compeg_image_scan_range(self._h, C.byref(o), C.byref(n))
        return o.value, n.value

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_image_free(self._h)
            self._h = None


class ScanBuffer:
    """ref: `ScanBuffer` (src/scan.rs:15-77; bench-only re-export, src/lib.rs:44-46)."""

    def __init__(self):
        self._h = C.c_void_p(lib.compeg_scanbuffer_new())

    def process(self, scan_data, expected_restart_intervals):
        a = _host_view(scan_data)
        check(lib.compeg_scanbuffer_process(self._h, a.ctypes.data, a.nbytes, expected_restart_intervals))

    def set_threads(self, threads):
        """Extension: threads that share one process() call (same output)."""
        check(lib.compeg_scanbuffer_set_threads(self._h, threads))

    def process_on_gpu(self, gpu, scan_data, expected_restart_intervals):
        """Same buffers, filled by the device-side scan kernels (extension)."""
        a = _host_view(scan_data)
        check(lib.compeg_scanbuffer_process_on_gpu(self._h, gpu._h, a.ctypes.data, a.nbytes,
                                                   expected_restart_intervals))

    def _get(self, fn):
        n = C.c_size_t()
        p = fn(self._h, C.byref(n))
        return C.string_at(p, n.value) if n.value else b""

    def processed_scan_data(self):
        return self._get(lib.compeg_scanbuffer_data)

    def start_positions(self):
        return self._get(lib.compeg_scanbuffer_start_positions)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_scanbuffer_free(self._h)
            self._h = None


class Texture:
    """Device-resident RGBA8 output (the role of wgpu::Texture in the reference).
    Exposes __cuda_array_interface__ so torch / cupy can wrap it without a copy."""

    def __init__(self, ptr, width, height, pitch, owner=None, owned=False):
        self.ptr, self.width, self.height, self.pitch = ptr, width, height, pitch
        self._owner, self._owned = owner, owned

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.height, self.width, 4), "typestr": "|u1", "data": (self.ptr, False),
                "strides": (self.pitch, 4, 1), "version": 3}

    def __del__(self):
        if getattr(self, "_owned", False) and self.ptr and lib is not None:
            lib.compeg_device_free(C.c_void_p(self.ptr))
            self.ptr = None


class DecodeOp:
    """ref: `DecodeOp` (src/lib.rs:541-574)."""

    def __init__(self, handle, decoder):
        self._h, self._decoder = handle, decoder

    def wait(self):
        check(lib.compeg_op_wait(self._h))

    def texture(self):
        return self._decoder.texture()

    def texture_changed(self):
        return bool(lib.compeg_op_texture_changed(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_op_free(self._h)
            self._h = None


class Decoder:
    """A GPU JPEG decode context (ref: `Decoder`, src/lib.rs:273-529).  One thread at a time."""

    def __init__(self, gpu):
        self._gpu = gpu
        h = C.c_void_p()
        check(lib.compeg_decoder_new(gpu._h, C.byref(h)))
        self._h = h

    new = classmethod(lambda cls, gpu: cls(gpu))

    def enqueue(self, data, hip_stream=0):
        """ref: Decoder::enqueue (src/lib.rs:385).  Returns texture_changed."""
        changed = C.c_int()
        check(lib.compeg_decoder_enqueue(self._h, data._h, C.c_void_p(hip_stream), C.byref(changed)))
        return bool(changed.value)

    def start_decode(self, data):
        op = C.c_void_p()
        check(lib.compeg_decoder_start_decode(self._h, data._h, C.byref(op)))
        return DecodeOp(op, self)

    def decode_blocking(self, data):
        op = C.c_void_p()
        check(lib.compeg_decoder_decode_blocking(self._h, data._h, C.byref(op)))
        return DecodeOp(op, self)

    def decode_planes(self, data, dst, format="planar", chroma="coded", pitch=None, hip_stream=0, blocking=False):
        """Extension (compeg_decoder_decode_planes): uploads and preprocesses `data` as enqueue does and records, on hip_stream
        (0 = the gpu's stream), a decode that writes the file's own Y, Cb and Cr samples into caller-owned device memory as
        planes_shape lays them out -- no colour step, no upsampling.  dst: (address, nbytes), a tensor, or a
        __cuda_array_interface__ object of at least total_bytes.  The texture and what the packs read are not touched.
        Returns without waiting; blocking=True (the gpu's stream only) waits for the decode."""
        spec = _planes_spec(format, chroma, pitch)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_planes: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_planes_blocking(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_planes(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_reduced(self, data, dst, format="rgba", pitch=None, hip_stream=0, blocking=False):
        """Extension (compeg_decoder_decode_reduced): uploads and preprocesses `data` as enqueue does and records, on
        hip_stream (0 = the gpu's stream), a decode at 1/8 scale -- one RGB pixel per luma data unit, from the DC terms
        alone -- into caller-owned device memory as reduced_shape lays it out.  It is pixel (8x, 8y) of the full decode
        with every AC coefficient zero, not the 8 x 8 mean of the full decode.  dst: (address, nbytes), a tensor, or a
        __cuda_array_interface__ object of at least total_bytes.  The texture and what the packs read are not touched.
        Returns without waiting; blocking=True (the gpu's stream only) waits for the decode."""
        spec = _reduced_spec(format, pitch)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_reduced: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_reduced_blocking(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_reduced(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_scaled(self, data, dst, denominator, format="rgba", pitch=None, hip_stream=0, blocking=False):
        """Extension (compeg_decoder_decode_scaled): uploads and preprocesses `data` as enqueue does and records, on
        hip_stream (0 = the gpu's stream), a decode at 1 / denominator (2, 4 or 8) into caller-owned device memory as
        scaled_shape lays it out.  Every data unit gives N x N samples, N = 8 / denominator, from the N-point inverse DCT
        of the N x N lowest-frequency corner of its coefficients (IJG libjpeg's scaled IDCT in pinned f32 arithmetic:
        include/compeg_hip.h, "Scaled decode"); chroma is taken to the nearest neighbour, the colour step is the full
        decode's.  The result is neither the N x N block mean of the full decode nor libjpeg-turbo's output.
        Denominator 8 is decode_reduced, byte for byte, and last_kernel() then says "reduced".  dst: (address, nbytes),
        a tensor, or a __cuda_array_interface__ object of at least total_bytes.  The texture and what the packs read are
        not touched.  Returns without waiting; blocking=True (the gpu's stream only) waits for the decode."""
        spec = _scaled_spec(denominator, format, pitch)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_scaled: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_scaled_blocking(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_scaled(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_levels(self, data, dst, order="zigzag", hip_stream=0, blocking=False):
        """Extension (compeg_decoder_decode_levels): uploads and preprocesses `data` as enqueue does and records, on
        hip_stream (0 = the gpu's stream), a decode of the file's quantised DCT coefficients (levels) into caller-owned
        device memory as levels_shape lays it out: per component int16[blocks_h][blocks_w][64], whole MCUs, every value as
        the entropy decode yields it (not multiplied by the quantiser; position 0 the DC predictor's low 16 bits; all 64
        positions kept), in the file's zig-zag order or "natural" (row-major 8 x 8).  dst: (address, nbytes), a tensor, or
        a __cuda_array_interface__ object of at least total_bytes at an address that is a multiple of 16.  The texture and
        what the packs read are not touched.  Returns without waiting; blocking=True (the gpu's stream only) waits."""
        spec = _levels_spec(order)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_levels: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_levels_blocking(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_levels(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_cropped(self, data, dst, rect, format="rgba", pitch=None, hip_stream=None, blocking=False):
        """Extension (compeg_decoder_decode_cropped): uploads and preprocesses `data` as enqueue does and records, on
        hip_stream (None or 0 = the gpu's stream), a decode of rect = (x, y, w, h) -- pixels of the image, non-empty,
        inside it -- into caller-owned device memory as crop_shape lays it out: pixel (i, j) is pixel (x + i, y + j) of the
        RGBA decode, byte for byte.  Restart intervals without an MCU in the rectangle are not decoded.  dst: (address,
        nbytes), a tensor, or a __cuda_array_interface__ object of at least total_bytes.  The texture and what the packs
        read are not touched.  Returns without waiting; blocking=True (the gpu's stream only) waits for the decode."""
        spec = _crop_spec(rect, format, pitch)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_cropped: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_cropped_blocking(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_cropped(self._h, data._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream or None)))

    def decode_cropped_regions(self, data, dst, regions, slot=None, format="rgba", pitch=None, hip_stream=None, blocking=False):
        """Extension (compeg_decoder_decode_cropped_regions): decode_cropped with a list of rectangles of the one image --
        regions: (0, (x, y, w, h)), (0, (x, y, w, h), (dst_x, dst_y)) or CropRegions -- region k into slot k of dst, a
        [len(regions), slot_h, slot_w, 4] ("rgba") or [len(regions), 3, slot_h, slot_w] ("rgb_planar") u8 block as
        crop_regions_shape lays it out; slot=None: the largest dst_x + w and dst_y + h of the list.  What lies outside a
        region's rectangle in its slot is not written.  Returns without waiting; blocking=True (the gpu's stream only)
        waits for the decode."""
        spec, array, count = _crop_regions_args(regions, slot, format, pitch)
        addr, nbytes = _device_range(dst)
        if blocking:
            if hip_stream:
                raise Error("decode_cropped_regions: blocking=True records on the gpu's own stream")
            check(lib.compeg_decoder_decode_cropped_regions_blocking(self._h, data._h, C.byref(spec), array, count, C.c_void_p(addr), nbytes))
        else:
            check(lib.compeg_decoder_decode_cropped_regions(self._h, data._h, C.byref(spec), array, count, C.c_void_p(addr), nbytes,
                                                            C.c_void_p(hip_stream or None)))

    def last_warning(self):
        return lib.compeg_decoder_last_warning(self._h).decode()

    def last_stage_times(self):
        """Host microseconds of the last decode's stages: the reference's three trace timers
        (t_preprocess, t_enqueue_writes, t_poll: src/lib.rs:391-396,452-475,516-522)."""
        t = (C.c_double * 3)()
        check(lib.compeg_decoder_last_stage_times(self._h, t))
        return {"preprocess_us": t[0], "enqueue_writes_us": t[1], "poll_us": t[2]}

    def last_kernel(self):
        """Diagnostics: the decode kernel the last enqueue went to (KERNEL_* names)."""
        return LAST_KERNEL_NAMES[lib.compeg_decoder_last_kernel(self._h)]

    def set_device_preprocess(self, on=True):
        """Extension: preprocess scans with the device-side scan kernels instead of on the host."""
        check(lib.compeg_decoder_set_device_preprocess(self._h, 1 if on else 0))

    def set_scan_threads(self, threads):
        """Extension: threads of this decoder's host scan preprocessor."""
        check(lib.compeg_decoder_set_scan_threads(self._h, threads))

    def texture(self):
        p, w, h, pitch = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib.compeg_decoder_output(self._h, C.byref(p), C.byref(w), C.byref(h), C.byref(pitch)))
        return Texture(p.value, w.value, h.value, pitch.value, owner=self)

    def into_texture(self):
        p, w, h, pitch = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib.compeg_decoder_take_output(self._h, C.byref(p), C.byref(w), C.byref(h), C.byref(pitch)))
        self._h = None
        return Texture(p.value, w.value, h.value, pitch.value, owned=True)

    def read_texture(self, width, height):
        """Tightly packed host copy of the WxH corner (what src/tests.rs:52-84 does)."""
        out = np.empty((height, width, 4), dtype=np.uint8)
        check(lib.compeg_decoder_read_output(self._h, out.ctypes.data, width, height))
        return out

    def pack_tensor(self, dst, dtype="f16", downscale=1, scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_decoder_pack_tensor): records, on hip_stream (0 = the gpu's stream), the pack of the last decoded image into
        caller-owned device memory as the planar tensor a model reads -- [3, H / downscale, W / downscale], alpha dropped, block mean over
        downscale x downscale pixels, then * scale[c] + bias[c] per plane, stored as dtype ("u8", "f16", "bf16", "f32").
        dst: (address, nbytes), a tensor (data_ptr / numel / element_size), or a __cuda_array_interface__ object.
        Returns without waiting; the pack runs behind the decode and the next decode behind the pack."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_decoder_pack_tensor(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def pack_tensor_resized(self, dst, size, crop=None, filter="bilinear", dtype="f16", downscale=1, scale=(1, 1, 1), bias=(0, 0, 0),
                            order="rgb", hip_stream=0, antialias=False):
        """Extension (compeg_decoder_pack_tensor_resized): like pack_tensor, but crop = (x, y, w, h) of the last decoded image (None: all
        of it) is block-averaged over downscale x downscale pixels and then resized to size = (ow, oh) with filter ("bilinear":
        half-pixel centres, no antialiasing; "nearest"), giving [3, oh, ow].  antialias=True (bilinear only) widens the filter
        with the reduction where an axis shrinks, as PIL and torch's interpolate(antialias=True) do; the prefiltered crop may be 64
        times the output at the most either way.  Returns without waiting."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        resize = _resize_spec(size, filter, antialias)
        rect = _rect(crop) if crop is not None else None
        addr, nbytes = _device_range(dst)
        check(lib.compeg_decoder_pack_tensor_resized(self._h, C.byref(spec), C.byref(resize), C.byref(rect) if rect is not None else None,
                                                     C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def pack_tensor_regions(self, dst, size, regions, pad=(0, 0, 0), filter="bilinear", dtype="f16", downscale=1, scale=(1, 1, 1),
                            bias=(0, 0, 0), order="rgb", hip_stream=0, antialias=False):
        """Extension (compeg_decoder_pack_tensor_regions): regions = [(0, src or None, dst or None), ...] of the last decoded image
        into [len(regions), 3, oh, ow]: crop src is resized as pack_tensor_resized does it into rectangle dst of its slot
        (region_fit gives the letterbox's), the rest of the slot is pad (R, G, B on the pixel scale) put through scale and
        bias.  Returns without waiting, like pack_tensor."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        resize = _resize_spec(size, filter, antialias)
        list_, n = _regions(regions)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_decoder_pack_tensor_regions(self._h, C.byref(spec), C.byref(resize), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                     C.c_void_p(hip_stream)))

    def pack_tensor_filtered(self, dst, size, regions=None, kernel="bicubic", pad=(0, 0, 0), dtype="f16", downscale=1, scale=(1, 1, 1),
                             bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_decoder_pack_tensor_filtered): pack_tensor_regions with one of FILTER_KERNELS -- PIL's box,
        triangle (BILINEAR), bicubic and lanczos3 resampling, each widened with the reduction.  regions=None: the whole
        image into the whole output, [1, 3, oh, ow].  Returns without waiting, like pack_tensor."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        list_, n = _regions(regions if regions is not None else [(0, None, None)])
        addr, nbytes = _device_range(dst)
        check(lib.compeg_decoder_pack_tensor_filtered(self._h, C.byref(spec), C.byref(filter), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                      C.c_void_p(hip_stream)))

    def pack_tensor_oriented(self, dst, size, regions=None, orientation="exif", kernel="bicubic", pad=(0, 0, 0), dtype="f16", downscale=1,
                             scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_decoder_pack_tensor_oriented): pack_tensor_filtered with an orientation per region -- a name of
        ORIENTATIONS, 1..8, or "exif" for the image's own tag.  size = (ow, oh) is the UPRIGHT slot, a region's dst lies in
        it, its src in the stored raster (orient_rect maps an upright crop there); regions are (0, src, dst) or
        (0, src, dst, orientation), `orientation` serving those that carry none.  regions=None: the whole image into the whole
        output.  Returns without waiting, like pack_tensor."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        list_, n = _oriented_regions(regions if regions is not None else [(0, None, None)], orientation)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_decoder_pack_tensor_oriented(self._h, C.byref(spec), C.byref(filter), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                      C.c_void_p(hip_stream)))

    def pack_tensor_nhwc(self, dst, size, regions=None, orientation="exif", channels=3, fill=0.0, kernel="bicubic", pad=(0, 0, 0), dtype="f16",
                         downscale=1, scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_decoder_pack_tensor_nhwc): pack_tensor_oriented into a channels-last destination,
        [count, oh, ow, channels] with channels 3 or 4; element 3 of every pixel is `fill`, converted like any value, with
        neither scale nor bias.  dst: (address, nbytes), a contiguous [.., oh, ow, C] tensor, or a [.., C, oh, ow] tensor with
        channels-last strides (torch.channels_last) as it is -- a planar tensor is refused.  Returns without waiting."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        nhwc = _nhwc_spec(channels, fill)
        list_, n = _oriented_regions(regions if regions is not None else [(0, None, None)], orientation)
        addr, nbytes = _nhwc_device_range(dst, size, channels)
        check(lib.compeg_decoder_pack_tensor_nhwc(self._h, C.byref(spec), C.byref(filter), C.byref(nhwc), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                  C.c_void_p(hip_stream)))

    def pack_tensor_luma(self, dst, size, regions=None, orientation="exif", weights="bt601", kernel="bicubic", pad=0.0, dtype="f16", downscale=1,
                         scale=1.0, bias=0.0, hip_stream=0):
        """Extension (compeg_decoder_pack_tensor_luma): pack_tensor_oriented with one channel a slot, [count, 1, oh, ow]: per
        source pixel L = (wR R + wG G + wB B + 32768) >> 16, resampled like a channel of the oriented pack.  weights: "bt601"
        (PIL's convert("L")), "bt709", "r", "g", "b", or three integers with a sum of 65536; a grayscale frame gives its own
        values under any of them.  pad, scale, bias: one number each.  dst: (address, nbytes), or a dense tensor of `count`
        slots, [.., 1, oh, ow], [.., oh, ow, 1] or [.., oh, ow].  Returns without waiting."""
        spec = _tensor_spec(dtype, downscale, (scale,) * 3, (bias,) * 3, "rgb")
        filter = _filter_spec(size, kernel)
        luma = _luma_spec(weights)
        list_, n = _oriented_regions(regions if regions is not None else [(0, None, None)], orientation)
        addr, nbytes = _luma_device_range(dst, size, n)
        check(lib.compeg_decoder_pack_tensor_luma(self._h, C.byref(spec), C.byref(filter), C.byref(luma), list_, n, _luma_pad(pad), C.c_void_p(addr),
                                                  nbytes, C.c_void_p(hip_stream)))

    def read_coefficients(self, total_dus):
        out = np.empty(total_dus * 32, dtype=np.int32)
        check(lib.compeg_decoder_read_coefficients(self._h, out.ctypes.data, out.size))
        return out

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_decoder_free(self._h)
            self._h = None


class Batch:
    """Extension (not in the reference): many independent images per launch sequence."""

    def __init__(self, gpu):
        self._gpu = gpu
        h = C.c_void_p()
        check(lib.compeg_batch_new(gpu._h, C.byref(h)))
        self._h = h
        self._images = []

    def upload(self, images, host_threads=0):
        self._images = list(images)
        arr = (C.c_void_p * len(self._images))(*[im._h for im in self._images])
        check(lib.compeg_batch_upload(self._h, arr, len(self._images), host_threads))

    def upload_jpegs(self, jpegs, host_threads=0, allow_sampling=False, standard_entropy=False, allow_grayscale=False):
        """Host-fed use: parse (on the worker threads), preprocess, upload.  jpegs: bytes-like objects, or a
        JpegList made from them once (saves this wrapper's per-call pointer gathering, nothing else)."""
        jl = jpegs if isinstance(jpegs, JpegList) else JpegList(jpegs)
        flags = (1 if allow_sampling else 0) | (2 if standard_entropy else 0) | (4 if allow_grayscale else 0)
        self._images = []
        check(lib.compeg_batch_upload_jpegs(self._h, jl.ptrs, jl.lens, jl.count, host_threads, flags))

    def upload_jpegs_begin(self, jpegs, host_threads=0, allow_sampling=False, standard_entropy=False, allow_grayscale=False):
        """compeg_batch_upload_jpegs_begin: returns when the transfers are queued; upload_end() (or decode()) finishes."""
        jl = jpegs if isinstance(jpegs, JpegList) else JpegList(jpegs)
        flags = (1 if allow_sampling else 0) | (2 if standard_entropy else 0) | (4 if allow_grayscale else 0)
        self._images = []
        self._feeding = jl   # (the bytes stay alive until the upload has ended)
        check(lib.compeg_batch_upload_jpegs_begin(self._h, jl.ptrs, jl.lens, jl.count, host_threads, flags))

    def upload_end(self):
        check(lib.compeg_batch_upload_end(self._h))
        self._feeding = None

    def set_device_preprocess(self, mode):
        """0 host (default), 1 scan kernels once at upload, 2 scan kernels in every decode."""
        check(lib.compeg_batch_set_device_preprocess(self._h, mode))

    def host_fallbacks(self):
        return lib.compeg_batch_host_fallbacks(self._h)

    def set_chunk(self, images_per_launch):
        check(lib.compeg_batch_set_chunk(self._h, images_per_launch))

    def decode(self, hip_stream=0):
        check(lib.compeg_batch_decode(self._h, C.c_void_p(hip_stream)))

    def decode_planes(self, dst, format="planar", chroma="coded", pitch=None, hip_stream=0):
        """Extension (compeg_batch_decode_planes): records, on hip_stream (0 = the gpu's stream), a decode of the last upload's
        images (all of one size and sampling) that writes each one's own Y, Cb and Cr samples into caller-owned device memory,
        image i at i * total_bytes of planes_shape -- no colour step, no upsampling.  dst: (address, nbytes), a tensor, or a
        __cuda_array_interface__ object.  The RGBA outputs are not touched.  Returns without waiting; wait() covers it."""
        spec = _planes_spec(format, chroma, pitch)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_planes(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_reduced(self, dst, format="rgba", pitch=None, hip_stream=0):
        """Extension (compeg_batch_decode_reduced): records, on hip_stream (0 = the gpu's stream), a decode of the last
        upload's images (all of one size and sampling) at 1/8 scale into caller-owned device memory, image i at
        i * total_bytes of reduced_shape.  dst: (address, nbytes), a tensor, or a __cuda_array_interface__ object.  The
        RGBA outputs are not touched; wait() covers it."""
        spec = _reduced_spec(format, pitch)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_reduced(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_scaled(self, dst, denominator, format="rgba", pitch=None, hip_stream=0):
        """Extension (compeg_batch_decode_scaled): records, on hip_stream (0 = the gpu's stream), a decode of the last
        upload's images (all of one size and sampling) at 1 / denominator (2, 4 or 8) into caller-owned device memory,
        image i at i * total_bytes of scaled_shape.  The samples are Decoder.decode_scaled's: the N-point inverse DCT of
        each data unit's N x N lowest frequencies, N = 8 / denominator -- neither the block mean of the full decode nor
        libjpeg-turbo's output; denominator 8 is decode_reduced.  dst: (address, nbytes), a tensor, or a
        __cuda_array_interface__ object.  The RGBA outputs are not touched; wait() covers it."""
        spec = _scaled_spec(denominator, format, pitch)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_scaled(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def decode_cropped(self, dst, rect, format="rgba", pitch=None, hip_stream=None):
        """Extension (compeg_batch_decode_cropped): records, on hip_stream (None or 0 = the gpu's stream), a decode of
        rect = (x, y, w, h), one rectangle for all of the last upload's images (all of one size and sampling), into
        caller-owned device memory, image i at i * total_bytes of crop_shape.  dst: (address, nbytes), a tensor, or a
        __cuda_array_interface__ object.  The RGBA outputs are not touched; wait() covers it."""
        spec = _crop_spec(rect, format, pitch)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_cropped(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream or None)))

    def decode_cropped_regions(self, dst, regions, slot=None, format="rgba", pitch=None, hip_stream=None):
        """Extension (compeg_batch_decode_cropped_regions): records, on hip_stream (None or 0 = the gpu's stream), a
        cropped decode of a region list -- regions: (image, (x, y, w, h)), (image, (x, y, w, h), (dst_x, dst_y)) or
        CropRegions, image an index into the last upload -- region k into slot k of dst, a [len(regions), slot_h, slot_w,
        4] ("rgba") or [len(regions), 3, slot_h, slot_w] ("rgb_planar") u8 block as crop_regions_shape lays it out;
        slot=None: the largest dst_x + w and dst_y + h of the list.  The images may be of any mix of sizes and samplings;
        set_chunk bounds the regions per launch.  What lies outside a region's rectangle in its slot is not written.
        The RGBA outputs are not touched; wait() covers it."""
        spec, array, count = _crop_regions_args(regions, slot, format, pitch)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_cropped_regions(self._h, C.byref(spec), array, count, C.c_void_p(addr), nbytes, C.c_void_p(hip_stream or None)))

    def wait(self):
        check(lib.compeg_batch_wait(self._h))

    def count(self):
        return lib.compeg_batch_count(self._h)

    def output(self, index):
        p, w, h, pitch = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_size_t()
        check(lib.compeg_batch_output(self._h, index, C.byref(p), C.byref(w), C.byref(h), C.byref(pitch)))
        return Texture(p.value, w.value, h.value, pitch.value, owner=self)

    def read_output(self, index):
        t = self.output(index)
        out = np.empty((t.height, t.width, 4), dtype=np.uint8)
        check(lib.compeg_batch_read_output(self._h, index, out.ctypes.data))
        return out

    def pack_tensor(self, dst, dtype="f16", downscale=1, scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_batch_pack_tensor): records, on hip_stream (0 = the gpu's stream), the pack of the last decode's images (all of one size) into
        caller-owned device memory as the planar tensor a model reads -- [count, 3, H / downscale, W / downscale], alpha dropped, block mean over
        downscale x downscale pixels, then * scale[c] + bias[c] per plane, stored as dtype ("u8", "f16", "bf16", "f32").
        dst: (address, nbytes), a tensor (data_ptr / numel / element_size), or a __cuda_array_interface__ object.
        Returns without waiting; the pack runs behind the decode and the next decode behind the pack."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_pack_tensor(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def pack_tensor_resized(self, dst, size, crops=None, filter="bilinear", dtype="f16", downscale=1, scale=(1, 1, 1), bias=(0, 0, 0),
                            order="rgb", hip_stream=0, antialias=False):
        """Extension (compeg_batch_pack_tensor_resized): the last decode's images, of whatever sizes, each block-averaged over downscale x
        downscale pixels and resized to size = (ow, oh), giving [count, 3, oh, ow].  crops: None (whole images), one (x, y, w, h)
        for every image, or a list with one per image.  antialias: as Decoder.pack_tensor_resized has it.  Returns without
        waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        resize = _resize_spec(size, filter, antialias)
        rects = None
        if crops is not None:
            n = self.count()
            if len(crops) == 4 and not isinstance(crops[0], (tuple, list, Rect)):
                crops = [crops] * n
            if len(crops) != n:
                raise Error(f"pack_tensor_resized: {len(crops)} crops for a batch of {n} images")
            rects = (Rect * max(n, 1))(*[c if isinstance(c, Rect) else _rect(c) for c in crops])
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_pack_tensor_resized(self._h, C.byref(spec), C.byref(resize), rects, C.c_void_p(addr), nbytes,
                                                   C.c_void_p(hip_stream)))

    def pack_tensor_regions(self, dst, size, regions, pad=(0, 0, 0), filter="bilinear", dtype="f16", downscale=1, scale=(1, 1, 1),
                            bias=(0, 0, 0), order="rgb", hip_stream=0, antialias=False):
        """Extension (compeg_batch_pack_tensor_regions): regions = [(image, src or None, dst or None), ...] over the last decode's
        images -- any of them any number of times, in any order -- into [len(regions), 3, oh, ow], as
        Decoder.pack_tensor_regions has it.  Returns without waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        resize = _resize_spec(size, filter, antialias)
        list_, n = _regions(regions)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_pack_tensor_regions(self._h, C.byref(spec), C.byref(resize), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                   C.c_void_p(hip_stream)))

    def pack_tensor_filtered(self, dst, size, regions=None, kernel="bicubic", pad=(0, 0, 0), dtype="f16", downscale=1, scale=(1, 1, 1),
                             bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_batch_pack_tensor_filtered): Decoder.pack_tensor_filtered over the last decode's images, regions as
        pack_tensor_regions takes them.  regions=None: every image, whole, into the whole output of its own slot,
        [count, 3, oh, ow].  Returns without waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        list_, n = _regions(regions if regions is not None else [(i, None, None) for i in range(self.count())])
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_pack_tensor_filtered(self._h, C.byref(spec), C.byref(filter), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                    C.c_void_p(hip_stream)))

    def pack_tensor_oriented(self, dst, size, regions=None, orientation="exif", kernel="bicubic", pad=(0, 0, 0), dtype="f16", downscale=1,
                             scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_batch_pack_tensor_oriented): Decoder.pack_tensor_oriented over the last decode's images, regions
        (image, src, dst) or (image, src, dst, orientation).  regions=None: every image, whole, into its own upright slot,
        [count, 3, oh, ow].  Returns without waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        list_, n = _oriented_regions(regions if regions is not None else [(i, None, None) for i in range(self.count())], orientation)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_pack_tensor_oriented(self._h, C.byref(spec), C.byref(filter), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                    C.c_void_p(hip_stream)))

    def pack_tensor_nhwc(self, dst, size, regions=None, orientation="exif", channels=3, fill=0.0, kernel="bicubic", pad=(0, 0, 0), dtype="f16",
                         downscale=1, scale=(1, 1, 1), bias=(0, 0, 0), order="rgb", hip_stream=0):
        """Extension (compeg_batch_pack_tensor_nhwc): Decoder.pack_tensor_nhwc over the last decode's images, regions as in
        pack_tensor_oriented.  regions=None: every image, whole, into its own upright slot, [count, oh, ow, channels].
        Returns without waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, scale, bias, order)
        filter = _filter_spec(size, kernel)
        nhwc = _nhwc_spec(channels, fill)
        list_, n = _oriented_regions(regions if regions is not None else [(i, None, None) for i in range(self.count())], orientation)
        addr, nbytes = _nhwc_device_range(dst, size, channels)
        check(lib.compeg_batch_pack_tensor_nhwc(self._h, C.byref(spec), C.byref(filter), C.byref(nhwc), list_, n, _pad(pad), C.c_void_p(addr), nbytes,
                                                C.c_void_p(hip_stream)))

    def pack_tensor_luma(self, dst, size, regions=None, orientation="exif", weights="bt601", kernel="bicubic", pad=0.0, dtype="f16", downscale=1,
                         scale=1.0, bias=0.0, hip_stream=0):
        """Extension (compeg_batch_pack_tensor_luma): Decoder.pack_tensor_luma over the last decode's images, regions as in
        pack_tensor_oriented.  regions=None: every image, whole, into its own upright slot, [count, 1, oh, ow].  Returns
        without waiting; wait() covers it."""
        spec = _tensor_spec(dtype, downscale, (scale,) * 3, (bias,) * 3, "rgb")
        filter = _filter_spec(size, kernel)
        luma = _luma_spec(weights)
        list_, n = _oriented_regions(regions if regions is not None else [(i, None, None) for i in range(self.count())], orientation)
        addr, nbytes = _luma_device_range(dst, size, n)
        check(lib.compeg_batch_pack_tensor_luma(self._h, C.byref(spec), C.byref(filter), C.byref(luma), list_, n, _luma_pad(pad), C.c_void_p(addr),
                                                nbytes, C.c_void_p(hip_stream)))

    def decode_levels(self, dst, order="zigzag", hip_stream=0):
        """Extension (compeg_batch_decode_levels): records, on hip_stream (0 = the gpu's stream), a decode of the last
        upload's images to their quantised DCT coefficients (levels) into caller-owned device memory, image i at
        i * total_bytes of levels_shape.  The values are Decoder.decode_levels's.  All images must have one size and one
        sampling; the address must be a multiple of 16.  Returns without waiting; wait() covers it."""
        spec = _levels_spec(order)
        addr, nbytes = _device_range(dst)
        check(lib.compeg_batch_decode_levels(self._h, C.byref(spec), C.c_void_p(addr), nbytes, C.c_void_p(hip_stream)))

    def quant_table(self, index, component, order="zigzag"):
        """The 64 quantisation factors (np.uint16, in `order`) of component `component` of image `index` of the last upload
        (compeg_batch_quant_table)."""
        out = (C.c_uint16 * 64)()
        check(lib.compeg_batch_quant_table(self._h, index, component, out, _levels_order(order)))
        return np.frombuffer(out, dtype=np.uint16).copy()

    def orientation(self, index):
        """The EXIF orientation tag (1..8) of image `index` of the last upload (compeg_batch_image_orientation)."""
        out = C.c_uint32()
        check(lib.compeg_batch_image_orientation(self._h, index, C.byref(out)))
        return out.value

    def algorithmic_bytes(self):
        return lib.compeg_batch_algorithmic_bytes(self._h)

    def pixels(self):
        return lib.compeg_batch_pixels(self._h)

    def last_kernel(self):
        """Diagnostics: the decode kernel the first launch of the last decode went to (KERNEL_NAMES)."""
        return LAST_KERNEL_NAMES[lib.compeg_batch_last_kernel(self._h)]

    def set_timing(self, on=True):
        """compeg_batch_set_timing: off = decodes record no timing events (they run closer together)."""
        check(lib.compeg_batch_set_timing(self._h, 1 if on else 0))

    def timing(self, reset=True):
        """(decodes, total_ms, huffman_ms, idct_composite_ms) summed over the decodes since the
        last upload/reset, from HIP events recorded on the stream the kernels ran on."""
        n, total = C.c_uint32(), C.c_double()
        stages = (C.c_double * 2)()
        check(lib.compeg_batch_timing(self._h, 1 if reset else 0, C.byref(n), C.byref(total), stages))
        return n.value, total.value, stages[0], stages[1]

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (lib is None once the interpreter is shutting down)
            lib.compeg_batch_free(self._h)
            self._h = None
