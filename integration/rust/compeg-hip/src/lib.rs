//! `compeg`-shaped API over `libcompeg_hip.so` (MI355X / gfx950).
//!
//! Same public items and call sequences as SludgePhD/Compeg's `src/lib.rs`
//! (`Gpu`, `Decoder`, `DecodeOp`, `ImageData`, the doc-hidden `ScanBuffer`,
//! `Error`/`Result`), with two substitutions a caller can see:
//!
//! * the output is a [`Texture`] (device pointer to RGBA8 rows + extent +
//!   pitch) instead of a `wgpu::Texture`;
//! * `Decoder::enqueue` records on a HIP stream ([`Stream`]) instead of a
//!   `wgpu::CommandEncoder`.
//!
//! [`Batch`] (many images per launch) is an extension the reference does not
//! have.  This crate has not been compiled in the repository's build image
//! (no Rust toolchain there); the C ABI underneath is what the test suite
//! exercises, through the same entry points in the same order.

mod ffi;

use std::borrow::Cow;
use std::ffi::CStr;
use std::fmt;
use std::marker::PhantomData;
use std::os::raw::{c_int, c_void};
use std::ptr::{self, NonNull};
use std::sync::Arc;

/// String-only error, `Display` = `Debug` = the message (like `compeg::Error`).
pub struct Error {
    message: String,
    code: i32,
}

impl Error {
    /// The C status behind the message (`COMPEG_E_*`); the reference has no equivalent.
    pub fn code(&self) -> i32 {
        self.code
    }

    fn last(code: c_int) -> Self {
        // thread-local in the library: valid until this thread's next failing call
        let message = unsafe { CStr::from_ptr(ffi::compeg_last_error()) }.to_string_lossy().into_owned();
        Error { message, code }
    }
}

impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        f.write_str(&self.message)
    }
}

impl fmt::Debug for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        f.write_str(&self.message)
    }
}

impl std::error::Error for Error {}

pub type Result<T, E = Error> = std::result::Result<T, E>;

fn check(code: c_int) -> Result<()> {
    if code == ffi::COMPEG_OK {
        Ok(())
    } else {
        Err(Error::last(code))
    }
}

/// A HIP stream owned by the caller (`hipStream_t`); null = the `Gpu`'s own stream.
#[derive(Clone, Copy)]
pub struct Stream(pub *mut c_void);

impl Stream {
    pub const DEFAULT: Stream = Stream(ptr::null_mut());
}

/// Element type of a packed tensor (`COMPEG_TENSOR_*`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum TensorType {
    U8 = 0,
    F16 = 1,
    Bf16 = 2,
    F32 = 3,
}

/// What `Decoder::pack_tensor` / `Batch::pack_tensor` make of the RGBA8 output (extension; compeg_hip.h, "Tensor
/// output"): planes in RGB or BGR order, alpha dropped, the mean over `downscale` x `downscale` pixels (1, 2, 4 or 8),
/// then `* scale[c] + bias[c]` per plane, stored as `dtype`.
#[derive(Clone, Copy, Debug)]
pub struct TensorSpec {
    pub dtype: TensorType,
    pub bgr: bool,
    pub downscale: u32,
    pub scale: [f32; 3],
    pub bias: [f32; 3],
}

impl TensorSpec {
    pub fn new(dtype: TensorType) -> Self {
        TensorSpec { dtype, bgr: false, downscale: 1, scale: [1.0; 3], bias: [0.0; 3] }
    }

    fn raw(&self) -> ffi::compeg_tensor_spec {
        ffi::compeg_tensor_spec {
            dtype: self.dtype as u32,
            order: if self.bgr { ffi::COMPEG_TENSOR_BGR } else { ffi::COMPEG_TENSOR_RGB },
            downscale: self.downscale,
            reserved: 0,
            scale: self.scale,
            bias: self.bias,
        }
    }

    /// `(width, height, bytes)` of one `width` x `height` image's tensor; no device needed.
    pub fn shape(&self, width: u32, height: u32) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe { ffi::compeg_tensor_shape(&self.raw(), width, height, &mut w, &mut h, &mut n) })?;
        Ok((w, h, n))
    }
}

/// Filter of a resized pack (`COMPEG_RESIZE_*`).  `BilinearAntialias` is `COMPEG_RESIZE_BILINEAR |
/// COMPEG_RESIZE_ANTIALIAS`: where an axis shrinks the filter widens with the reduction, as PIL and torch's
/// `interpolate(antialias=True)` do; where none shrinks it is `Bilinear` element for element.  The block-averaged crop
/// may then be 64 times the output at the most either way.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ResizeFilter {
    Nearest = 0,
    Bilinear = 1,
    BilinearAntialias = (ffi::COMPEG_RESIZE_BILINEAR | ffi::COMPEG_RESIZE_ANTIALIAS) as isize,
}

/// A crop in pixels (`compeg_rect`).
pub type Rect = ffi::compeg_rect;

/// The fixed output extent of `Decoder::pack_tensor_resized` / `Batch::pack_tensor_resized` (extension; compeg_hip.h,
/// "Resized tensor output"): the crop is block-averaged as `TensorSpec::downscale` says, then resized to `width` x
/// `height` -- bilinear with half-pixel centres (antialiased or not), or nearest.
#[derive(Clone, Copy, Debug)]
pub struct ResizeSpec {
    pub width: u32,
    pub height: u32,
    pub filter: ResizeFilter,
}

impl ResizeSpec {
    pub fn new(width: u32, height: u32) -> Self {
        ResizeSpec { width, height, filter: ResizeFilter::Bilinear }
    }

    /// The antialias switch: the same extent with `BilinearAntialias` (on) or `Bilinear` (off).  The flag goes with no
    /// other filter, so this replaces `Nearest` too.
    pub fn antialias(mut self, on: bool) -> Self {
        self.filter = if on { ResizeFilter::BilinearAntialias } else { ResizeFilter::Bilinear };
        self
    }

    fn raw(&self) -> ffi::compeg_resize_spec {
        ffi::compeg_resize_spec { out_width: self.width, out_height: self.height, filter: self.filter as u32, reserved: 0 }
    }

    /// `(pre_width, pre_height, bytes)`: the extent of the block-averaged crop of a `width` x `height` image that the
    /// filter reads, and one image's tensor in bytes; no device needed.
    pub fn shape(&self, tensor: &TensorSpec, width: u32, height: u32, crop: Option<&Rect>) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        let crop = crop.map_or(ptr::null(), |c| c as *const Rect);
        check(unsafe { ffi::compeg_resized_tensor_shape(&tensor.raw(), &self.raw(), width, height, crop, &mut w, &mut h, &mut n) })?;
        Ok((w, h, n))
    }
}

/// One output slot of `Decoder::pack_tensor_regions` / `Batch::pack_tensor_regions` (extension; compeg_hip.h, "Region
/// tensor output"): crop `src` of image `image` is resized into rectangle `dst` of the slot, the rest of the slot is the
/// pad value.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Region {
    /// Index into the batch's last upload; 0 for a decoder.
    pub image: u32,
    /// `None`: the whole image.
    pub src: Option<Rect>,
    /// `None`: the whole output.
    pub dst: Option<Rect>,
}

/// Where `Region::fit` puts the fitted rectangle (`COMPEG_FIT_*`).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum FitAlign {
    Center = 0,
    TopLeft = 1,
}

impl Region {
    pub fn whole(image: u32) -> Self {
        Region { image, src: None, dst: None }
    }

    /// The rectangle of an `out` = (width, height) output that a crop of `src` = (width, height) pixels fills when it
    /// is fitted with its aspect ratio kept (the letterbox's inner rectangle); no device needed.
    pub fn fit(src: (u32, u32), out: (u32, u32), align: FitAlign) -> Result<Rect> {
        let mut r = Rect { x: 0, y: 0, width: 0, height: 0 };
        check(unsafe { ffi::compeg_region_fit(src.0, src.1, out.0, out.1, align as std::os::raw::c_uint, &mut r) })?;
        Ok(r)
    }

    fn raw(&self) -> ffi::compeg_region {
        let zero = Rect { x: 0, y: 0, width: 0, height: 0 };
        ffi::compeg_region { image: self.image, reserved: 0, src: self.src.unwrap_or(zero), dst: self.dst.unwrap_or(zero) }
    }

    /// `(pre_width, pre_height, bytes)`: the extent of the block-averaged crop that the filter reads, and one slot in
    /// bytes, for this region of a `width` x `height` image; checked as the pack calls check it, all but `image`.
    pub fn shape(&self, tensor: &TensorSpec, resize: &ResizeSpec, width: u32, height: u32) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe { ffi::compeg_region_tensor_shape(&tensor.raw(), &resize.raw(), width, height, &self.raw(), &mut w, &mut h, &mut n) })?;
        Ok((w, h, n))
    }
}

/// Resampling kernel of a filtered pack (`COMPEG_FILTER_*`): PIL's `Image.resize` filters, each widened with the
/// reduction.  `Triangle` is PIL's BILINEAR, `Bicubic` (a = -0.5) PIL's BICUBIC and torch's bicubic with
/// `antialias=True`, `Lanczos3` PIL's LANCZOS.  The block-averaged crop may be 128, 64, 32 and 21 times the inner
/// rectangle at the most either way.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum FilterKernel {
    Box = 0,
    Triangle = 1,
    Bicubic = 2,
    Lanczos3 = 3,
}

/// The fixed output extent and the kernel of `Decoder::pack_tensor_filtered` / `Batch::pack_tensor_filtered`
/// (extension; compeg_hip.h, "Filtered tensor output").
#[derive(Clone, Copy, Debug)]
pub struct FilterSpec {
    pub width: u32,
    pub height: u32,
    pub kernel: FilterKernel,
}

impl FilterSpec {
    pub fn new(width: u32, height: u32, kernel: FilterKernel) -> Self {
        FilterSpec { width, height, kernel }
    }

    fn raw(&self) -> ffi::compeg_filter_spec {
        ffi::compeg_filter_spec { out_width: self.width, out_height: self.height, kernel: self.kernel as u32, reserved: 0 }
    }

    /// `(pre_width, pre_height, bytes)`: `Region::shape` for the filtered calls, the kernel's tap limit checked against
    /// the region's inner rectangle; no device needed.
    pub fn shape(&self, tensor: &TensorSpec, region: &Region, width: u32, height: u32) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe { ffi::compeg_filtered_tensor_shape(&tensor.raw(), &self.raw(), width, height, &region.raw(), &mut w, &mut h, &mut n) })?;
        Ok((w, h, n))
    }
}

/// The orientation of one slot of an oriented pack (compeg_hip.h, "Oriented tensor output"): the EXIF values, named by
/// what has to be done to the stored raster to see it upright, or `Exif` for the image's own tag.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum Orientation {
    Exif = 0,
    Normal = 1,
    Mirror = 2,
    Rotate180 = 3,
    Flip = 4,
    Transpose = 5,
    Rotate90 = 6,
    Transverse = 7,
    Rotate270 = 8,
}

impl Orientation {
    /// The orientation of an EXIF value 1..8 (`ImageData::orientation`); anything else is `Normal`.
    pub fn from_tag(tag: u32) -> Self {
        use Orientation::*;
        [Normal, Normal, Mirror, Rotate180, Flip, Transpose, Rotate90, Transverse, Rotate270].get(tag as usize).copied().unwrap_or(Normal)
    }

    /// The rectangle of the stored raster that holds the pixels of `upright`, a rectangle of the upright image of
    /// `size` = (width, height): what goes into `Region::src` for a crop chosen on the upright image.  Not for `Exif`.
    pub fn stored_rect(self, size: (u32, u32), upright: &Rect) -> Result<Rect> {
        let mut r = Rect { x: 0, y: 0, width: 0, height: 0 };
        check(unsafe { ffi::compeg_orient_rect(size.0, size.1, self as u32, upright, &mut r) })?;
        Ok(r)
    }
}

/// One output slot of `Decoder::pack_tensor_oriented` / `Batch::pack_tensor_oriented`: `region.src` in the stored raster,
/// `region.dst` in the upright slot.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct OrientedRegion {
    pub region: Region,
    pub orientation: Orientation,
}

impl OrientedRegion {
    fn raw(&self) -> ffi::compeg_oriented_region {
        ffi::compeg_oriented_region { region: self.region.raw(), orientation: self.orientation as u32, reserved: 0 }
    }

    /// `(pre_width, pre_height, bytes)`: `FilterSpec::shape` for the oriented calls -- `filter`'s extent is the upright
    /// slot, the tap limit is taken along the stored axes; `Exif` counts as `Normal` here.  No device needed.
    pub fn shape(&self, tensor: &TensorSpec, filter: &FilterSpec, width: u32, height: u32) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe { ffi::compeg_oriented_tensor_shape(&tensor.raw(), &filter.raw(), width, height, &self.raw(), &mut w, &mut h, &mut n) })?;
        Ok((w, h, n))
    }
}

/// The layout of `Decoder::pack_tensor_nhwc` / `Batch::pack_tensor_nhwc` (compeg_hip.h, "Channels-last tensor output"):
/// the destination is `[count][oh][ow][channels]`; with four channels element 3 of every pixel is `fill`.
#[derive(Clone, Copy, Debug, PartialEq)]
pub enum NhwcSpec {
    /// Three elements a pixel, in the tensor spec's order.
    Three,
    /// Four: the fourth is this value, converted to the element type like any other, with neither scale nor bias.
    Four { fill: f32 },
}

impl NhwcSpec {
    fn raw(&self) -> ffi::compeg_nhwc_spec {
        match *self {
            NhwcSpec::Three => ffi::compeg_nhwc_spec { channels: 3, fill: 0.0, reserved: [0; 2] },
            NhwcSpec::Four { fill } => ffi::compeg_nhwc_spec { channels: 4, fill, reserved: [0; 2] },
        }
    }

    /// `(pre_width, pre_height, bytes)`: `OrientedRegion::shape` for the channels-last calls.  No device needed.
    pub fn shape(&self, tensor: &TensorSpec, filter: &FilterSpec, width: u32, height: u32, region: &OrientedRegion) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe {
            ffi::compeg_nhwc_tensor_shape(&tensor.raw(), &filter.raw(), &self.raw(), width, height, &region.raw(), &mut w, &mut h, &mut n)
        })?;
        Ok((w, h, n))
    }
}

/// The format of a planes decode (compeg_hip.h, "Planar YCbCr output").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PlanesFormat {
    /// Y, then Cb, then Cr: I422 / I444 / I440 / I420 / Y800 by the file's sampling.
    Planar,
    /// Y, then interleaved Cb Cr pairs: NV16 / NV24 / NV12.
    Semiplanar,
    /// One packed plane, 4:2:2 files only.
    Yuyv,
    Uyvy,
}

/// What `Decoder::decode_planes` / `Batch::decode_planes` write: the format, whether 4:2:2 chroma is averaged to 4:2:0
/// (planar and semiplanar formats, 4:2:2 files only), and the row pitches in bytes (0 = tight).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct PlanesSpec {
    pub format: PlanesFormat,
    pub chroma_420: bool,
    pub luma_pitch: u32,
    pub chroma_pitch: u32,
}

impl PlanesSpec {
    pub fn new(format: PlanesFormat) -> Self {
        PlanesSpec { format, chroma_420: false, luma_pitch: 0, chroma_pitch: 0 }
    }

    fn raw(&self) -> ffi::compeg_planes_spec {
        let format = match self.format {
            PlanesFormat::Planar => ffi::COMPEG_PLANES_PLANAR,
            PlanesFormat::Semiplanar => ffi::COMPEG_PLANES_SEMIPLANAR,
            PlanesFormat::Yuyv => ffi::COMPEG_PLANES_YUYV,
            PlanesFormat::Uyvy => ffi::COMPEG_PLANES_UYVY,
        };
        let chroma = if self.chroma_420 { ffi::COMPEG_CHROMA_420 } else { ffi::COMPEG_CHROMA_AS_CODED };
        ffi::compeg_planes_spec { format, chroma, luma_pitch: self.luma_pitch, chroma_pitch: self.chroma_pitch, reserved: [0; 4] }
    }
}

/// No device needed: one image's planes for a `width x height` image of `components` components (3, or 1: grayscale)
/// whose luma is sampled `sampling` (`ImageData::sampling`).
pub fn planes_shape(spec: &PlanesSpec, width: u32, height: u32, components: u32, sampling: (u32, u32)) -> Result<ffi::compeg_planes_layout> {
    let mut layout = ffi::compeg_planes_layout::default();
    check(unsafe { ffi::compeg_planes_shape(&spec.raw(), width, height, components, sampling.0, sampling.1, &mut layout) })?;
    Ok(layout)
}

/// The format of a reduced decode (compeg_hip.h, "Reduced-size decode").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ReducedFormat {
    /// Interleaved R G B A, A = 255; address and pitch multiples of 4.
    Rgba,
    /// `[3, oh, ow]` bytes, tight: a CHW u8 tensor.
    RgbPlanar,
}

/// What `Decoder::decode_reduced` / `Batch::decode_reduced` write: the image at 1/8 scale, one RGB pixel per luma data
/// unit from the DC terms alone.  `pitch`: the RGBA rows' pitch in bytes, 0 = tight.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ReducedSpec {
    pub format: ReducedFormat,
    pub pitch: u32,
}

/// `reduced_shape`'s answer: the reduced extent, the pitch in use and one image's bytes.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ReducedShape {
    pub width: u32,
    pub height: u32,
    pub pitch: u32,
    pub total_bytes: u64,
}

impl ReducedSpec {
    pub fn new(format: ReducedFormat) -> Self {
        ReducedSpec { format, pitch: 0 }
    }

    fn raw(&self) -> ffi::compeg_reduced_spec {
        let format = match self.format {
            ReducedFormat::Rgba => ffi::COMPEG_REDUCED_RGBA,
            ReducedFormat::RgbPlanar => ffi::COMPEG_REDUCED_RGB_PLANAR,
        };
        ffi::compeg_reduced_spec { denominator: 8, format, pitch: self.pitch }
    }
}

/// No device needed: the 1/8-scale extent and size of a `width x height` image.
pub fn reduced_shape(spec: &ReducedSpec, width: u32, height: u32) -> Result<ReducedShape> {
    let mut s = ReducedShape { width: 0, height: 0, pitch: 0, total_bytes: 0 };
    check(unsafe { ffi::compeg_reduced_shape(&spec.raw(), width, height, &mut s.width, &mut s.height, &mut s.pitch, &mut s.total_bytes) })?;
    Ok(s)
}

/// The format of a scaled decode (compeg_hip.h, "Scaled decode").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ScaledFormat {
    /// Interleaved R G B A, A = 255; address and pitch multiples of 4.
    Rgba,
    /// `[3, oh, ow]` bytes, tight: a CHW u8 tensor.
    RgbPlanar,
}

/// What `Decoder::decode_scaled` / `Batch::decode_scaled` write: the image at 1 / `denominator` (2, 4 or 8; the library
/// refuses any other), N x N pixels per luma data unit, N = 8 / denominator, from the N-point inverse DCT of each data
/// unit's N x N lowest frequencies (IJG libjpeg's scaled IDCT in pinned f32 arithmetic) -- neither the block mean of the
/// full decode nor libjpeg-turbo's output.  Denominator 8 is the reduced decode.  `pitch`: the RGBA rows' pitch in
/// bytes, 0 = tight.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ScaledSpec {
    pub denominator: u32,
    pub format: ScaledFormat,
    pub pitch: u32,
}

/// `scaled_shape`'s answer: the scaled extent, the pitch in use and one image's bytes.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct ScaledShape {
    pub width: u32,
    pub height: u32,
    pub pitch: u32,
    pub total_bytes: u64,
}

impl ScaledSpec {
    pub fn new(denominator: u32, format: ScaledFormat) -> Self {
        ScaledSpec { denominator, format, pitch: 0 }
    }

    fn raw(&self) -> ffi::compeg_scaled_spec {
        let format = match self.format {
            ScaledFormat::Rgba => ffi::COMPEG_SCALED_RGBA,
            ScaledFormat::RgbPlanar => ffi::COMPEG_SCALED_RGB_PLANAR,
        };
        ffi::compeg_scaled_spec { denominator: self.denominator, format, pitch: self.pitch }
    }
}

/// No device needed: the extent and size of a `width x height` image at the spec's scale.
pub fn scaled_shape(spec: &ScaledSpec, width: u32, height: u32) -> Result<ScaledShape> {
    let mut s = ScaledShape { width: 0, height: 0, pitch: 0, total_bytes: 0 };
    check(unsafe { ffi::compeg_scaled_shape(&spec.raw(), width, height, &mut s.width, &mut s.height, &mut s.pitch, &mut s.total_bytes) })?;
    Ok(s)
}

/// The order of a block's 64 values in a levels decode (compeg_hip.h, "Levels decode").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum LevelsOrder {
    /// The file's zig-zag order.
    Zigzag,
    /// Row-major 8 x 8, the horizontal frequency fastest (libjpeg's `JBLOCK`).
    Natural,
}

impl LevelsOrder {
    fn raw(self) -> u32 {
        match self {
            LevelsOrder::Zigzag => ffi::COMPEG_LEVELS_ZIGZAG,
            LevelsOrder::Natural => ffi::COMPEG_LEVELS_NATURAL,
        }
    }
}

/// What `Decoder::decode_levels` / `Batch::decode_levels` write: the file's quantised DCT coefficients (levels) as
/// `i16` blocks of 64, per component `[blocks_h][blocks_w][64]`, whole MCUs -- every value as the entropy decode yields it
/// (not multiplied by the quantiser; position 0 the DC predictor's low 16 bits; all 64 positions kept).
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct LevelsSpec {
    pub order: LevelsOrder,
}

impl LevelsSpec {
    pub fn new(order: LevelsOrder) -> Self {
        LevelsSpec { order }
    }

    fn raw(&self) -> ffi::compeg_levels_spec {
        ffi::compeg_levels_spec { order: self.order.raw(), reserved: [0; 3] }
    }
}

/// No device needed: where the blocks of a `width x height` image of `components` components (3, or 1: grayscale)
/// whose luma is sampled `sampling` (`ImageData::sampling`) lie, and how many bytes one image takes.
pub fn levels_shape(spec: &LevelsSpec, width: u32, height: u32, components: u32, sampling: (u32, u32)) -> Result<ffi::compeg_levels_layout> {
    let mut layout = ffi::compeg_levels_layout::default();
    check(unsafe { ffi::compeg_levels_shape(&spec.raw(), width, height, components, sampling.0, sampling.1, &mut layout) })?;
    Ok(layout)
}

/// The format of a cropped decode (compeg_hip.h, "Cropped decode").
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CropFormat {
    /// Interleaved R G B A, A = 255; address and pitch multiples of 4.
    Rgba,
    /// `[3, height, width]` bytes, tight: a CHW u8 tensor.
    RgbPlanar,
}

/// What `Decoder::decode_cropped` / `Batch::decode_cropped` write: the rectangle `width x height` at `(x, y)` of the image
/// -- non-empty, inside it -- pixel for pixel what the RGBA decode has there.  `pitch`: the RGBA rows' pitch in bytes,
/// 0 = tight.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct CropSpec {
    pub x: u32,
    pub y: u32,
    pub width: u32,
    pub height: u32,
    pub format: CropFormat,
    pub pitch: u32,
}

/// `crop_shape`'s answer: the pitch in use and one image's bytes.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct CropShape {
    pub pitch: u32,
    pub total_bytes: u64,
}

impl CropSpec {
    pub fn new(x: u32, y: u32, width: u32, height: u32, format: CropFormat) -> Self {
        CropSpec { x, y, width, height, format, pitch: 0 }
    }

    fn raw(&self) -> ffi::compeg_crop_spec {
        let format = match self.format {
            CropFormat::Rgba => ffi::COMPEG_CROP_RGBA,
            CropFormat::RgbPlanar => ffi::COMPEG_CROP_RGB_PLANAR,
        };
        ffi::compeg_crop_spec { x: self.x, y: self.y, width: self.width, height: self.height, format, pitch: self.pitch, reserved: [0; 2] }
    }
}

/// No device needed: checks the rectangle against an `image_width x image_height` image and gives the destination's size.
pub fn crop_shape(spec: &CropSpec, image_width: u32, image_height: u32) -> Result<CropShape> {
    let mut s = CropShape { pitch: 0, total_bytes: 0 };
    check(unsafe { ffi::compeg_crop_shape(&spec.raw(), image_width, image_height, &mut s.pitch, &mut s.total_bytes) })?;
    Ok(s)
}

/// The weights of `Decoder::pack_tensor_luma` / `Batch::pack_tensor_luma` (compeg_hip.h, "Luma tensor output"): per source
/// pixel `L = (wR R + wG G + wB B + 32768) >> 16`; the destination is `[count][1][oh][ow]`.  A grayscale frame gives its
/// own values under any of them.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum LumaSpec {
    /// {19595, 38470, 7471}: PIL's `Image.convert("L")`, byte for byte.
    Bt601,
    /// {13933, 46871, 4732}.
    Bt709,
    /// R, G or B alone.
    Red,
    Green,
    Blue,
    /// For R, G and B: each 0..=65536, their sum exactly 65536 (the library checks).
    Weights([u32; 3]),
}

impl LumaSpec {
    fn raw(&self) -> ffi::compeg_luma_spec {
        let weights = match *self {
            LumaSpec::Bt601 => [19595, 38470, 7471],
            LumaSpec::Bt709 => [13933, 46871, 4732],
            LumaSpec::Red => [65536, 0, 0],
            LumaSpec::Green => [0, 65536, 0],
            LumaSpec::Blue => [0, 0, 65536],
            LumaSpec::Weights(w) => w,
        };
        ffi::compeg_luma_spec { weights, reserved: 0 }
    }

    /// `(pre_width, pre_height, bytes)`: `OrientedRegion::shape` for the luma calls, a third of its bytes.  No device needed.
    pub fn shape(&self, tensor: &TensorSpec, filter: &FilterSpec, width: u32, height: u32, region: &OrientedRegion) -> Result<(u32, u32, usize)> {
        let (mut w, mut h, mut n) = (0, 0, 0);
        check(unsafe {
            ffi::compeg_luma_tensor_shape(&tensor.raw(), &filter.raw(), &self.raw(), width, height, &region.raw(), &mut w, &mut h, &mut n)
        })?;
        Ok((w, h, n))
    }
}

/// Device + stream + loaded gfx950 code object.  Immutable after creation and
/// reference-counted inside the library; share it as `Arc<Gpu>` like the reference.
pub struct Gpu {
    raw: NonNull<ffi::compeg_gpu>,
}

unsafe impl Send for Gpu {}
unsafe impl Sync for Gpu {}

impl Gpu {
    /// Opens the default device.  `async` only to keep the reference's signature.
    pub async fn open() -> Result<Self> {
        Self::open_device(-1)
    }

    /// Opens HIP device `index` (-1 = current default).
    pub fn open_device(index: i32) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::compeg_gpu_open(index, &mut raw) })?;
        Ok(Gpu { raw: NonNull::new(raw).expect("compeg_gpu_open returned null") })
    }

    /// The `from_wgpu` analogue: work is recorded on a stream the caller owns.
    ///
    /// # Safety
    /// `stream` must be a valid `hipStream_t` of device `device` and outlive the `Gpu`.
    pub unsafe fn from_stream(device: i32, stream: Stream) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(ffi::compeg_gpu_from_stream(device, stream.0, &mut raw))?;
        Ok(Gpu { raw: NonNull::new(raw).expect("compeg_gpu_from_stream returned null") })
    }

    pub fn device(&self) -> i32 {
        unsafe { ffi::compeg_gpu_device(self.raw.as_ptr()) }
    }

    pub fn name(&self) -> String {
        unsafe { CStr::from_ptr(ffi::compeg_gpu_name(self.raw.as_ptr())) }.to_string_lossy().into_owned()
    }
}

impl Drop for Gpu {
    fn drop(&mut self) {
        unsafe { ffi::compeg_gpu_release(self.raw.as_ptr()) }
    }
}

/// Extensions of `ImageData::with_flags`; all off = the reference's behaviour.
#[derive(Clone, Copy, Default)]
pub struct ParseFlags {
    /// 4:4:4, 4:4:0 and 4:2:0 are accepted as well as 4:2:2.
    pub any_luma_sampling: bool,
    /// Bit reader topped up in front of DC codes, ZRL = 16 positions (ITU-T T.81).
    pub standard_entropy: bool,
    /// Frames with one component are accepted: R = G = B = the luma sample.
    pub grayscale: bool,
}

/// A parsed and validated JPEG (baseline, 8 bit, YCbCr 4:2:2, restart intervals).
/// Borrows or owns the bytes exactly like the reference's `Cow`.
pub struct ImageData<'a> {
    raw: NonNull<ffi::compeg_image>,
    _jpeg: Cow<'a, [u8]>,
}

unsafe impl Send for ImageData<'_> {}
unsafe impl Sync for ImageData<'_> {}

impl<'a> ImageData<'a> {
    pub fn new(jpeg: impl Into<Cow<'a, [u8]>>) -> Result<Self> {
        let jpeg = jpeg.into();
        let mut raw = ptr::null_mut();
        // copy = 0: `_jpeg` keeps the bytes alive for as long as the handle exists
        check(unsafe { ffi::compeg_image_parse(jpeg.as_ptr(), jpeg.len(), 0, &mut raw) })?;
        Ok(ImageData { raw: NonNull::new(raw).expect("compeg_image_parse returned null"), _jpeg: jpeg })
    }

    /// Extension: like `new`, but 4:4:4, 4:4:0 and 4:2:0 are accepted as well as 4:2:2.
    pub fn new_any_sampling(jpeg: impl Into<Cow<'a, [u8]>>) -> Result<Self> {
        Self::with_flags(jpeg, ParseFlags { any_luma_sampling: true, ..ParseFlags::default() })
    }

    /// Extension: `ParseFlags` widen the accepted subset / switch the entropy decoder to ITU-T T.81
    /// behaviour where the reference deviates (see `include/compeg_hip.h`).
    pub fn with_flags(jpeg: impl Into<Cow<'a, [u8]>>, flags: ParseFlags) -> Result<Self> {
        let jpeg = jpeg.into();
        let mut raw = ptr::null_mut();
        let bits = if flags.any_luma_sampling { ffi::COMPEG_PARSE_ANY_LUMA_SAMPLING } else { 0 }
            | if flags.standard_entropy { ffi::COMPEG_PARSE_STANDARD_ENTROPY } else { 0 }
            | if flags.grayscale { ffi::COMPEG_PARSE_GRAYSCALE } else { 0 };
        check(unsafe { ffi::compeg_image_parse_ext(jpeg.as_ptr(), jpeg.len(), 0, bits, &mut raw) })?;
        Ok(ImageData { raw: NonNull::new(raw).expect("compeg_image_parse_ext returned null"), _jpeg: jpeg })
    }

    pub fn width(&self) -> u32 {
        unsafe { ffi::compeg_image_width(self.raw.as_ptr()) }
    }

    pub fn height(&self) -> u32 {
        unsafe { ffi::compeg_image_height(self.raw.as_ptr()) }
    }

    /// Number of restart intervals = lanes that decode in parallel.
    pub fn parallelism(&self) -> u32 {
        unsafe { ffi::compeg_image_parallelism(self.raw.as_ptr()) }
    }

    /// Extension: components of the frame -- 3, or 1 for a grayscale image (`ParseFlags::grayscale`).
    pub fn components(&self) -> u32 {
        unsafe { ffi::compeg_image_components(self.raw.as_ptr()) }
    }

    /// Extension: the luma component's sampling factors (h, v) -- (2, 1) for 4:2:2, (1, 1) for 4:4:4 and grayscale,
    /// (1, 2) for 4:4:0, (2, 2) for 4:2:0: what `planes_shape` sizes the planes with.
    pub fn sampling(&self) -> (u32, u32) {
        let (mut h, mut v) = (0, 0);
        unsafe { ffi::compeg_image_sampling(self.raw.as_ptr(), &mut h, &mut v) };
        (h, v)
    }

    /// Extension: the 64 quantisation factors of component `component` in `order` -- what a level of `decode_levels` is
    /// multiplied by to give the coefficient.
    pub fn quant_table(&self, component: u32, order: LevelsOrder) -> Result<[u16; 64]> {
        let mut q = [0u16; 64];
        check(unsafe { ffi::compeg_image_quant_table(self.raw.as_ptr(), component, q.as_mut_ptr(), order.raw()) })?;
        Ok(q)
    }

    /// Extension: the file's EXIF orientation tag, 1..8; 1 where it has no usable one.
    pub fn orientation(&self) -> u32 {
        unsafe { ffi::compeg_image_orientation(self.raw.as_ptr()) }
    }
}

impl Drop for ImageData<'_> {
    fn drop(&mut self) {
        unsafe { ffi::compeg_image_free(self.raw.as_ptr()) }
    }
}

/// The decoder's output: RGBA8 (`R, G, B, 255`), row-major, resident in HBM.
/// Like the reference's texture it never shrinks, so `width`/`height` may
/// exceed the last image; only that image's own corner is defined.
#[derive(Clone, Copy)]
pub struct Texture<'a> {
    pub device_ptr: *mut c_void,
    pub width: u32,
    pub height: u32,
    pub pitch_bytes: usize,
    _owner: PhantomData<&'a ()>,
}

/// `Decoder::into_texture()`: the allocation now belongs to the caller.
pub struct OwnedTexture {
    pub device_ptr: *mut c_void,
    pub width: u32,
    pub height: u32,
    pub pitch_bytes: usize,
}

unsafe impl Send for OwnedTexture {}

impl Drop for OwnedTexture {
    fn drop(&mut self) {
        unsafe { ffi::compeg_device_free(self.device_ptr) }
    }
}

/// Owns all device buffers of one decode pipeline and a reusable scan buffer.
/// Every method takes `&mut self`: one thread at a time per decoder, many decoders per `Gpu`.
pub struct Decoder {
    raw: NonNull<ffi::compeg_decoder>,
    _gpu: Arc<Gpu>,
}

unsafe impl Send for Decoder {}

impl Decoder {
    pub fn new(gpu: Arc<Gpu>) -> Self {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::compeg_decoder_new(gpu.raw.as_ptr(), &mut raw) }).expect("compeg_decoder_new");
        Decoder { raw: NonNull::new(raw).expect("compeg_decoder_new returned null"), _gpu: gpu }
    }

    /// Extension: run the scan preprocessing on the GPU (the raw entropy-coded
    /// segment is uploaded instead of the preprocessed one).  Same results.
    pub fn set_device_preprocess(&mut self, on: bool) {
        check(unsafe { ffi::compeg_decoder_set_device_preprocess(self.raw.as_ptr(), on as c_int) })
            .expect("compeg_decoder_set_device_preprocess");
    }

    /// Extension: threads of this decoder's host scan preprocessor (1..=16).
    pub fn set_scan_threads(&mut self, threads: u32) {
        check(unsafe { ffi::compeg_decoder_set_scan_threads(self.raw.as_ptr(), threads as std::os::raw::c_uint) })
            .expect("compeg_decoder_set_scan_threads");
    }

    /// Preprocesses, uploads and records the decode on `stream` without
    /// waiting; returns whether the output was reallocated (always on the
    /// first call).  The reference records into a `CommandEncoder` here.
    pub fn enqueue(&mut self, data: &ImageData<'_>, stream: Stream) -> bool {
        let mut changed = 0;
        check(unsafe { ffi::compeg_decoder_enqueue(self.raw.as_ptr(), data.raw.as_ptr(), stream.0, &mut changed) })
            .expect("compeg_decoder_enqueue");
        changed != 0
    }

    /// Enqueues on the `Gpu`'s own stream and submits; returns at once.
    pub fn start_decode(&mut self, data: &ImageData<'_>) -> DecodeOp<'_> {
        let mut op = ptr::null_mut();
        check(unsafe { ffi::compeg_decoder_start_decode(self.raw.as_ptr(), data.raw.as_ptr(), &mut op) })
            .expect("compeg_decoder_start_decode");
        DecodeOp { raw: NonNull::new(op).expect("null op"), decoder: self }
    }

    /// `start_decode` + wait.
    pub fn decode_blocking(&mut self, data: &ImageData<'_>) -> DecodeOp<'_> {
        let mut op = ptr::null_mut();
        check(unsafe { ffi::compeg_decoder_decode_blocking(self.raw.as_ptr(), data.raw.as_ptr(), &mut op) })
            .expect("compeg_decoder_decode_blocking");
        DecodeOp { raw: NonNull::new(op).expect("null op"), decoder: self }
    }

    /// The reference drops a restart-interval count mismatch silently; here it can be read back.
    pub fn last_warning(&self) -> Option<String> {
        let p = unsafe { ffi::compeg_decoder_last_warning(self.raw.as_ptr()) };
        if p.is_null() {
            return None;
        }
        let s = unsafe { CStr::from_ptr(p) }.to_string_lossy();
        if s.is_empty() { None } else { Some(s.into_owned()) }
    }

    /// Host time of the stages of the last decode: what the reference traces as `t_preprocess`,
    /// `t_enqueue_writes` and `t_poll` (src/lib.rs:391-396,452-475,516-522).
    pub fn last_stage_times(&self) -> ffi::compeg_stage_times {
        let mut t = ffi::compeg_stage_times::default();
        check(unsafe { ffi::compeg_decoder_last_stage_times(self.raw.as_ptr(), &mut t) })
            .expect("compeg_decoder_last_stage_times");
        t
    }

    pub fn texture(&self) -> Texture<'_> {
        let (mut p, mut w, mut h, mut pitch) = (ptr::null_mut(), 0, 0, 0);
        check(unsafe { ffi::compeg_decoder_output(self.raw.as_ptr(), &mut p, &mut w, &mut h, &mut pitch) })
            .expect("compeg_decoder_output");
        Texture { device_ptr: p, width: w, height: h, pitch_bytes: pitch, _owner: PhantomData }
    }

    pub fn into_texture(self) -> OwnedTexture {
        let (mut p, mut w, mut h, mut pitch) = (ptr::null_mut(), 0, 0, 0);
        // compeg_decoder_take_output frees the decoder: skip our Drop
        let raw = self.raw;
        let gpu = unsafe { ptr::read(&self._gpu) };
        std::mem::forget(self);
        let rc = unsafe { ffi::compeg_decoder_take_output(raw.as_ptr(), &mut p, &mut w, &mut h, &mut pitch) };
        drop(gpu);
        check(rc).expect("compeg_decoder_take_output");
        OwnedTexture { device_ptr: p, width: w, height: h, pitch_bytes: pitch }
    }

    /// Extension: records on `stream` the pack of the last decoded image into `[3, h, w]` at `device_dst`
    /// (caller-owned device memory of `dst_bytes` bytes) and returns without waiting; the pack runs behind the
    /// decode, the next decode behind the pack.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor(&mut self, spec: &TensorSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_pack_tensor(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Extension: like `pack_tensor`, with `crop` of the last decoded image (`None`: all of it) resized to the extent of
    /// `resize`, giving `[3, resize.height, resize.width]` at `device_dst`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_resized(&mut self, spec: &TensorSpec, resize: &ResizeSpec, crop: Option<&Rect>, device_dst: *mut c_void,
                                      dst_bytes: usize, stream: Stream) -> Result<()> {
        let crop = crop.map_or(ptr::null(), |c| c as *const Rect);
        check(ffi::compeg_decoder_pack_tensor_resized(self.raw.as_ptr(), &spec.raw(), &resize.raw(), crop, device_dst, dst_bytes, stream.0))
    }

    /// Extension: like `pack_tensor_resized`, for a list of regions of the last decoded image (`Region::image` 0), giving
    /// `[regions.len(), 3, resize.height, resize.width]` at `device_dst`.  `pad`: R, G, B on the pixel scale (`None`:
    /// zeros), put through the spec's scale and bias like every other element.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_regions(&mut self, spec: &TensorSpec, resize: &ResizeSpec, regions: &[Region], pad: Option<&[f32; 3]>,
                                      device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_region> = regions.iter().map(Region::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_decoder_pack_tensor_regions(self.raw.as_ptr(), &spec.raw(), &resize.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                      dst_bytes, stream.0))
    }

    /// Extension: `pack_tensor_regions` with one of the four resampling kernels of `FilterSpec`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_filtered(&mut self, spec: &TensorSpec, filter: &FilterSpec, regions: &[Region], pad: Option<&[f32; 3]>,
                                       device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_region> = regions.iter().map(Region::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_decoder_pack_tensor_filtered(self.raw.as_ptr(), &spec.raw(), &filter.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                       dst_bytes, stream.0))
    }

    /// Extension: `pack_tensor_filtered` with an orientation per region; `filter`'s extent is the upright slot.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_oriented(&mut self, spec: &TensorSpec, filter: &FilterSpec, regions: &[OrientedRegion], pad: Option<&[f32; 3]>,
                                       device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_decoder_pack_tensor_oriented(self.raw.as_ptr(), &spec.raw(), &filter.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                       dst_bytes, stream.0))
    }

    /// Extension: `pack_tensor_oriented` into a channels-last destination, `[count][oh][ow][C]`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_nhwc(&mut self, spec: &TensorSpec, filter: &FilterSpec, nhwc: &NhwcSpec, regions: &[OrientedRegion],
                                   pad: Option<&[f32; 3]>, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_decoder_pack_tensor_nhwc(self.raw.as_ptr(), &spec.raw(), &filter.raw(), &nhwc.raw(), raw.as_ptr(), raw.len(), pad,
                                                   device_dst, dst_bytes, stream.0))
    }

    /// Extension: `pack_tensor_oriented` with one channel a slot, `[count][1][oh][ow]`; `pad` is one value; of `spec`'s
    /// scale and bias element 0 is read.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_luma(&mut self, spec: &TensorSpec, filter: &FilterSpec, luma: &LumaSpec, regions: &[OrientedRegion],
                                   pad: Option<f32>, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.as_ref().map_or(ptr::null(), |p| p as *const f32);
        check(ffi::compeg_decoder_pack_tensor_luma(self.raw.as_ptr(), &spec.raw(), &filter.raw(), &luma.raw(), raw.as_ptr(), raw.len(), pad,
                                                   device_dst, dst_bytes, stream.0))
    }

    /// Extension: uploads and preprocesses `image` as `enqueue` does and records a decode that writes the file's own
    /// Y, Cb and Cr samples into caller-owned device memory as `planes_shape` lays them out -- no colour step, no
    /// upsampling.  The texture and what the packs read are not touched.  Returns without waiting: synchronise `stream`,
    /// or use `decode_planes_blocking`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_planes(&mut self, image: &ImageData, spec: &PlanesSpec, device_dst: *mut c_void, dst_bytes: usize,
                                stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_decode_planes(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// `decode_planes` on the gpu's own stream, and the wait for it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes.
    pub unsafe fn decode_planes_blocking(&mut self, image: &ImageData, spec: &PlanesSpec, device_dst: *mut c_void,
                                         dst_bytes: usize) -> Result<()> {
        check(ffi::compeg_decoder_decode_planes_blocking(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes))
    }

    /// Extension: uploads and preprocesses `image` as `enqueue` does and records, on `stream`, a decode at 1/8 scale
    /// into caller-owned device memory as `reduced_shape` lays it out.  The texture and what the packs read are not
    /// touched.  Returns without waiting: synchronise `stream`, or use `decode_reduced_blocking`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_reduced(&mut self, image: &ImageData, spec: &ReducedSpec, device_dst: *mut c_void, dst_bytes: usize,
                                 stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_decode_reduced(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// `decode_reduced` on the gpu's own stream, and the wait for it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes.
    pub unsafe fn decode_reduced_blocking(&mut self, image: &ImageData, spec: &ReducedSpec, device_dst: *mut c_void,
                                          dst_bytes: usize) -> Result<()> {
        check(ffi::compeg_decoder_decode_reduced_blocking(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes))
    }

    /// Extension: uploads and preprocesses `image` as `enqueue` does and records, on `stream`, a decode at the spec's
    /// scale (1/2, 1/4 or 1/8) into caller-owned device memory as `scaled_shape` lays it out.  The texture and what the
    /// packs read are not touched.  Returns without waiting: synchronise `stream`, or use `decode_scaled_blocking`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_scaled(&mut self, image: &ImageData, spec: &ScaledSpec, device_dst: *mut c_void, dst_bytes: usize,
                                stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_decode_scaled(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Extension: uploads and preprocesses `image` as `enqueue` does and records on `stream` a decode of its quantised DCT
    /// coefficients (levels) into caller-owned device memory as `levels_shape` lays it out.  The texture and what the
    /// packs read are not touched.  Returns without waiting: synchronise `stream`, or use `decode_levels_blocking`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes, at an address that is a multiple of 16, that stays
    /// valid until the stream has run.
    pub unsafe fn decode_levels(&mut self, image: &ImageData, spec: &LevelsSpec, device_dst: *mut c_void, dst_bytes: usize,
                                stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_decode_levels(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// `decode_levels` on the gpu's own stream, and the wait for it.
    ///
    /// # Safety
    /// As for `decode_levels`.
    pub unsafe fn decode_levels_blocking(&mut self, image: &ImageData, spec: &LevelsSpec, device_dst: *mut c_void,
                                         dst_bytes: usize) -> Result<()> {
        check(ffi::compeg_decoder_decode_levels_blocking(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes))
    }

    /// `decode_scaled` on the gpu's own stream, and the wait for it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes.
    pub unsafe fn decode_scaled_blocking(&mut self, image: &ImageData, spec: &ScaledSpec, device_dst: *mut c_void,
                                         dst_bytes: usize) -> Result<()> {
        check(ffi::compeg_decoder_decode_scaled_blocking(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes))
    }

    /// Extension: uploads and preprocesses `image` as `enqueue` does and records, on `stream`, a decode of the spec's
    /// rectangle into caller-owned device memory as `crop_shape` lays it out; restart intervals without an MCU in the
    /// rectangle are not decoded.  The texture and what the packs read are not touched.  Returns without waiting:
    /// synchronise `stream`, or use `decode_cropped_blocking`.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_cropped(&mut self, image: &ImageData, spec: &CropSpec, device_dst: *mut c_void, dst_bytes: usize,
                                 stream: Stream) -> Result<()> {
        check(ffi::compeg_decoder_decode_cropped(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// `decode_cropped` on the gpu's own stream, and the wait for it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes.
    pub unsafe fn decode_cropped_blocking(&mut self, image: &ImageData, spec: &CropSpec, device_dst: *mut c_void,
                                          dst_bytes: usize) -> Result<()> {
        check(ffi::compeg_decoder_decode_cropped_blocking(self.raw.as_ptr(), image.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes))
    }

    /// Test helper (the reference's tests copy the texture to a buffer): waits and
    /// returns the image's `width x height` corner, tightly packed.
    pub fn read_output(&mut self, width: u32, height: u32) -> Result<Vec<u8>> {
        let mut v = vec![0u8; width as usize * height as usize * 4];
        check(unsafe { ffi::compeg_decoder_read_output(self.raw.as_ptr(), v.as_mut_ptr(), width, height) })?;
        Ok(v)
    }
}

impl Drop for Decoder {
    fn drop(&mut self) {
        unsafe { ffi::compeg_decoder_free(self.raw.as_ptr()) }
    }
}

/// An in-flight decode; `wait` replaces polling the wgpu submission index.
pub struct DecodeOp<'a> {
    raw: NonNull<ffi::compeg_op>,
    decoder: &'a Decoder,
}

impl DecodeOp<'_> {
    pub fn wait(&self) {
        check(unsafe { ffi::compeg_op_wait(self.raw.as_ptr()) }).expect("compeg_op_wait");
    }

    pub fn texture(&self) -> Texture<'_> {
        self.decoder.texture()
    }

    pub fn texture_changed(&self) -> bool {
        unsafe { ffi::compeg_op_texture_changed(self.raw.as_ptr()) != 0 }
    }
}

impl Drop for DecodeOp<'_> {
    fn drop(&mut self) {
        unsafe { ffi::compeg_op_free(self.raw.as_ptr()) }
    }
}

/// Scan preprocessing on its own (the reference exposes it for its benchmark).
#[doc(hidden)]
pub struct ScanBuffer {
    raw: NonNull<ffi::compeg_scanbuffer>,
}

unsafe impl Send for ScanBuffer {}

impl ScanBuffer {
    pub fn new() -> Self {
        ScanBuffer { raw: NonNull::new(unsafe { ffi::compeg_scanbuffer_new() }).expect("compeg_scanbuffer_new") }
    }

    /// `Err` on a restart-interval count mismatch; the buffers then hold the truncated result.
    pub fn process(&mut self, scan_data: &[u8], expected_restart_intervals: u32) -> Result<()> {
        check(unsafe {
            ffi::compeg_scanbuffer_process(self.raw.as_ptr(), scan_data.as_ptr(), scan_data.len(), expected_restart_intervals)
        })
    }

    /// Extension: `threads` threads (1..=16) share every following `process` call; same bytes.
    pub fn set_threads(&mut self, threads: u32) -> Result<()> {
        check(unsafe { ffi::compeg_scanbuffer_set_threads(self.raw.as_ptr(), threads as std::os::raw::c_uint) })
    }

    /// Extension: the same bytes, computed by the device-side scan kernels.
    pub fn process_on_gpu(&mut self, gpu: &Gpu, scan_data: &[u8], expected_restart_intervals: u32) -> Result<()> {
        check(unsafe {
            ffi::compeg_scanbuffer_process_on_gpu(self.raw.as_ptr(), gpu.raw.as_ptr(), scan_data.as_ptr(), scan_data.len(),
                                                  expected_restart_intervals)
        })
    }

    pub fn processed_scan_data(&self) -> &[u8] {
        let mut n = 0;
        let p = unsafe { ffi::compeg_scanbuffer_data(self.raw.as_ptr(), &mut n) };
        if n == 0 { &[] } else { unsafe { std::slice::from_raw_parts(p, n) } }
    }

    pub fn start_positions(&self) -> &[u8] {
        let mut n = 0;
        let p = unsafe { ffi::compeg_scanbuffer_start_positions(self.raw.as_ptr(), &mut n) };
        if n == 0 { &[] } else { unsafe { std::slice::from_raw_parts(p, n) } }
    }
}

impl Default for ScanBuffer {
    fn default() -> Self {
        Self::new()
    }
}

impl Drop for ScanBuffer {
    fn drop(&mut self) {
        unsafe { ffi::compeg_scanbuffer_free(self.raw.as_ptr()) }
    }
}

/// Where a [`Batch`] preprocesses its scans.
#[derive(Clone, Copy, PartialEq, Eq)]
pub enum Preprocess {
    /// On the host during `upload`, like the reference.
    Host = 0,
    /// Raw segments are uploaded and preprocessed once by the scan kernels.
    DeviceOnce = 1,
    /// Every `decode` re-runs the scan kernels first (raw scan bytes in HBM -> RGBA).
    DeviceEveryDecode = 2,
}

/// Extension: many independent images decoded by one launch sequence.  The
/// images' scans and tables are made resident in HBM once; every `decode` is
/// pure device work.  Outputs are RGBA8 images, rows `pitch_bytes` apart (the width rounded up to 16 pixels).
pub struct Batch {
    raw: NonNull<ffi::compeg_batch>,
    _gpu: Arc<Gpu>,
}

unsafe impl Send for Batch {}

impl Batch {
    pub fn new(gpu: Arc<Gpu>) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::compeg_batch_new(gpu.raw.as_ptr(), &mut raw) })?;
        Ok(Batch { raw: NonNull::new(raw).expect("compeg_batch_new returned null"), _gpu: gpu })
    }

    /// Set before `upload`.
    pub fn set_preprocess(&mut self, mode: Preprocess) -> Result<()> {
        check(unsafe { ffi::compeg_batch_set_device_preprocess(self.raw.as_ptr(), mode as c_int) })
    }

    /// Host front-end for all images (`host_threads` = 0: one per core) + upload; replaces previous content.
    pub fn upload(&mut self, images: &[&ImageData<'_>], host_threads: usize) -> Result<()> {
        let raws: Vec<*const ffi::compeg_image> = images.iter().map(|i| i.raw.as_ptr() as *const _).collect();
        check(unsafe { ffi::compeg_batch_upload(self.raw.as_ptr(), raws.as_ptr(), raws.len(), host_threads as c_int) })
    }

    /// Images of the last upload that the scan kernels handed back to the host.
    pub fn host_fallbacks(&self) -> usize {
        unsafe { ffi::compeg_batch_host_fallbacks(self.raw.as_ptr()) }
    }

    /// Records the decode of every uploaded image on `stream` and returns without waiting.
    pub fn decode(&mut self, stream: Stream) -> Result<()> {
        check(unsafe { ffi::compeg_batch_decode(self.raw.as_ptr(), stream.0) })
    }

    /// Records on `stream` the pack of the last decode's images (all of one size) into `[len, 3, h, w]` at
    /// `device_dst`; `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor(&mut self, spec: &TensorSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_pack_tensor(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Records on `stream` the resized pack of the last decode's images, of whatever sizes, into
    /// `[len, 3, resize.height, resize.width]` at `device_dst`; `crops`: `None` for whole images, or one per image.
    /// `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_resized(&mut self, spec: &TensorSpec, resize: &ResizeSpec, crops: Option<&[Rect]>, device_dst: *mut c_void,
                                      dst_bytes: usize, stream: Stream) -> Result<()> {
        if let Some(c) = crops {
            if c.len() != self.len() {
                let message = format!("pack_tensor_resized: {} crops for a batch of {} images", c.len(), self.len());
                return Err(Error { message, code: ffi::COMPEG_E_INVALID_ARG });
            }
        }
        let crops = crops.map_or(ptr::null(), |c| c.as_ptr());
        check(ffi::compeg_batch_pack_tensor_resized(self.raw.as_ptr(), &spec.raw(), &resize.raw(), crops, device_dst, dst_bytes, stream.0))
    }

    /// Records on `stream` the region pack of the last decode: `regions` over its images, any of them any number of
    /// times and in any order, into `[regions.len(), 3, resize.height, resize.width]` at `device_dst`; `pad` as
    /// `Decoder::pack_tensor_regions` has it.  `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_regions(&mut self, spec: &TensorSpec, resize: &ResizeSpec, regions: &[Region], pad: Option<&[f32; 3]>,
                                      device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_region> = regions.iter().map(Region::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_batch_pack_tensor_regions(self.raw.as_ptr(), &spec.raw(), &resize.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                    dst_bytes, stream.0))
    }

    /// Records on `stream` the filtered pack of the last decode: `pack_tensor_regions` with one of the four resampling
    /// kernels of `FilterSpec`.  `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_filtered(&mut self, spec: &TensorSpec, filter: &FilterSpec, regions: &[Region], pad: Option<&[f32; 3]>,
                                       device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_region> = regions.iter().map(Region::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_batch_pack_tensor_filtered(self.raw.as_ptr(), &spec.raw(), &filter.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                     dst_bytes, stream.0))
    }

    /// Records on `stream` the oriented pack of the last decode: `pack_tensor_filtered` with an orientation per region;
    /// `filter`'s extent is the upright slot.  `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_oriented(&mut self, spec: &TensorSpec, filter: &FilterSpec, regions: &[OrientedRegion], pad: Option<&[f32; 3]>,
                                       device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_batch_pack_tensor_oriented(self.raw.as_ptr(), &spec.raw(), &filter.raw(), raw.as_ptr(), raw.len(), pad, device_dst,
                                                     dst_bytes, stream.0))
    }

    /// Records on `stream` the channels-last pack of the last decode: `pack_tensor_oriented` into `[count][oh][ow][C]`.
    /// `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_nhwc(&mut self, spec: &TensorSpec, filter: &FilterSpec, nhwc: &NhwcSpec, regions: &[OrientedRegion],
                                   pad: Option<&[f32; 3]>, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.map_or(ptr::null(), |p| p.as_ptr());
        check(ffi::compeg_batch_pack_tensor_nhwc(self.raw.as_ptr(), &spec.raw(), &filter.raw(), &nhwc.raw(), raw.as_ptr(), raw.len(), pad,
                                                 device_dst, dst_bytes, stream.0))
    }

    /// Records on `stream` the luma pack of the last decode: `pack_tensor_oriented` with one channel a slot,
    /// `[count][1][oh][ow]`.  `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn pack_tensor_luma(&mut self, spec: &TensorSpec, filter: &FilterSpec, luma: &LumaSpec, regions: &[OrientedRegion],
                                   pad: Option<f32>, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        let raw: Vec<ffi::compeg_oriented_region> = regions.iter().map(OrientedRegion::raw).collect();
        let pad = pad.as_ref().map_or(ptr::null(), |p| p as *const f32);
        check(ffi::compeg_batch_pack_tensor_luma(self.raw.as_ptr(), &spec.raw(), &filter.raw(), &luma.raw(), raw.as_ptr(), raw.len(), pad,
                                                 device_dst, dst_bytes, stream.0))
    }

    /// Extension: records a decode of the last upload's images (all of one size and sampling) that writes each one's own
    /// Y, Cb and Cr samples into caller-owned device memory, image i at `i * total_bytes` of `planes_shape`.  The RGBA
    /// outputs are not touched.  Returns without waiting; `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_planes(&mut self, spec: &PlanesSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_decode_planes(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Extension: records a decode of the last upload's images (all of one size and sampling) at 1/8 scale into
    /// caller-owned device memory, image i at `i * total_bytes` of `reduced_shape`.  The RGBA outputs are not touched.
    /// Returns without waiting; `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_reduced(&mut self, spec: &ReducedSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_decode_reduced(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Extension: records a decode of the last upload's images (all of one size and sampling) at the spec's scale (1/2,
    /// 1/4 or 1/8) into caller-owned device memory, image i at `i * total_bytes` of `scaled_shape`.  The RGBA outputs are
    /// not touched.  Returns without waiting; `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_scaled(&mut self, spec: &ScaledSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_decode_scaled(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Extension: records a decode of the spec's rectangle, one for all of the last upload's images (all of one size and
    /// sampling), into caller-owned device memory, image i at `i * total_bytes` of `crop_shape`.  The RGBA outputs are not
    /// touched.  Returns without waiting; `wait` covers it.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes that stays valid until the stream has run.
    pub unsafe fn decode_cropped(&mut self, spec: &CropSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_decode_cropped(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// Records on `stream` a decode of the last upload's images to their quantised DCT coefficients (levels) into
    /// caller-owned device memory, image i at `i * total_bytes` of `levels_shape`.  The RGBA outputs are not touched.
    ///
    /// # Safety
    /// `device_dst` must be device memory of at least `dst_bytes` bytes, at an address that is a multiple of 16, that stays
    /// valid until the stream has run.
    pub unsafe fn decode_levels(&mut self, spec: &LevelsSpec, device_dst: *mut c_void, dst_bytes: usize, stream: Stream) -> Result<()> {
        check(ffi::compeg_batch_decode_levels(self.raw.as_ptr(), &spec.raw(), device_dst, dst_bytes, stream.0))
    }

    /// The 64 quantisation factors, in `order`, of component `component` of image `index` of the last upload.
    pub fn quant_table(&self, index: usize, component: u32, order: LevelsOrder) -> Result<[u16; 64]> {
        let mut q = [0u16; 64];
        check(unsafe { ffi::compeg_batch_quant_table(self.raw.as_ptr(), index, component, q.as_mut_ptr(), order.raw()) })?;
        Ok(q)
    }

    /// The EXIF orientation tag (1..8) of image `index` of the last upload.
    pub fn orientation(&self, index: usize) -> Result<u32> {
        let mut o = 0;
        check(unsafe { ffi::compeg_batch_image_orientation(self.raw.as_ptr(), index, &mut o) })?;
        Ok(o)
    }

    pub fn wait(&mut self) -> Result<()> {
        check(unsafe { ffi::compeg_batch_wait(self.raw.as_ptr()) })
    }

    pub fn len(&self) -> usize {
        unsafe { ffi::compeg_batch_count(self.raw.as_ptr()) }
    }

    pub fn is_empty(&self) -> bool {
        self.len() == 0
    }

    pub fn texture(&self, index: usize) -> Result<Texture<'_>> {
        let (mut p, mut w, mut h, mut pitch) = (ptr::null_mut(), 0, 0, 0);
        check(unsafe { ffi::compeg_batch_output(self.raw.as_ptr(), index, &mut p, &mut w, &mut h, &mut pitch) })?;
        Ok(Texture { device_ptr: p, width: w, height: h, pitch_bytes: pitch, _owner: PhantomData })
    }

    pub fn pixels(&self) -> u64 {
        unsafe { ffi::compeg_batch_pixels(self.raw.as_ptr()) }
    }
}

impl Drop for Batch {
    fn drop(&mut self) {
        unsafe { ffi::compeg_batch_free(self.raw.as_ptr()) }
    }
}
