"""Expected values of the channels-last tensor output (include/compeg_hip.h, "Channels-last tensor output"), shared by
the CPU and GPU tests: orient_reference's upright slot with the channel axis moved behind the columns, and for four
channels `fill`, put through the reference's own conversion, as element 3 of every pixel.  tests/test_nhwc_reference.py
holds the layout against torch.channels_last and PIL."""
import numpy as np

import orient_reference as orf

fr = orf.fr
store = fr.gr.rr.store   # f32 -> the element type, as every reference converts (bf16: uint16 bit patterns)
CHANNELS = (3, 4)


def fill_element(fill, dtype):
    """`fill` as one stored element: rounded to f32 as the C interface takes it, then converted; neither scale nor bias."""
    return store(np.array([fill], dtype=np.float32), dtype)[0]


def channels_last(planar, channels=3, fill=0.0, dtype=None):
    """[oh, ow, C] from the planar [3, oh, ow]; dtype names the element type when C = 4 needs the fill converted."""
    assert planar.shape[0] == 3 and channels in CHANNELS
    out = np.empty(planar.shape[1:] + (channels,), dtype=planar.dtype)
    out[..., :3] = np.moveaxis(planar, 0, -1)
    if channels == 4:
        out[..., 3] = fill_element(fill, dtype)
    return out


def expected(rgba, size, k, dtype, scale, bias, order="rgb", kernel="bicubic", src=None, dst=None, pad=(0, 0, 0), o=1, channels=3, fill=0.0):
    """One upright slot, [oh, ow, C]: orient_reference.expected moved to channels-last."""
    return channels_last(orf.expected(rgba, size, k, dtype, scale, bias, order, kernel, src, dst, pad, o), channels, fill, dtype)
