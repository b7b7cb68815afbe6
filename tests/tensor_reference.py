"""Expected values of the tensor output (include/compeg_hip.h, "Tensor output"), shared by the CPU and GPU tests:
the oracle's RGBA put through the header's formula in numpy, operation by operation in float32."""
import functools

import numpy as np

from oracle import oracle as orc
from tools import synth

DTYPES = ("u8", "f16", "bf16", "f32")
ELEM_BYTES = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4}
# what a model's input transform does to a channel x in 0..255: (x / 255 - mean) / std, as one scale and one bias
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMAGENET_SCALE = tuple(float(np.float32(1.0 / (255.0 * s))) for s in _STD)
IMAGENET_BIAS = tuple(float(np.float32(-m / s)) for m, s in zip(_MEAN, _STD))
IDENTITY = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
# u8 with something to round and to clamp on both sides
U8_SCALE, U8_BIAS = (1.7, 0.5, 1.003), (-40.5, 0.5, 2.25)


def ks_for(w, h):
    return [k for k in (1, 2, 4, 8) if w >= k and h >= k]


@functools.lru_cache(maxsize=None)
def frame(w, h, seed=3, sampling=(2, 1), ri=4):
    """(jpeg bytes, the oracle's RGBA) of one synthetic frame; computed once per process."""
    jpeg = synth.make_jpeg(w, h, seed=seed, quality=85, sampling=sampling, ri=ri)
    rgba = orc.ImageData(jpeg, allow_sampling=sampling != (2, 1)).decode()
    assert rgba.shape == (h, w, 4)
    rgba.setflags(write=False)
    return jpeg, rgba


def expected(rgba, k, dtype, scale, bias, order="rgb"):
    """[3, oh, ow] as the header defines it.  bf16 comes back as its uint16 bit patterns."""
    h, w = rgba.shape[:2]
    oh, ow = h // k, w // k
    planes = []
    for c in range(3):
        ch = rgba[:oh * k, :ow * k, c if order == "rgb" else 2 - c].astype(np.uint32)
        s = ch.reshape(oh, k, ow, k).sum(axis=(1, 3), dtype=np.uint32)
        m = s.astype(np.float32) * np.float32(1.0 / (k * k))
        v = m * np.float32(scale[c])
        v = v + np.float32(bias[c])
        assert v.dtype == np.float32
        planes.append(v)
    v = np.stack(planes)
    if dtype == "f32":
        return v
    if dtype == "f16":
        return v.astype(np.float16)
    if dtype == "bf16":
        u = v.view(np.uint32)
        return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.rint(v).clip(0, 255).astype(np.uint8)


def from_bytes(raw, dtype, shape):
    """The destination's bytes as an array comparable with expected()."""
    np_type = {"u8": np.uint8, "f16": np.float16, "bf16": np.uint16, "f32": np.float32}[dtype]
    return np.frombuffer(raw, dtype=np_type).reshape(shape)


def same(got, want, dtype):
    """Values, not the bit patterns of +-0 (the library is built -fno-signed-zeros)."""
    if dtype == "bf16":
        got = (got.astype(np.uint32) << np.uint32(16)).view(np.float32)
        want = (want.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return got.shape == want.shape and np.array_equal(got, want)
