"""tests/nhwc_reference.py against what "channels-last" means elsewhere: its bytes are the storage of the planar slot put
through torch's .contiguous(memory_format=torch.channels_last), and for u8 with three channels what numpy sees of a PIL
image.  CPU only; torch is used on the CPU."""
import numpy as np
import pytest

import nhwc_reference as nr

fr = nr.fr
RGBA = fr.frame(50, 26, seed=5)[1]
ARGS = ((3, 1, 45, 21), (1, 3, 11, 13), (10.0, 114.0, 250.5))   # src, dst in the upright (24, 20), pad


def _planar(dtype, o=5, order="rgb"):
    scale, bias = fr.params(dtype)
    return nr.orf.expected(RGBA, (24, 20), 1, dtype, scale, bias, order, "bicubic", *ARGS, o)


@pytest.mark.parametrize("dtype", ["u8", "f16", "f32"])
def test_the_references_bytes_are_the_storage_of_torchs_channels_last(dtype):
    torch = pytest.importorskip("torch")
    planar = _planar(dtype)
    scale, bias = fr.params(dtype)
    want = nr.expected(RGBA, (24, 20), 1, dtype, scale, bias, "rgb", "bicubic", *ARGS, 5)
    assert want.shape == (20, 24, 3) and want.dtype == planar.dtype
    t = torch.from_numpy(planar)[None].contiguous(memory_format=torch.channels_last)
    assert tuple(t.shape) == (1, 3, 20, 24) and t.stride() == (20 * 24 * 3, 1, 24 * 3, 3) and not t.is_contiguous()
    # the storage in memory order: the tensor seen [N, H, W, C] is contiguous, its bytes are the storage's
    storage = t.permute(0, 2, 3, 1)
    assert storage.is_contiguous() and storage.data_ptr() == t.data_ptr()
    assert storage.numpy().tobytes() == want.tobytes()
    # ... and read as NCHW the channels-last tensor is the planar slot
    assert np.array_equal(t[0].numpy(), planar)


def test_three_u8_channels_are_what_numpy_sees_of_a_pil_image():
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    planar = _planar("u8", o=6)
    image = Image.merge("RGB", [Image.fromarray(planar[c]) for c in range(3)])
    want = nr.channels_last(planar)
    assert image.size == (24, 20) and np.array_equal(np.asarray(image), want)
    assert image.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", fr.DTYPES)
def test_four_channels_carry_the_converted_fill_and_leave_the_three_alone(dtype):
    planar = _planar(dtype, o=7, order="bgr")
    four = nr.channels_last(planar, 4, 127.5, dtype)
    assert four.shape == (20, 24, 4) and np.array_equal(four[..., :3], nr.channels_last(planar))
    # 127.5: a tie in u8 (to even: 128), exact in the float types
    want = {"u8": 128, "f16": np.float16(127.5), "bf16": 0x42FF, "f32": np.float32(127.5)}[dtype]
    assert (four[..., 3] == want).all()


def test_the_fill_is_rounded_like_any_value():
    assert nr.fill_element(0.1, "f16") == np.float16(0.1) and nr.fill_element(300.0, "u8") == 255 and nr.fill_element(-3.0, "u8") == 0
    assert nr.fill_element(2.5, "u8") == 2 and nr.fill_element(3.5, "u8") == 4
    # bf16 keeps 8 bits: 1 + 2^-8 is a tie (to even: 1.0), 1 + 3 * 2^-8 one too (up: 1 + 2^-6)
    assert nr.fill_element(1.00390625, "bf16") == 0x3F80 and nr.fill_element(1.01171875, "bf16") == 0x3F82
