"""The tensor-output entry points that need no device (include/compeg_hip.h, "Tensor output"): compeg_tensor_shape
and the rejections it shares with the pack calls, through the C ABI and through the Python mirror."""
import ctypes as C
import math

import pytest

import compeg_amd as ca
from compeg_amd._lib import TensorSpec, lib

U8, F16, BF16, F32 = 0, 1, 2, 3


def _spec(dtype=F16, order=0, downscale=1, reserved=0, scale=(1, 1, 1), bias=(0, 0, 0)):
    s = TensorSpec()
    s.dtype, s.order, s.downscale, s.reserved = dtype, order, downscale, reserved
    s.scale[:] = scale
    s.bias[:] = bias
    return s


def _shape(spec, w, h):
    ow, oh, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_tensor_shape(C.byref(spec) if spec is not None else None, w, h, C.byref(ow), C.byref(oh), C.byref(n))
    return rc, ow.value, oh.value, n.value


def test_shape_and_byte_count():
    assert _shape(_spec(F16, downscale=2), 50, 26) == (0, 25, 13, 1950)
    assert _shape(_spec(U8, downscale=8), 16, 8) == (0, 2, 1, 6)
    assert _shape(_spec(BF16, downscale=4), 330, 70) == (0, 82, 17, 3 * 82 * 17 * 2)
    assert _shape(_spec(F32, order=1), 7, 5) == (0, 7, 5, 420)


def test_byte_count_does_not_wrap_at_32_bits():
    rc, ow, oh, n = _shape(_spec(F32), 65528, 65528)
    assert (rc, ow, oh) == (0, 65528, 65528)
    assert n == 3 * 65528 ** 2 * 4 and n > 2 ** 32


def test_outputs_are_optional():
    assert lib.compeg_tensor_shape(C.byref(_spec()), 16, 8, None, None, None) == 0


@pytest.mark.parametrize("spec, w, h, words", [
    (None, 16, 8, "NULL"),
    (_spec(dtype=4), 16, 8, "dtype 4"),
    (_spec(dtype=7), 16, 8, "dtype 7"),
    (_spec(order=2), 16, 8, "order 2"),
    (_spec(downscale=0), 16, 8, "downscale 0"),
    (_spec(downscale=3), 16, 8, "downscale 3"),
    (_spec(downscale=16), 64, 64, "downscale 16"),
    (_spec(reserved=1), 16, 8, "reserved"),
    (_spec(scale=(1, math.inf, 1)), 16, 8, "plane 1"),
    (_spec(scale=(math.nan, 1, 1)), 16, 8, "plane 0"),
    (_spec(bias=(0, 0, -math.inf)), 16, 8, "plane 2"),
    (_spec(downscale=8), 7, 5, "7x5"),
    (_spec(downscale=8), 16, 7, "16x7"),
    (_spec(downscale=2), 1, 9, "1x9"),
    (_spec(), 0, 9, "0x9"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_rejections_carry_a_message(spec, w, h, words):
    rc, ow, oh, n = _shape(spec, w, h)
    assert rc == ca.E_INVALID_ARG
    assert (ow, oh, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and words in message, message
    assert "COMPEG_" not in message   # (values, not macro names: test_shipped_library_has_no_laboratory_switches)


def test_pack_calls_reject_null_handles_and_specs():
    spec = _spec()
    for fn in (lib.compeg_decoder_pack_tensor, lib.compeg_batch_pack_tensor):
        assert fn(None, C.byref(spec), C.c_void_p(256), 1 << 20, None) == ca.E_INVALID_ARG
        assert lib.compeg_last_error().decode()


def test_python_mirror():
    assert ca.tensor_shape(50, 26, dtype="f16", downscale=2) == ((3, 13, 25), 1950)
    assert ca.tensor_shape(16, 8, dtype="u8", downscale=8) == ((3, 1, 2), 6)
    assert ca.tensor_shape(3840, 2160) == ((3, 2160, 3840), 3 * 2160 * 3840 * 2)
    for args in ((7, 5, "u8", 8), (16, 8, "f64", 1), (16, 8, "f16", 5)):
        with pytest.raises(ca.Error) as e:
            ca.tensor_shape(*args)
        assert e.value.code == ca.E_INVALID_ARG and str(e.value)
    assert hasattr(ca.Decoder, "pack_tensor") and hasattr(ca.Batch, "pack_tensor")


def test_destination_forms_need_no_framework():
    """(address, nbytes); data_ptr / numel / element_size; __cuda_array_interface__ -- and the wrapper imports no torch."""
    import subprocess
    import sys
    code = ("import sys, compeg_amd as ca\n"
            "class T:\n"
            "    def data_ptr(self): return 4096\n"
            "    def numel(self): return 30\n"
            "    def element_size(self): return 2\n"
            "class A:\n"
            "    __cuda_array_interface__ = {'shape': (2, 3, 5), 'typestr': '<f4', 'data': (8192, False), 'version': 3}\n"
            "class S:\n"
            "    __cuda_array_interface__ = {'shape': (2, 3), 'typestr': '|u1', 'data': (8192, False), 'strides': (4, 1), 'version': 3}\n"
            "assert ca._device_range((123, 45)) == (123, 45)\n"
            "assert ca._device_range(T()) == (4096, 60)\n"
            "assert ca._device_range(A()) == (8192, 120)\n"
            "try:\n"
            "    ca._device_range(S())\n"
            "    raise SystemExit('a strided destination was accepted')\n"
            "except ca.Error:\n"
            "    pass\n"
            "assert 'torch' not in sys.modules\n")
    from conftest import ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
