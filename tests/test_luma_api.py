"""The luma tensor output where no device is needed (include/compeg_hip.h, "Luma tensor output"):
compeg_luma_tensor_shape / luma_tensor_shape against compeg_oriented_tensor_shape, every rejection the weights add with
its words, the order in which the pack calls check their arguments, and the helper that turns a destination into
(address, bytes): a dense [.., 1, oh, ow], [.., oh, ow, 1] or [.., oh, ow] tensor of as many slots as regions is accepted,
a three-channel tensor, a slice or another extent is an error.  (What needs a decoded frame -- a short or misaligned
destination -- is in tests/test_gpu_luma.py.)"""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import luma_reference as lr
import orient_reference as orf
from compeg_amd._lib import LumaSpec, OrientedRegion, lib
from test_orient_api import F16, _filter, _oriented, _shape, _spec   # (helpers, no tests)

ESIZE = {0: 1, 1: 2, 2: 2, 3: 4}


def _luma(weights=lr.BT601, reserved=0):
    return LumaSpec((C.c_uint32 * 3)(*weights), reserved)


def _luma_shape(spec, filter, luma, w, h, region=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_luma_tensor_shape(C.byref(spec), C.byref(filter), C.byref(luma) if luma is not None else None, w, h,
                                      C.byref(region) if region is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_struct_size_and_offsets():
    assert C.sizeof(LumaSpec) == 16 and C.sizeof(ca.LumaSpec) == 16
    assert (LumaSpec.weights.offset, LumaSpec.weights.size, LumaSpec.reserved.offset) == (0, 12, 12)


def test_the_presets_by_name_are_the_headers():
    assert ca.LUMA_WEIGHTS == lr.PRESETS
    assert all(sum(w) == 65536 and all(0 <= x <= 65536 for x in w) for w in ca.LUMA_WEIGHTS.values())
    spec = ca._luma_spec("bt709")
    assert tuple(spec.weights) == (13933, 46871, 4732) and spec.reserved == 0
    assert tuple(ca._luma_spec((1, 2, 65533)).weights) == (1, 2, 65533)
    for wrong in ("bt2020", (1, 2), (0.5, 0.25, 0.25), (-1, 65536, 1)):
        with pytest.raises(ca.Error, match="luma weights"):
            ca._luma_spec(wrong)


@pytest.mark.parametrize("dtype", (0, 1, 2, 3))
def test_bytes_per_slot_are_a_third_of_the_oriented_shapes(dtype):
    for o in orf.ORIENTATIONS:
        region = _oriented(o, (101, 3, 64, 60), (2, 4, 20, 6))
        planar = _shape(_spec(dtype), _filter(24, 20), 330, 70, region)
        got = _luma_shape(_spec(dtype), _filter(24, 20), _luma(), 330, 70, region)
        assert planar[0] == 0 and planar[3] == 3 * 20 * 24 * ESIZE[dtype]
        assert got == (0, planar[1], planar[2], planar[3] // 3) and got[3] == 20 * 24 * ESIZE[dtype]
    name = ("u8", "f16", "bf16", "f32")[dtype]
    shape, nbytes, pre = ca.luma_tensor_shape(330, 70, (13, 31), dtype=name, orientation="rotate90", weights="bt709")
    assert shape == (1, 31, 13) and nbytes == 31 * 13 * ESIZE[dtype] and pre == (70, 330)
    # no region at all: the whole image at orientation 1
    assert _luma_shape(_spec(dtype), _filter(13, 31), _luma(), 330, 70) == (0, 330, 70, 31 * 13 * ESIZE[dtype])


def test_the_order_has_no_effect_on_the_shape():
    a = _luma_shape(_spec(F16, order=0), _filter(), _luma(), 330, 70, _oriented(6))
    b = _luma_shape(_spec(F16, order=1), _filter(), _luma(lr.BT709), 330, 70, _oriented(6))
    assert a == b == (0, 330, 70, 20 * 24 * 2)


@pytest.mark.parametrize("luma, words", [
    (None, ("luma is NULL",)),
    (_luma((65537, 0, 0)), ("weight 65537", "R", "65536")),
    (_luma((0, 70000, 0)), ("weight 70000", "G")),
    (_luma((0, 0, 0xffffffff)), ("weight 4294967295", "B")),
    (_luma((0, 0, 0)), ("sum 0", "65536")),
    (_luma((19595, 38470, 7470)), ("sum 65535", "65536")),
    (_luma((19595, 38470, 7472)), ("sum 65537",)),
    (_luma((65536, 65536, 65536)), ("sum 196608",)),
    (_luma(lr.BT601, 1), ("luma", "reserved must be 0")),
], ids=lambda v: None)
def test_what_the_weights_add_is_rejected_with_a_message(luma, words):
    rc, pw, ph, n = _luma_shape(_spec(), _filter(), luma, 330, 70, _oriented(6))
    assert rc == ca.E_INVALID_ARG and (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message


def test_what_the_oriented_shape_rejects_is_rejected_here_with_its_words():
    for spec, filter, region in ((_spec(dtype=4), _filter(), _oriented(6)), (_spec(), _filter(kernel=4), _oriented(6)), (_spec(), _filter(), _oriented(9)),
                                 (_spec(order=2), _filter(), _oriented(6)), (_spec(downscale=3), _filter(), _oriented(6)),
                                 (_spec(), _filter(), _oriented(6, reserved=1)), (_spec(), _filter(), _oriented(5, dst=(0, 0, 20, 24))),
                                 (_spec(), _filter(), _oriented(6, (101, 3, 200, 64), (2, 4, 20, 6))), (_spec(), _filter(), _oriented(7, src=(1, 0, 330, 70)))):
        want = _shape(spec, filter, 330, 70, region)
        message = lib.compeg_last_error().decode()
        got = _luma_shape(spec, filter, _luma(), 330, 70, region)
        assert want[0] == ca.E_INVALID_ARG and got == want and lib.compeg_last_error().decode() == message
    # the specs are looked at before the weights, the weights before the region
    assert _luma_shape(_spec(dtype=4), _filter(), _luma((1, 1, 1)), 330, 70, _oriented(9))[0] == ca.E_INVALID_ARG
    assert "dtype 4" in lib.compeg_last_error().decode()
    assert _luma_shape(_spec(), _filter(), _luma((1, 1, 1)), 330, 70, _oriented(9))[0] == ca.E_INVALID_ARG
    assert "sum 3" in lib.compeg_last_error().decode()
    with pytest.raises(ca.Error, match="sum 3"):
        ca.luma_tensor_shape(330, 70, (24, 20), weights=(1, 1, 1))
    # scale and bias beyond element 0 are validated as ever
    bad = _spec()
    bad.scale[2] = float("nan")
    want = _shape(bad, _filter(), 330, 70, _oriented(6))
    message = lib.compeg_last_error().decode()
    assert want[0] == ca.E_INVALID_ARG and _luma_shape(bad, _filter(), _luma(), 330, 70, _oriented(6)) == want
    assert lib.compeg_last_error().decode() == message


@pytest.mark.parametrize("call", ("compeg_decoder_pack_tensor_luma", "compeg_batch_pack_tensor_luma"))
def test_the_pack_calls_check_their_arguments_before_their_object(call):
    fn = getattr(lib, call)
    one = (OrientedRegion * 1)(_oriented(6))
    pad = C.pointer(C.c_float(0.0))   # one float: the calls read no second one

    def said(spec, filter, luma, regions, count, pad_):
        rc = fn(None, C.byref(spec), C.byref(filter), C.byref(luma) if luma is not None else None, regions, count, pad_, None, 0, None)
        assert rc == ca.E_INVALID_ARG
        return lib.compeg_last_error().decode()
    assert "kernel 9" in said(_spec(), _filter(kernel=9), _luma((1, 1, 1)), one, 1, pad)
    assert "regions is NULL" in said(_spec(), _filter(), _luma((1, 1, 1)), None, 1, pad)
    assert "count of 0" in said(_spec(), _filter(), _luma((1, 1, 1)), one, 0, pad)
    for value in (float("nan"), float("inf"), float("-inf")):
        message = said(_spec(), _filter(), _luma(), one, 1, C.pointer(C.c_float(value)))
        assert "pad" in message and "not finite" in message
    assert "luma is NULL" in said(_spec(), _filter(), None, one, 1, pad)
    assert "weight 65537" in said(_spec(), _filter(), _luma((65537, 0, 0)), one, 1, pad)
    assert "sum 3" in said(_spec(), _filter(), _luma((1, 1, 1)), one, 1, pad)
    assert "reserved" in said(_spec(), _filter(), _luma(lr.BT709, 2), one, 1, pad)
    assert "NULL" in said(_spec(), _filter(), _luma(), one, 1, pad)   # (the object, at last)
    assert "NULL" in said(_spec(), _filter(), _luma(), one, 1, None)   # (no pad: 0)


# ---- the destination ---------------------------------------------------------------------------------------------------

def _range(dst, size=(7, 5), count=2):
    return ca._luma_device_range(dst, size, count)


def test_an_address_and_a_byte_count_pass_as_they_are():
    assert _range((4096, 123)) == (4096, 123)


def test_dense_tensors_in_the_three_forms_are_accepted():
    torch = pytest.importorskip("torch")
    for shape in ((2, 1, 5, 7), (2, 5, 7, 1), (2, 5, 7)):
        t = torch.empty(*shape, dtype=torch.float16)
        assert _range(t) == (t.data_ptr(), 2 * 5 * 7 * 2)
    # one slot without a batch axis, more than one axis in front, axes of 1 (whose strides say nothing)
    one = torch.empty(5, 7, dtype=torch.uint8)
    assert _range(one, count=1) == (one.data_ptr(), 35)
    many = torch.empty(2, 3, 1, 5, 7, dtype=torch.uint8)
    assert _range(many, count=6) == (many.data_ptr(), 6 * 35)
    last = torch.empty(2, 1, 5, 7).contiguous(memory_format=torch.channels_last)   # (C = 1: the same memory)
    assert _range(last) == (last.data_ptr(), 2 * 35 * 4)
    column = torch.empty(2, 1, 5, 1)
    assert _range(column, size=(1, 5)) == (column.data_ptr(), 2 * 5 * 4)


def test_a_three_channel_a_sliced_and_a_wrongly_shaped_tensor_are_refused():
    torch = pytest.importorskip("torch")
    with pytest.raises(ca.Error, match="holds 6 slots.*packs 2"):   # [N, 3, oh, ow]: the oriented pack's tensor
        _range(torch.empty(2, 3, 5, 7))
    with pytest.raises(ca.Error, match="none of"):   # ... and the channels-last pack's
        _range(torch.empty(2, 5, 7, 3))
    with pytest.raises(ca.Error, match="densely"):   # one plane sliced out of three
        _range(torch.empty(2, 3, 5, 7)[:, :1])
    with pytest.raises(ca.Error, match="densely"):
        _range(torch.empty(4, 1, 5, 7)[::2])
    with pytest.raises(ca.Error, match="densely"):
        _range(torch.empty(1, 1, 5, 7).expand(2, 1, 5, 7))
    with pytest.raises(ca.Error, match="densely"):   # a transposed view of [.., ow, oh]
        _range(torch.empty(2, 7, 5).transpose(1, 2))
    for wrong in ((2, 1, 6, 7), (2, 1, 5, 8), (2, 1, 7, 5), (2, 5, 7, 2)):
        with pytest.raises(ca.Error, match="none of"):
            _range(torch.empty(*wrong))
    with pytest.raises(ca.Error, match="holds 3 slots"):
        _range(torch.empty(3, 1, 5, 7))
    with pytest.raises(ca.Error, match="none of"):   # a flat buffer says nothing about its layout: (address, nbytes) is for that
        _range(torch.empty(2 * 5 * 7))
    with pytest.raises(ca.Error, match="neither"):
        _range(object())


class _Cai:
    """An object that has nothing but __cuda_array_interface__ (strides in bytes, or None for row-major)."""

    def __init__(self, shape, typestr, strides=None, address=0x7000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (address, False), "strides": strides, "version": 3}


def test_cuda_array_interface_objects_go_by_their_strides_too():
    assert _range(_Cai((2, 1, 5, 7), "<f2")) == (0x7000, 140)
    assert _range(_Cai((2, 5, 7), "<f2", (70, 14, 2))) == (0x7000, 140)
    with pytest.raises(ca.Error, match="holds 6 slots"):
        _range(_Cai((2, 3, 5, 7), "<f4"))
    with pytest.raises(ca.Error, match="densely"):
        _range(_Cai((2, 5, 7), "|u1", (70, 14, 2)))
    with pytest.raises(ca.Error, match="element size"):
        _range(_Cai((2, 5, 7), "<f2", (71, 14, 2)))
    a = np.zeros((5, 7), np.uint8)
    assert _range(_Cai(a.shape, a.dtype.str, a.strides), count=1) == (0x7000, 35)
