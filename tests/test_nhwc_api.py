"""The channels-last tensor output where no device is needed (include/compeg_hip.h, "Channels-last tensor output"):
compeg_nhwc_tensor_shape / nhwc_tensor_shape against compeg_oriented_tensor_shape, every rejection the layout adds with
its words, the order in which the pack calls check their arguments, and the helper that turns a destination into
(address, bytes): a channels_last torch tensor on the CPU is accepted as it is, a planar one is an error."""
import ctypes as C

import numpy as np
import pytest

import compeg_amd as ca
import orient_reference as orf
from compeg_amd._lib import NhwcSpec, OrientedRegion, lib
from test_orient_api import F16, _filter, _oriented, _shape, _spec   # (helpers, no tests)

ESIZE = {0: 1, 1: 2, 2: 2, 3: 4}


def _nhwc(channels=3, fill=0.0, reserved=(0, 0)):
    return NhwcSpec(channels, fill, (C.c_uint32 * 2)(*reserved))


def _nhwc_shape(spec, filter, nhwc, w, h, region=None):
    pw, ph, n = C.c_uint32(0xdead), C.c_uint32(0xdead), C.c_size_t(0xdead)
    rc = lib.compeg_nhwc_tensor_shape(C.byref(spec), C.byref(filter), C.byref(nhwc) if nhwc is not None else None, w, h,
                                      C.byref(region) if region is not None else None, C.byref(pw), C.byref(ph), C.byref(n))
    return rc, pw.value, ph.value, n.value


def test_struct_size():
    assert C.sizeof(NhwcSpec) == 16 and C.sizeof(ca.NhwcSpec) == 16
    assert (NhwcSpec.channels.offset, NhwcSpec.fill.offset, NhwcSpec.reserved.offset) == (0, 4, 8)


@pytest.mark.parametrize("channels", (3, 4))
@pytest.mark.parametrize("dtype", (0, 1, 2, 3))
def test_bytes_per_slot_count_the_channels(dtype, channels):
    for o in orf.ORIENTATIONS:
        region = _oriented(o, (101, 3, 64, 60), (2, 4, 20, 6))
        planar = _shape(_spec(dtype), _filter(24, 20), 330, 70, region)
        got = _nhwc_shape(_spec(dtype), _filter(24, 20), _nhwc(channels, 1.0), 330, 70, region)
        assert planar[0] == 0 and got == (0, planar[1], planar[2], 20 * 24 * channels * ESIZE[dtype])
    name = ("u8", "f16", "bf16", "f32")[dtype]
    shape, nbytes, pre = ca.nhwc_tensor_shape(330, 70, (13, 31), channels=channels, dtype=name, orientation="rotate90")
    assert shape == (31, 13, channels) and nbytes == 31 * 13 * channels * ESIZE[dtype] and pre == (70, 330)
    # no region at all: the whole image at orientation 1
    assert _nhwc_shape(_spec(dtype), _filter(13, 31), _nhwc(channels), 330, 70) == (0, 330, 70, 31 * 13 * channels * ESIZE[dtype])


def test_three_channels_ignore_the_fill():
    a = _nhwc_shape(_spec(F16), _filter(), _nhwc(3, 0.0), 330, 70, _oriented(6))
    b = _nhwc_shape(_spec(F16), _filter(), _nhwc(3, -1e30), 330, 70, _oriented(6))
    assert a == b == (0, 330, 70, 20 * 24 * 3 * 2)
    assert ca.nhwc_tensor_shape(330, 70, (24, 20), channels=3, fill=255) == ca.nhwc_tensor_shape(330, 70, (24, 20), channels=3)


@pytest.mark.parametrize("nhwc, words", [
    (None, ("nhwc is NULL",)),
    (_nhwc(0), ("channels 0", "3", "4")),
    (_nhwc(1), ("channels 1",)),
    (_nhwc(2), ("channels 2",)),
    (_nhwc(5), ("channels 5",)),
    (_nhwc(0xffffffff), ("channels 4294967295",)),
    (_nhwc(4, float("nan")), ("fill", "not finite")),
    (_nhwc(4, float("inf")), ("fill", "not finite")),
    (_nhwc(3, float("-inf")), ("fill", "not finite")),
    (_nhwc(4, 0.0, (1, 0)), ("nhwc", "reserved must be 0")),
    (_nhwc(3, 0.0, (0, 7)), ("nhwc", "reserved must be 0")),
], ids=lambda v: None)
def test_what_the_layout_adds_is_rejected_with_a_message(nhwc, words):
    rc, pw, ph, n = _nhwc_shape(_spec(), _filter(), nhwc, 330, 70, _oriented(6))
    assert rc == ca.E_INVALID_ARG and (pw, ph, n) == (0xdead, 0xdead, 0xdead)   # (nothing written on failure)
    message = lib.compeg_last_error().decode()
    assert message and all(w in message for w in words), message
    assert "COMPEG_" not in message


def test_what_the_oriented_shape_rejects_is_rejected_here_with_its_words():
    for spec, filter, region in ((_spec(dtype=4), _filter(), _oriented(6)), (_spec(), _filter(kernel=4), _oriented(6)), (_spec(), _filter(), _oriented(9)),
                                 (_spec(), _filter(), _oriented(6, reserved=1)), (_spec(), _filter(), _oriented(5, dst=(0, 0, 20, 24))),
                                 (_spec(), _filter(), _oriented(6, (101, 3, 200, 64), (2, 4, 20, 6))), (_spec(), _filter(), _oriented(7, src=(1, 0, 330, 70)))):
        want = _shape(spec, filter, 330, 70, region)
        message = lib.compeg_last_error().decode()
        got = _nhwc_shape(spec, filter, _nhwc(4, 1.0), 330, 70, region)
        assert want[0] == ca.E_INVALID_ARG and got == want and lib.compeg_last_error().decode() == message
    # the specs are looked at before the layout, the layout before the region
    assert _nhwc_shape(_spec(dtype=4), _filter(), _nhwc(5), 330, 70, _oriented(9))[0] == ca.E_INVALID_ARG
    assert "dtype 4" in lib.compeg_last_error().decode()
    assert _nhwc_shape(_spec(), _filter(), _nhwc(5), 330, 70, _oriented(9))[0] == ca.E_INVALID_ARG
    assert "channels 5" in lib.compeg_last_error().decode()
    with pytest.raises(ca.Error, match="channels 5"):
        ca.nhwc_tensor_shape(330, 70, (24, 20), channels=5)


@pytest.mark.parametrize("call", ("compeg_decoder_pack_tensor_nhwc", "compeg_batch_pack_tensor_nhwc"))
def test_the_pack_calls_check_their_arguments_before_their_object(call):
    fn = getattr(lib, call)
    one = (OrientedRegion * 1)(_oriented(6))
    pad = (C.c_float * 3)(0, 0, 0)

    def said(spec, filter, nhwc, regions, count, pad_):
        rc = fn(None, C.byref(spec), C.byref(filter), C.byref(nhwc) if nhwc is not None else None, regions, count, pad_, None, 0, None)
        assert rc == ca.E_INVALID_ARG
        return lib.compeg_last_error().decode()
    assert "kernel 9" in said(_spec(), _filter(kernel=9), _nhwc(5), one, 1, pad)
    assert "regions is NULL" in said(_spec(), _filter(), _nhwc(5), None, 1, pad)
    assert "nhwc is NULL" in said(_spec(), _filter(), None, one, 1, pad)
    assert "channels 5" in said(_spec(), _filter(), _nhwc(5), one, 1, pad)
    assert "fill" in said(_spec(), _filter(), _nhwc(4, float("nan")), one, 1, pad)
    assert "reserved" in said(_spec(), _filter(), _nhwc(4, 0.0, (0, 1)), one, 1, pad)
    assert "NULL" in said(_spec(), _filter(), _nhwc(4, 255.0), one, 1, pad)   # (the object, at last)


# ---- the destination ---------------------------------------------------------------------------------------------------

def _range(dst, size=(7, 5), channels=3):
    return ca._nhwc_device_range(dst, size, channels)


def test_an_address_and_a_byte_count_pass_as_they_are():
    assert _range((4096, 123)) == (4096, 123)


def test_tensors_in_either_channels_last_form_are_accepted_as_they_are():
    torch = pytest.importorskip("torch")
    for channels in (3, 4):
        last = torch.empty(2, 5, 7, channels, dtype=torch.float16)
        assert last.is_contiguous() and _range(last, channels=channels) == (last.data_ptr(), 2 * 5 * 7 * channels * 2)
        first = torch.empty(2, channels, 5, 7).contiguous(memory_format=torch.channels_last)
        assert not first.is_contiguous() and first.stride() == (5 * 7 * channels, 1, 7 * channels, channels)
        assert _range(first, channels=channels) == (first.data_ptr(), 2 * 5 * 7 * channels * 4)
    # one slot without a batch axis, more than one axis in front, and axes of 1 (whose strides say nothing)
    one = torch.empty(5, 7, 3, dtype=torch.uint8)
    assert _range(one) == (one.data_ptr(), 105)
    many = torch.empty(2, 3, 5, 7, 3, dtype=torch.uint8)
    assert _range(many) == (many.data_ptr(), 6 * 105)
    single = torch.empty(1, 3, 5, 7).contiguous(memory_format=torch.channels_last)
    assert _range(single) == (single.data_ptr(), 105 * 4)
    column = torch.empty(2, 3, 5, 1).contiguous(memory_format=torch.channels_last)
    assert _range(column, size=(1, 5)) == (column.data_ptr(), 2 * 15 * 4)
    # the permuted view of a contiguous NHWC tensor is the same memory
    nhwc = torch.empty(2, 5, 7, 3)
    assert _range(nhwc.permute(0, 3, 1, 2)) == _range(nhwc)


def test_a_planar_a_sliced_and_a_wrongly_shaped_tensor_are_refused():
    torch = pytest.importorskip("torch")
    with pytest.raises(ca.Error, match="planar"):
        _range(torch.empty(2, 3, 5, 7))
    with pytest.raises(ca.Error, match="densely"):
        _range(torch.empty(2, 5, 7, 4)[..., :3])
    with pytest.raises(ca.Error, match="densely"):
        _range(torch.empty(4, 5, 7, 3)[::2])
    with pytest.raises(ca.Error, match="densely"):
        _range(torch.empty(1, 5, 7, 3).expand(2, 5, 7, 3))
    for wrong in ((2, 5, 7, 4), (2, 6, 7, 3), (2, 5, 8, 3), (2, 7, 5, 3)):
        with pytest.raises(ca.Error, match="neither"):
            _range(torch.empty(*wrong))
    with pytest.raises(ca.Error, match="neither"):   # channels-last strides, four channels where three are packed
        _range(torch.empty(2, 4, 5, 7).contiguous(memory_format=torch.channels_last))
    with pytest.raises(ca.Error, match="neither"):   # a flat buffer says nothing about its layout: (address, nbytes) is for that
        _range(torch.empty(2 * 5 * 7 * 3))
    with pytest.raises(ca.Error, match="neither"):
        _range(object())


class _Cai:
    """An object that has nothing but __cuda_array_interface__ (strides in bytes, or None for row-major)."""

    def __init__(self, shape, typestr, strides=None, address=0x7000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (address, False), "strides": strides, "version": 3}


def test_cuda_array_interface_objects_go_by_their_strides_too():
    assert _range(_Cai((2, 5, 7, 3), "<f2")) == (0x7000, 420)
    assert _range(_Cai((2, 5, 7, 3), "<f2", (210, 42, 6, 2))) == (0x7000, 420)
    assert _range(_Cai((2, 3, 5, 7), "<f4", (420, 4, 84, 12))) == (0x7000, 840)
    with pytest.raises(ca.Error, match="planar"):
        _range(_Cai((2, 3, 5, 7), "<f4"))
    with pytest.raises(ca.Error, match="densely"):
        _range(_Cai((2, 5, 7, 3), "|u1", (210, 42, 6, 2)))
    with pytest.raises(ca.Error, match="element size"):
        _range(_Cai((2, 5, 7, 3), "<f2", (211, 42, 6, 2)))
    # numpy's arrays describe themselves the same way: the reference's own layout passes
    a = np.zeros((5, 7, 3), np.uint8)
    assert _range(_Cai(a.shape, a.dtype.str, a.strides)) == (0x7000, 105)
