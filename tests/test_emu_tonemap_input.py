"""CPU: HDR10 device input (H264E_set_tonemap, enc_tonemap.h) in the lane-loop emulation of the kernels (tests/emu), both lane orders.  The
emulation's "device" memory is what H264E_dev_malloc hands out; its global-memory accessors abort on any other address, and with the
"separate" and "padded" addressings every source block ends with the last sample of the plane's last row, so a read beyond it would
abort the test.  The cases are tests/tonemap_cases.py's, the ones the GPU runs."""
import os
import subprocess

import numpy as np
import pytest

import pkg
import tonemap_cases as TC
import tonemap_model as TM

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


class DevArray:
    """an array in device memory, described the way GPU array libraries do"""

    def __init__(self, ptr, shape, strides, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), strides=tuple(strides), typestr=typestr, data=(ptr, False), version=3)


class Emu:
    """the backend of tests/tonemap_cases.py over one emulation library; close() frees what it allocated"""

    def __init__(self, lib):
        self.lib = lib
        self.L = pkg.load_pkg().load(lib)
        self.blocks = []

    def block(self, host):
        host = np.ascontiguousarray(host).view(np.uint8).reshape(-1)
        base = self.L.H264E_dev_malloc(0, host.size)
        assert base and base % 4 == 0
        self.blocks.append(base)
        assert self.L.H264E_dev_memcpy(base, host.ctypes.data, host.size, 1) == 0
        return base

    @staticmethod
    def typestr(a, signed):
        return "|u1" if a.dtype.itemsize == 1 else "<i2" if signed else "<u2"

    def array(self, a):
        a = np.ascontiguousarray(a)
        return DevArray(self.block(a), a.shape, a.strides, self.typestr(a, False))

    def plane(self, a, off, stride, signed):
        """the plane in a block of its own, `off` bytes in, rows `stride` bytes apart: the block ENDS with the plane's last sample"""
        sb, (h, w) = a.dtype.itemsize, a.shape
        host = np.full(off + stride * (h - 1) + w * sb, SENTINEL, np.uint8)
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(h, w * sb)
        for r in range(h):
            host[off + r * stride: off + r * stride + w * sb] = raw[r]
        return DevArray(self.block(host) + off, a.shape, (stride, sb), self.typestr(a, signed))

    def planes(self, planes, kind, signed=False):
        out = []
        for a in planes:
            sb, w = a.dtype.itemsize, a.shape[1]
            if kind in ("tight", "separate"):       # (every block here is an allocation of its own)
                out.append(self.plane(a, 0, w * sb, signed))
            elif kind == "padded":                  # one word in, rows an odd number of words apart: addresses 2 mod 4
                out.append(self.plane(a, sb, (w + 1 + (w & 1)) * sb, signed))
            else:                                   # a view of a wider array: a whole number of dwords apart, three words in
                out.append(self.plane(a, 3 * sb, (w + 6 + (w & 1)) * sb, signed))
        return out

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


@pytest.fixture(params=["fwd", "rev"])
def both(request):
    b = Emu({"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}[request.param])
    yield b
    b.close()


@pytest.fixture
def B():
    b = Emu(pkg.EMU_LIB)
    yield b
    b.close()


@pytest.mark.parametrize("fmt,depth,w,h,kind,color,curve,signed", TC.at_size_cases())
def test_at_size_slot_and_stream(fmt, depth, w, h, kind, color, curve, signed):
    b = Emu(pkg.EMU_REV_LIB if (w + depth) & 2 else pkg.EMU_LIB)
    try:
        TC.case_at_size(b, fmt, depth, w, h, kind, color, curve, signed)
    finally:
        b.close()


@pytest.mark.parametrize("curve", TM.CURVES)
def test_all_codes(both, curve):
    TC.case_all_codes(both, curve)


@pytest.mark.parametrize("name,fmt,depth,kind,color,curve", [
    ("2to1", "p010", 16, "tight", "bt709", "hable"), ("2to1", "i420_16", 10, "padded", None, "clip"),
    ("crop", "nv12_16", 10, "separate", None, "reinhard"), ("crop", "i420_16", 12, "view", "bt709", "hable"),
    ("pure_crop", "i420_16", 10, "tight", "bt709", "hable"), ("pure_crop", "p010", 16, "padded", None, "reinhard")])
def test_window_slot_and_stream(B, name, fmt, depth, kind, color, curve):
    TC.case_window(B, name, fmt, depth, kind, color, curve)


@pytest.mark.parametrize("fmt,depth", [("p010", 16), ("i420_16", 10)])
def test_frame_at_a_time(B, fmt, depth):
    TC.case_frame_at_a_time(B, fmt, depth)


def test_ladder_from_a_p010_source(B):
    TC.case_ladder(B)


def test_off_means_off(both):
    TC.case_off_means_off(both)


def test_refusals_name_the_value_move_nothing_and_leave_the_encoders_usable(B):
    TC.case_refusals(B)


def test_binding_option():
    P = pkg.load_pkg()
    assert (P.TONEMAP_OFF, P.TONEMAP_PQ, P.TONECURVE_HABLE, P.TONECURVE_REINHARD, P.TONECURVE_CLIP) == (0, 1, 0, 1, 2)
    assert P.tonemap_args("pq") == (1, 0, 0.0, 0.0) and P.tonemap_args(None) == (0, 0, 0.0, 0.0) and P.tonemap_args("off") == (0, 0, 0.0, 0.0)
    assert P.tonemap_args({"transfer": "pq", "curve": "reinhard", "peak": 4000, "ref_white": 100}) == (1, 1, 4000.0, 100.0)
    assert P.tonemap_args({"curve": "clip"}) == (1, 2, 0.0, 0.0)
    for bad in ("hlg", {"curve": "aces"}, {"peak": "bright"}, {"nits": 1}, 3):
        with pytest.raises(P.H264EError, match="tonemap"):
            P.tonemap_args(bad)
    assert P.load(pkg.EMU_LIB).H264E_struct_size(3) == -1
