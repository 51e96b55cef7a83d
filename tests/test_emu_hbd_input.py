"""CPU: decoder surfaces as device input -- 16-bit samples (H264E_DEV_DEPTH) and 4:4:4 chroma (H264E_DEV_CHROMA_444) -- in the lane-loop
emulation of the kernels (tests/emu), both lane orders.  The emulation's "device" memory is what H264E_dev_malloc hands out; its
global-memory accessors abort on any other address, and every source block here ends with the last byte of the plane's last row, so a
read beyond it would abort the test.

For every case the input slot (H264E_clip_download) holds exactly the model's picture (tests/hbd_model.py), the 4:2:0 16-bit layouts
also exactly what the existing 8-bit device path makes of the quantised planes, and the clip's stream is the stream of that 8-bit picture
through the existing upload.  Every comparison is equality of bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hbd_model as HM
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}
SENTINEL = 0xA5
GOP, QP = 30, 26
SIZES = [(2, 2), (6, 4), (1030, 4), (64, 48)]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


class DevArray:
    """an array in device memory, described the way GPU array libraries do"""

    def __init__(self, ptr, shape, strides, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), strides=tuple(strides), typestr=typestr, data=(ptr, False), version=3)


class DevMem:
    """device memory of one library (H264E_dev_malloc), freed by close()"""

    def __init__(self, lib):
        self.L = pkg.load_pkg().load(lib)
        self.blocks = []

    def block(self, host):
        host = np.ascontiguousarray(host, np.uint8).reshape(-1)
        base = self.L.H264E_dev_malloc(0, host.size)
        assert base
        self.blocks.append(base)
        assert self.L.H264E_dev_memcpy(base, host.ctypes.data, host.size, 1) == 0
        return base

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def put_plane(mem, plane, odd):
    """one 2-D plane in a block of its own that ENDS with the plane's last sample: (pointer, row stride in bytes).  odd: the plane starts
    one sample into the block (2 mod 4 for 16-bit samples, 1 mod 4 for 8-bit -- the allocator's blocks are at least dword aligned) and its
    rows are apart by a number of bytes that is 2 mod 4 (16-bit) or odd (8-bit)"""
    sb = plane.dtype.itemsize
    h, rb = plane.shape[0], plane.shape[1] * sb
    stride, off = rb, 0
    if odd:
        off = sb
        stride = rb + sb
        while stride % 4 != (2 if sb == 2 else 1):
            stride += sb
    host = np.full(off + stride * (h - 1) + rb, SENTINEL, np.uint8)
    raw = np.ascontiguousarray(plane).view(np.uint8).reshape(h, rb)
    for r in range(h):
        host[off + r * stride: off + r * stride + rb] = raw[r]
    base = mem.block(host)
    assert base % 4 == 0
    return base + off, stride


def source(mem, planes, fmt, odd=False, signed=False):
    """the frame (y, u, v) in device memory, as upload_device(..., fmt) takes it"""
    y, u, v = planes
    ts = ("<i2" if signed else "<u2") if y.dtype.itemsize == 2 else "|u1"
    sb = y.dtype.itemsize
    if fmt.startswith("nv12") or fmt in ("p010", "p016"):
        parts = [y, HM.interleave(u, v)]
    elif not odd and not HM.is_444(fmt):             # packed I420: one array
        base = mem.block(np.concatenate([p.reshape(-1) for p in planes]).view(np.uint8))
        h, w = y.shape
        return DevArray(base, (h * 3 // 2, w), (w * sb, sb), ts)
    elif not odd:                                   # 4:4:4: one (3, h, w) array
        h, w = y.shape
        base = mem.block(np.stack(planes).reshape(-1).view(np.uint8))
        return DevArray(base, (3, h, w), (h * w * sb, w * sb, sb), ts)
    else:
        parts = [y, u, v]
    out = []
    for p in parts:
        ptr, stride = put_plane(mem, p, odd)
        out.append(DevArray(ptr, p.shape, (stride, sb), ts))
    return out


def eight_bit_source(mem, planes, fmt):
    """the quantised planes in the existing 8-bit layout of the same family: ("i420" | "nv12", frame)"""
    if fmt.startswith("nv12"):
        return "nv12", [DevArray(put_plane(mem, p, False)[0], p.shape, (p.shape[1], 1), "|u1") for p in (planes[0], HM.interleave(planes[1], planes[2]))]
    return "i420", [DevArray(put_plane(mem, p, False)[0], p.shape, (p.shape[1], 1), "|u1") for p in planes]


def run_clip(lib, w, h, n, put):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, lib=lib, gop=GOP, qp=QP)
    try:
        put(ce)
        slots = ce.download()
        out, sizes, _ = ce.encode()
        return slots, out, sizes
    finally:
        ce.close()


def check(lib, fmt, depth, frames, dw, dh, src_size=None, crop=None, odd=False, signed=False):
    """slots and stream of the frames through the new format against the model and the existing 8-bit paths"""
    n = len(frames)
    kw = dict(depth=depth) if HM.is_16(fmt) else {}
    win = dict(src_size=src_size, crop=crop) if src_size else {}
    model = np.stack([HM.slot(f, fmt, depth, dw, dh, crop) if src_size else HM.slot(f, fmt, depth) for f in frames])
    mem = DevMem(lib)
    try:
        slots, got, sizes = run_clip(lib, dw, dh, n, lambda ce: ce.upload_device([source(mem, f, fmt, odd, signed) for f in frames], fmt, **win, **kw))
        assert np.array_equal(slots, model), "%s depth %s: the slot differs from the model" % (fmt, depth)
        want_slots, want, want_sizes = run_clip(lib, dw, dh, n, lambda ce: ce.upload(model))
        assert np.array_equal(want_slots, model)
        assert got == want and sizes == want_sizes, "%s depth %s: the stream differs from that of the 8-bit picture" % (fmt, depth)
        if fmt in ("i420_16", "nv12_16"):           # ... and the existing 8-bit device path, fed with the quantised planes
            q = [eight_bit_source(mem, HM.eight_bit(f, fmt, depth), fmt) for f in frames]
            slots8, got8, _ = run_clip(lib, dw, dh, n, lambda ce: ce.upload_device([s for _, s in q], q[0][0], **win))
            assert np.array_equal(slots8, slots) and got8 == got, "%s depth %s: differs from the 8-bit device path" % (fmt, depth)
        if fmt == "i444_16":                        # ... = I444 of the quantised planes
            slots8, got8, _ = run_clip(lib, dw, dh, n, lambda ce: ce.upload_device([source(mem, HM.eight_bit(f, fmt, depth), "i444", odd) for f in frames], "i444", **win))
            assert np.array_equal(slots8, slots) and got8 == got
    finally:
        mem.close()


def cases_at_size():
    out = []
    for i, fmt in enumerate(HM.FORMATS):
        for j, (w, h) in enumerate(SIZES):
            for k, d in enumerate((10, 12, 16) if HM.is_16(fmt) else (8,)):
                out.append(pytest.param(fmt, w, h, d, (i + j + k) & 1, id="%s-%dx%d-d%d" % (fmt, w, h, d)))
    return out


@pytest.mark.parametrize("fmt,w,h,depth,flip", cases_at_size())
def test_at_size_slot_and_stream(fmt, w, h, depth, flip):
    """2 x 2: a lone partial group; 6 x 4: a whole and a partial group; 1030 x 4: 258 groups, an odd chroma width; 64 x 48: a picture.
    Half of the cases have plane pointers and strides that are 2 mod 4 (odd for 8-bit 4:4:4); every plane ends with its buffer"""
    frames = [HM.picture(w, h, fmt, depth, t) for t in range(2)]
    check(LIBS["rev" if flip else "fwd"], fmt, depth, frames, w, h, odd=bool(flip), signed=bool(flip) and depth == 16)


@pytest.mark.parametrize("fmt", HM.FORMATS)
@pytest.mark.parametrize("odd", [False, True], ids=["tight", "2mod4"])
def test_addressing(fmt, odd):
    """22 x 6: 5 whole groups and one of two samples in luma, 2 and 3 in chroma, in both addressings for every layout"""
    check(LIBS["fwd"], fmt, 10, [HM.picture(22, 6, fmt, 10, 3)], 22, 6, odd=odd)


@pytest.mark.parametrize("depth", list(HM.DEPTHS))
def test_all_words(depth):
    """every 16-bit word at every depth: luma holds each twice, U the lower half, V the upper"""
    check(LIBS["rev" if depth & 1 else "fwd"], "i420_16", depth, [HM.all_patterns_picture()], 512, 256)


def window_cases():
    out = []
    for i, fmt in enumerate(HM.FORMATS):
        for j, name in enumerate(HM.windows_of(fmt)):
            out.append(pytest.param(fmt, name, (10, 12, 16)[(i + j) % 3], (i + j) & 1, id="%s-%s" % (fmt, name)))
    return out


@pytest.mark.parametrize("fmt,name,depth,flip", window_cases())
def test_window_slot_and_stream(fmt, name, depth, flip):
    (sw, sh), (dw, dh), crop = HM.WINDOWS[name]
    frames = [HM.picture(sw, sh, fmt, depth, t) for t in range(1 if sw > 256 else 2)]
    check(LIBS["rev" if flip else "fwd"], fmt, depth, frames, dw, dh, (sw, sh), crop, odd=bool(flip))
    if name == "pure_crop":                         # ... which is the ingest of the cropped region
        cut = tuple(p[48:, 64:] if HM.is_444(fmt) else (p[48:, 64:] if k == 0 else p[24:, 32:]) for k, p in enumerate(frames[0]))
        assert np.array_equal(HM.slot(frames[0], fmt, depth, dw, dh, crop), HM.slot(cut, fmt, depth))


@pytest.mark.parametrize("fmt", HM.FORMATS + ("p010",))
def test_frame_at_a_time(fmt):
    """H264E_encode_device and H264E_encode_device_scaled, once per layout ("p010": the alias of nv12_16 at depth 16)"""
    depth = 16 if fmt == "p010" else 10
    model_fmt = "nv12_16" if fmt == "p010" else fmt
    P = pkg.load_pkg()
    assert P.dev_format(fmt) == P.dev_format(model_fmt, depth=16) if HM.is_16(fmt) else True
    for (sw, sh), (dw, dh), crop in (((64, 48), (64, 48), None), ((100, 76), (64, 48), (2, 4, 96, 72))):
        frames = [HM.picture(sw, sh, model_fmt, depth, t) for t in range(2)]
        lib = LIBS["fwd"]
        n = len(frames)
        scaled = (sw, sh) != (dw, dh)
        win = dict(src_size=(sw, sh), crop=crop) if scaled else {}
        kw = dict(depth=depth) if HM.is_16(fmt) and fmt != "p010" else {}
        model = np.stack([HM.slot(f, model_fmt, depth, dw, dh, crop) if scaled else HM.slot(f, model_fmt, depth) for f in frames])
        _, want, want_sizes = run_clip(lib, dw, dh, n, lambda ce: ce.upload(model))
        mem = DevMem(lib)
        try:
            e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
            parts = [e.encode_device(source(mem, f, fmt, odd=scaled), fmt, **win, **kw) for f in frames]
            e.close()
            assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes
        finally:
            mem.close()


# ---------------------------------------------------------------- the binding


def test_binding_names_codes_and_types():
    P = pkg.load_pkg()
    assert P.DEV_CHROMA_444 == 0x1000 and P.DEV_FORMAT_I444 == 0x1000 and P.DEV_DEPTH(9) == 0x100 and P.DEV_DEPTH(16) == 0x800
    assert P.DEV_FORMAT_P016 == P.DEV_FORMAT_P010 == 0x801
    assert P.dev_format("i420_16") == 0x800 and P.dev_format("i420_16", depth=10) == 0x200 and P.dev_format("nv12_16", depth=12) == 0x401
    assert P.dev_format("i444") == 0x1000 and P.dev_format("i444_16", depth=10) == 0x1200 and P.dev_format("p010") == P.dev_format("p016") == 0x801
    for fmt, depth in (("i420_16", 8), ("nv12_16", 17), ("p010", 10), ("i420", 10), ("i444", 10)):
        with pytest.raises(P.H264EError, match="depth"):
            P.dev_format(fmt, depth=depth)
    u16 = DevArray(4096, (3, 4, 6), (48, 12, 2), "<u2")
    d, _ = P.dev_frame(u16, "i444_16", 6, 4, depth=10)
    assert d.format == 0x1200 and list(d.plane) == [4096, 4144, 4192] and list(d.stride) == [12, 12, 12]
    d, _ = P.dev_frame(DevArray(4096, (6, 4), (8, 2), "<i2"), "i420_16", 4, 4)
    assert d.format == 0x800 and list(d.plane) == [4096, 4128, 4136] and list(d.stride) == [8, 4, 4]
    d, _ = P.dev_frame([DevArray(4096, (4, 4), (10, 2), "<u2"), DevArray(8192, (2, 4), (8, 2), "<u2")], "p010", 4, 4)
    assert d.format == 0x801 and list(d.plane)[:2] == [4096, 8192] and list(d.stride)[:2] == [10, 8]
    d, _ = P.dev_frame([(4096, 10), (8192, 6), (8200, 6)], "i420_16", 4, 4, depth=12)
    assert d.format == 0x400 and list(d.stride) == [10, 6, 6]
    u8 = DevArray(4096, (3, 4, 6), (24, 6, 1), "|u1")
    for name in HM.FORMATS_16:                      # 8-bit arrays for a 16-bit name, with the type named
        with pytest.raises(P.H264EError, match=r"%r takes 16-bit samples.*not \|u1" % name):
            P.dev_frame(u8 if name == "i444_16" else [u8, u8] if name == "nv12_16" else [u8] * 3, name, 6, 4)
    with pytest.raises(P.H264EError, match="8-bit samples, not <u2"):               # ... and the reverse
        P.dev_frame(u16, "i444", 6, 4)
    with pytest.raises(P.H264EError, match="device input must be 8-bit samples, not <u2"):      # today's refusal keeps its text
        P.dev_frame(DevArray(4096, (6, 4), (8, 2), "<u2"), "i420", 4, 4)
    with pytest.raises(P.H264EError, match="last axis is contiguous"):
        P.dev_frame(DevArray(4096, (3, 4, 6), (2, 72, 12), "<u2"), "i444_16", 6, 4)
    with pytest.raises(P.H264EError, match=r"contiguous \(6, 4\) array"):
        P.dev_frame(DevArray(4096, (6, 4), (10, 2), "<u2"), "i420_16", 4, 4)


# ---------------------------------------------------------------- refusals


def test_refusals_name_the_value_launch_nothing_and_leave_the_encoders_usable():
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), n = (128, 96), (64, 48), 2
    lib = pkg.EMU_LIB
    fmt, depth = "i420_16", 10
    small = [HM.picture(dw, dh, fmt, depth, t) for t in range(n)]
    big = [HM.picture(sw, sh, fmt, depth, t) for t in range(n)]
    want_plain = run_clip(lib, dw, dh, n, lambda ce: ce.upload(np.stack([HM.slot(f, fmt, depth) for f in small])))[1]
    want_scaled = run_clip(lib, dw, dh, n, lambda ce: ce.upload(np.stack([HM.slot(f, fmt, depth, dw, dh) for f in big])))[1]
    mem = DevMem(lib)
    ce = P.ClipEncoder(dw, dh, n, gop=GOP, qp=QP, lib=lib)
    try:
        marker = np.arange(n * dw * dh * 3 // 2, dtype=np.uint32).astype(np.uint8).reshape(n, -1)
        ce.upload(marker)                           # what the slots hold while calls are refused; a picture for the way out to refuse
        ce.encode()
        py, pu, pv = [put_plane(mem, p, False) for p in small[0]]
        qy, qu, qv = [put_plane(mem, p, False) for p in big[0]]
        huge = put_plane(mem, np.zeros((dh * 9, dw * 9), np.uint8), False)          # enough for a 4:4:4 window beyond 8:1
        whole = dict(src_size=(sw, sh))
        I420, NV12, RGB, RGBP, D10, C444 = P.DEV_FORMAT_I420, P.DEV_FORMAT_NV12, P.DEV_FORMAT_RGB, P.DEV_FORMAT_RGBP, P.DEV_DEPTH(10), P.DEV_CHROMA_444
        cases = [
            # (planes, format, window, what the message holds)
            ([py, pu, pv], 0x2000, {}, "unknown format 8192"),                      # a bit outside 0x1f33
            ([py, pu, pv], I420 | D10 | 0x4, {}, "unknown format 516"),
            ([py, pu, pv], I420 | D10 | 0x40, {}, "unknown format 576"),
            ([qy, qu, qv], 0x2000 | D10, whole, "unknown format 8704"),
            ([py, pu, pv], I420 | 0x900, {}, "unknown format 2304"),                # 9 .. 15 in bits 8-11
            ([py, pu, pv], NV12 | 0xf00, {}, "unknown format 3841"),
            ([qy, qu, qv], I420 | 0xc00, whole, "unknown format 3072"),
            ([py, pu, pv], RGB | D10, {}, r"format 514 asks for 16-bit samples of RGB \(format 2\)"),
            ([py, pu, pv], RGBP | D10, {}, r"format 515 asks for 16-bit samples of RGBP \(format 3\)"),
            ([py, pu, pv], RGB | C444, {}, r"format 4098 asks for 4:4:4 chroma of RGB \(format 2\)"),
            ([py, pu, pv], RGBP | C444, {}, r"format 4099 asks for 4:4:4 chroma of RGBP \(format 3\)"),
            ([qy, qu, qv], RGBP | C444 | D10, whole, r"format 4611 asks for 16-bit samples of RGBP \(format 3\)"),
            ([py, pu, pv], NV12 | C444, {}, r"format 4097 asks for 4:4:4 chroma \(0x1000\) of NV12 \(format 1\)"),
            ([qy, qu, qv], NV12 | C444 | D10, whole, r"format 4609 asks for 4:4:4 chroma \(0x1000\) of NV12 \(format 1\)"),
            ([py, pu, pv], I420 | D10 | P.DEV_SAMPLE_F16, {}, r"format 528 asks for both 10-bit integer samples \(0x200\) and f16 samples \(0x10\) of I420 \(format 0\)"),
            ([py, pu, pv], RGBP | P.DEV_DEPTH(16) | P.DEV_SAMPLE_F32, {}, r"format 2099 asks for both 16-bit integer samples \(0x800\) and f32 samples \(0x30\) of RGBP \(format 3\)"),
            ([qy, qu, qv], NV12 | D10 | P.DEV_SAMPLE_BF16, whole, r"format 545 asks for both 10-bit integer samples \(0x200\) and bf16 samples \(0x20\) of NV12"),
            ([py, (pu[0] + 1, pu[1]), pv], I420 | D10, {}, r"plane 1 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes of a u16 sample"),
            ([py, pu, (pv[0], pv[1] + 1)], I420 | D10, {}, "stride %d of plane 2 is not a multiple of the 2 bytes of a u16 sample" % (pv[1] + 1)),
            ([(py[0] + 1, py[1]), pu, pv], NV12 | P.DEV_DEPTH(16), {}, r"plane 0 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes of a u16 sample"),
            ([qy, (qu[0], qu[1] + 3), qv], I420 | C444 | D10, whole, "stride %d of plane 1 is not a multiple of the 2 bytes of a u16 sample" % (qu[1] + 3)),
            ([qy, qu, (qv[0] + 1, qv[1])], I420 | D10, whole, r"plane 2 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes"),
            ([(py[0], 2 * dw - 2), pu, pv], I420 | D10, {}, "stride 126 of plane 0 is below its 128 row bytes"),
            ([py, (pu[0], dw - 2), pv], I420 | D10, {}, "stride 62 of plane 1 is below its 64 row bytes"),
            ([py, (pu[0], 2 * dw - 2), pv], NV12 | D10, {}, "stride 126 of plane 1 is below its 128 row bytes"),
            ([py, py, (py[0], 2 * dw - 2)], I420 | C444 | D10, {}, "stride 126 of plane 2 is below its 128 row bytes"),
            ([py, (py[0], dw - 1), py], I420 | C444, {}, "stride 63 of plane 1 is below its 64 row bytes"),
            ([qy, (qu[0], sw - 2), qv], I420 | D10, whole, "stride 126 of plane 1 is below the 128 bytes of a source row"),
            ([qy, (qu[0], 2 * sw - 2), qv], NV12 | D10, whole, "stride 254 of plane 1 is below the 256 bytes of a source row"),
            ([qy, qy, (qy[0], 2 * sw - 2)], I420 | C444 | D10, whole, "stride 254 of plane 2 is below the 256 bytes of a source row"),
            # a 4:4:4 window beyond 8 times the picture (its chroma would go beyond 16:1); 4:2:0 takes the same window
            ([huge, huge, huge], I420 | C444, dict(src_size=(dw * 9, dh * 8), crop=(0, 0, dw * 8 + 2, dh * 8)),
             "4:4:4 window width 514 is more than 8 times the picture's 64 .*at most 16 to 1"),
            ([huge, huge, huge], I420 | C444, dict(src_size=(dw * 8, dh * 9), crop=(0, 0, dw * 8, dh * 8 + 2)),
             "4:4:4 window height 386 is more than 8 times the picture's 48 .*at most 16 to 1"),
        ]
        for planes, code, kw, msg in cases:
            d = P.DevFrame(format=code, pixel_bytes=3)
            for k, (ptr, stride) in enumerate(planes):
                d.plane[k], d.stride[k] = ptr, stride
            win = P.dev_window(kw.get("src_size"), kw.get("crop"), dw, dh)[0]
            e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
            data, size = C.c_void_p(), C.c_int()
            if win is not None:
                assert ce.L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(win)) != 0
                text = ce.L.H264E_last_error().decode()
                assert e.L.H264E_encode_device_scaled(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(win), C.byref(data), C.byref(size)) != 0
            else:
                assert ce.L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) != 0
                text = ce.L.H264E_last_error().decode()
                assert e.L.H264E_encode_device(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(data), C.byref(size)) != 0
            assert re.search(msg, text), (msg, text)
            assert re.search(msg, e.L.H264E_last_error().decode()), (msg, e.L.H264E_last_error().decode())
            assert np.array_equal(ce.download(), marker), "a refused call wrote the slot: " + msg       # nothing was launched
            e.close()
        # the 4:2:0 layouts take the 16:1 window that 4:4:4 refuses
        d = P.DevFrame(format=I420, pixel_bytes=0)
        for k in range(3):
            d.plane[k], d.stride[k] = huge
        win = P.dev_window((dw * 9, dh * 9), (0, 0, dw * 8 + 2, dh * 8 + 2), dw, dh)[0]
        assert ce.L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(win)) == 0
        # the way out accepts none of the new bits: its refusal is the one it had
        out = mem.block(np.full(4 * dw * dh * 3, SENTINEL, np.uint8))
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
        e.encode(marker[0])
        for code in (I420 | D10, NV12 | P.DEV_DEPTH(16), I420 | C444, I420 | C444 | D10, P.DEV_FORMAT_P010, 0x100, 0x1000):
            d = P.DevFrame(format=code, pixel_bytes=0)
            for k in range(3):
                d.plane[k], d.stride[k] = out + k * 4 * dw * dh, 2 * dw
            assert ce.L.H264E_clip_read_recon_device(ce.c, 0, C.byref(d)) != 0
            assert ce.L.H264E_last_error().decode().endswith("egress: unknown format %d" % code)
            assert e.L.H264E_read_recon_device(e.persist, C.byref(d)) != 0
            assert e.L.H264E_last_error().decode().endswith("egress: unknown format %d" % code)
        e.close()
        host = np.empty(4 * dw * dh * 3, np.uint8)
        assert ce.L.H264E_dev_memcpy(host.ctypes.data, out, host.size, 0) == 0 and (host == SENTINEL).all()
        for name in ("i444", "i420_16", "p010"):
            with pytest.raises(P.H264EError, match="unknown format"):
                ce.read_recon_device(0, name, out=[(out, 2 * dw)] * (2 if name == "p010" else 3))
        # ... and the streams continue: the next frames are taken, from both encoders, at size and through a window
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
        ce.upload_device([source(mem, f, fmt, True) for f in small], fmt, depth=depth)
        assert ce.encode()[0] == want_plain
        assert b"".join(e.encode_device(source(mem, f, fmt), fmt, depth=depth) for f in small) == want_plain
        e.close()
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
        ce.upload_device([source(mem, f, fmt, True) for f in big], fmt, depth=depth, **whole)
        assert ce.encode()[0] == want_scaled
        assert b"".join(e.encode_device(source(mem, f, fmt), fmt, depth=depth, **whole) for f in big) == want_scaled
        e.close()
    finally:
        ce.close()
        mem.close()
