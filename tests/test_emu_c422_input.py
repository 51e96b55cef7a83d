"""CPU: 4:2:2 device input -- I422, NV16 and packed YUYV / UYVY, 8-bit samples or 16-bit words (H264E_DEV_CHROMA_422, H264E_DEV_PACK_*) --
in the lane-loop emulation of the kernels of enc_422.h (tests/emu), both lane orders.  The emulation's "device" memory is what
H264E_dev_malloc hands out; its global-memory accessors abort on any other address, and every source block here ends with the last byte
of the plane's last row, so a read beyond it would abort the test.

For every case the input slot (H264E_clip_download) holds exactly the model's picture (tests/c422_model.py) and the clip's stream is the
stream of that 8-bit picture through the existing upload.  Every comparison is equality of bytes."""
import ctypes as C
import re

import numpy as np
import pytest

import c422_model as CM
import pkg
from test_emu_hbd_input import GOP, LIBS, QP, SENTINEL, DevArray, DevMem, _emu, put_plane, run_clip  # noqa: F401  (_emu builds the emulation)

SIZES = [(2, 2), (6, 4), (1030, 4), (64, 48)]
ALIASES_16 = ("p210", "p216", "y210", "y216")


def source(mem, planes, fmt, odd=False, signed=False):
    """the 4:2:2 frame (y, u, v) in device memory, as upload_device(..., fmt) takes it.  odd: a strided view per array (8-bit: odd
    pointers and strides; 16-bit: 2 mod 4); else ONE array -- ffmpeg's buffer for "i422", luma rows then U,V rows for "nv16", (h, w, 2) for
    the packed orders.  Every block ends with its last sample"""
    y = planes[0]
    sb = y.dtype.itemsize
    ts = ("<i2" if signed else "<u2") if sb == 2 else "|u1"
    arrays = CM.layout(planes, fmt)
    h, w = y.shape
    if odd:
        out = []
        for p in arrays:
            ptr, stride = put_plane(mem, p, True)
            out.append(DevArray(ptr, p.shape, (stride, sb), ts))
        return out if len(out) > 1 else out[0]
    base = mem.block(np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in arrays]).view(np.uint8))
    if len(arrays) == 1:
        return DevArray(base, (h, w, 2), (2 * w * sb, 2 * sb, sb), ts)
    return DevArray(base, (2 * h, w), (w * sb, sb), ts)


def check(lib, fmt, depth, frames, dw, dh, src_size=None, crop=None, odd=False, signed=False):
    """slots and stream of the frames through the 4:2:2 format against the model and the existing upload of the model's picture"""
    n = len(frames)
    kw = dict(depth=depth) if CM.is_16(fmt) and fmt not in ALIASES_16 else {}
    win = dict(src_size=src_size, crop=crop) if src_size else {}
    model = np.stack([CM.slot(f, fmt, depth, dw, dh, crop) if src_size else CM.slot(f, fmt, depth) for f in frames])
    mem = DevMem(lib)
    try:
        slots, got, sizes = run_clip(lib, dw, dh, n, lambda ce: ce.upload_device([source(mem, f, fmt, odd, signed) for f in frames], fmt, **win, **kw))
        assert np.array_equal(slots, model), "%s depth %s: the slot differs from the model" % (fmt, depth)
        want_slots, want, want_sizes = run_clip(lib, dw, dh, n, lambda ce: ce.upload(model))
        assert np.array_equal(want_slots, model)
        assert got == want and sizes == want_sizes, "%s depth %s: the stream differs from that of the 8-bit picture" % (fmt, depth)
    finally:
        mem.close()
    return slots


def cases_at_size():
    out = []
    for i, fmt in enumerate(CM.FORMATS):
        for j, (w, h) in enumerate(SIZES):
            for k, d in enumerate((10, 12, 16) if CM.is_16(fmt) else (8,)):
                out.append(pytest.param(fmt, w, h, d, (i + j + k) & 1, id="%s-%dx%d-d%d" % (fmt, w, h, d)))
    return out


@pytest.mark.parametrize("fmt,w,h,depth,flip", cases_at_size())
def test_at_size_slot_and_stream(fmt, w, h, depth, flip):
    """2 x 2: a lone partial group, one chroma row from two; 6 x 4: a whole and a partial group; 1030 x 4: 258 groups, an odd chroma
    width; 64 x 48: a picture.  Half of the cases have pointers and strides that are odd (8-bit) or 2 mod 4 (16-bit) and run the lanes in
    reverse; every array ends with its buffer"""
    frames = [CM.picture(w, h, fmt, depth, t) for t in range(2)]
    check(LIBS["rev" if flip else "fwd"], fmt, depth, frames, w, h, odd=bool(flip), signed=bool(flip) and depth == 16)


@pytest.mark.parametrize("fmt", CM.FORMATS)
@pytest.mark.parametrize("odd", [False, True], ids=["tight", "odd"])
def test_addressing(fmt, odd):
    """22 x 6: 5 whole groups and one of two samples in luma, 2 and 3 in chroma, in both addressings for every layout"""
    check(LIBS["fwd"], fmt, 10, [CM.picture(22, 6, fmt, 10, 3)], 22, 6, odd=odd)


def window_cases():
    out = []
    for i, fmt in enumerate(CM.FORMATS):
        for j, name in enumerate(CM.WINDOWS):
            out.append(pytest.param(fmt, name, (10, 12, 16)[(i + j) % 3], (i + j) & 1, id="%s-%s" % (fmt, name)))
    return out


@pytest.mark.parametrize("fmt,name,depth,flip", window_cases())
def test_window_slot_and_stream(fmt, name, depth, flip):
    (sw, sh), (dw, dh), crop = CM.WINDOWS[name]
    frames = [CM.picture(sw, sh, fmt, depth, t) for t in range(1 if sw > 256 else 2)]
    slots = check(LIBS["rev" if flip else "fwd"], fmt, depth, frames, dw, dh, (sw, sh), crop, odd=bool(flip))
    if name == "pure_crop":                         # ... which is the ingest of the cropped region, from the kernels too
        cx, cy, cw, ch = crop
        cut = [tuple(np.ascontiguousarray(p[cy:cy + ch, (cx if k == 0 else cx // 2):(cx + cw if k == 0 else (cx + cw) // 2)]) for k, p in enumerate(f)) for f in frames]
        assert np.array_equal(check(LIBS["fwd"], fmt, depth, cut, dw, dh), slots)


@pytest.mark.parametrize("fmt", ["i422", "nv16_16", "uyvy", "yuyv_16", "p210", "y210"])
def test_frame_at_a_time(fmt):
    """H264E_encode_device and H264E_encode_device_scaled, planar, semi-planar and packed ("p210" / "y210": nv16_16 / yuyv_16 at depth 16)"""
    depth = 16 if fmt in ALIASES_16 else 10
    P = pkg.load_pkg()
    if fmt in ALIASES_16:
        assert P.dev_format(fmt) == P.dev_format(CM.ALIASES[fmt], depth=16)
    kw = dict(depth=depth) if CM.is_16(fmt) and fmt not in ALIASES_16 else {}
    lib = LIBS["fwd"]
    for (sw, sh), (dw, dh), crop in (((64, 48), (64, 48), None), ((100, 76), (64, 48), (2, 4, 96, 72))):
        frames = [CM.picture(sw, sh, fmt, depth, t) for t in range(2)]
        scaled = (sw, sh) != (dw, dh)
        win = dict(src_size=(sw, sh), crop=crop) if scaled else {}
        model = np.stack([CM.slot(f, fmt, depth, dw, dh, crop) if scaled else CM.slot(f, fmt, depth) for f in frames])
        _, want, want_sizes = run_clip(lib, dw, dh, len(frames), lambda ce: ce.upload(model))
        mem = DevMem(lib)
        try:
            e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
            parts = [e.encode_device(source(mem, f, fmt, odd=scaled), fmt, **win, **kw) for f in frames]
            e.close()
            assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes
        finally:
            mem.close()


def test_ladder_from_a_y210_source():
    """two rungs from one Y210 source: each rung's stream is the stream from the quantised, row-averaged NV12 source"""
    P = pkg.load_pkg()
    lib, (sw, sh), n = LIBS["fwd"], (128, 96), 2
    frames = [CM.picture(sw, sh, "y210", 16, t) for t in range(n)]
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26))]
    mem = DevMem(lib)
    try:
        got = P.encode_ladder([source(mem, f, "y210") for f in frames], "y210", (sw, sh), rungs, gop=GOP, lib=lib)
        for (out, sizes, _), (dw, dh, kw) in zip(got, rungs):
            model = np.stack([CM.slot(f, "y210", 16, dw, dh) if (dw, dh) != (sw, sh) else CM.slot(f, "y210", 16) for f in frames])
            ce = P.ClipEncoder(dw, dh, n, lib=lib, gop=GOP, **kw)
            ce.upload(model)
            want, want_sizes, _ = ce.encode()
            ce.close()
            assert out == want and sizes == want_sizes and len(out) > 0
    finally:
        mem.close()


# ---------------------------------------------------------------- the binding


def test_binding_names_codes_and_shapes():
    P = pkg.load_pkg()
    assert (P.DEV_CHROMA_422, P.DEV_PACK_YUYV, P.DEV_PACK_UYVY) == (0x4000, 0x4, 0x8)
    assert (P.DEV_FORMAT_I422, P.DEV_FORMAT_NV16, P.DEV_FORMAT_YUYV, P.DEV_FORMAT_UYVY) == (0x4000, 0x4001, 0x4004, 0x4008)
    assert P.DEV_FORMAT_P210 == P.DEV_FORMAT_P216 == 0x4801 and P.DEV_FORMAT_Y210 == P.DEV_FORMAT_Y216 == 0x4804
    assert [P.dev_format(f) for f in ("i422", "nv16", "yuyv", "yuy2", "uyvy")] == [0x4000, 0x4001, 0x4004, 0x4004, 0x4008]
    assert [P.dev_format(f, depth=10) for f in CM.FORMATS_16] == [0x4200, 0x4201, 0x4204, 0x4208]
    assert [P.dev_format(f) for f in ALIASES_16] == [0x4801, 0x4801, 0x4804, 0x4804] and P.dev_format("uyvy_16") == 0x4808
    for fmt, depth in (("i422_16", 8), ("yuyv_16", 17), ("p210", 10), ("y216", 12), ("i422", 10), ("uyvy", 16)):
        with pytest.raises(P.H264EError, match="depth"):
            P.dev_format(fmt, depth=depth)
    w, h = 6, 4
    u8 = lambda shape, strides: DevArray(4096, shape, strides, "|u1")          # noqa: E731
    u16 = lambda shape, strides: DevArray(4096, shape, strides, "<i2")         # noqa: E731
    d, _ = P.dev_frame(u8((8, 6), (6, 1)), "i422", w, h)
    assert d.format == 0x4000 and list(d.plane) == [4096, 4096 + 24, 4096 + 36] and list(d.stride) == [6, 3, 3]
    d, _ = P.dev_frame([u8((4, 6), (9, 1)), u8((4, 3), (5, 1)), u8((4, 3), (7, 1))], "i422", w, h)
    assert list(d.stride) == [9, 5, 7]
    d, _ = P.dev_frame(u16((8, 6), (12, 2)), "i422_16", w, h, depth=10)
    assert d.format == 0x4200 and list(d.plane) == [4096, 4096 + 48, 4096 + 72] and list(d.stride) == [12, 6, 6]
    d, _ = P.dev_frame(u8((8, 6), (10, 1)), "nv16", w, h)                      # one array, any row stride: the U,V rows follow the luma rows
    assert d.format == 0x4001 and list(d.plane)[:2] == [4096, 4096 + 40] and list(d.stride)[:2] == [10, 10]
    d, _ = P.dev_frame([u16((4, 6), (14, 2)), u16((4, 6), (12, 2))], "p210", w, h)
    assert d.format == 0x4801 and list(d.stride)[:2] == [14, 12]
    for shape, strides in (((4, 12), (13, 1)), ((4, 6, 2), (12, 2, 1))):
        d, _ = P.dev_frame(u8(shape, strides), "uyvy", w, h)
        assert d.format == 0x4008 and d.plane[0] == 4096 and d.stride[0] == strides[0]
    d, _ = P.dev_frame(u16((4, 6, 2), (26, 4, 2)), "y210", w, h)
    assert d.format == 0x4804 and d.stride[0] == 26
    d, _ = P.dev_frame((4096, 30), "yuy2", w, h)
    assert d.format == 0x4004 and d.plane[0] == 4096 and d.stride[0] == 30
    d, _ = P.dev_frame([(4096, 12), (8192, 6), (8200, 6)], "i422_16", w, h, depth=12)
    assert d.format == 0x4400 and list(d.stride) == [12, 6, 6]
    for name in CM.FORMATS_16 + ALIASES_16:         # 8-bit arrays for a 16-bit name, with the type named
        with pytest.raises(P.H264EError, match=r"%r takes 16-bit samples.*not \|u1" % name):
            P.dev_frame(u8((4, 12), (12, 1)) if CM.family(name) in ("yuyv", "uyvy") else u8((8, 6), (6, 1)), name, w, h)
    for name in CM.FORMATS_8:                       # ... and the reverse
        with pytest.raises(P.H264EError, match="device input must be 8-bit samples, not <i2"):
            P.dev_frame(u16((4, 12), (24, 2)) if CM.family(name) in ("yuyv", "uyvy") else u16((8, 6), (12, 2)), name, w, h)
    with pytest.raises(P.H264EError, match=r"packed 4:2:2 must be a \(4, 12\) or \(4, 6, 2\) array"):
        P.dev_frame(u8((4, 6), (6, 1)), "yuyv", w, h)
    with pytest.raises(P.H264EError, match=r"packed 4:2:2 must be"):
        P.dev_frame(u8((4, 6, 2), (24, 4, 1)), "uyvy", w, h)                   # pixels apart: not a packed row
    with pytest.raises(P.H264EError, match=r"contiguous \(8, 6\) array"):
        P.dev_frame(u8((8, 6), (7, 1)), "i422", w, h)
    with pytest.raises(P.H264EError, match=r"\(4, 3\) array"):
        P.dev_frame([u8((4, 6), (6, 1)), u8((2, 3), (3, 1)), u8((2, 3), (3, 1))], "i422", w, h)       # chroma planes of 4:2:0 size
    with pytest.raises(P.H264EError, match=r"NV16 takes \(y, uv\)"):
        P.dev_frame([u8((4, 6), (6, 1))] * 3, "nv16", w, h)


# ---------------------------------------------------------------- refusals


def test_refusals_name_the_value_launch_nothing_and_leave_the_encoders_usable():
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), n = (128, 96), (64, 48), 2
    lib = pkg.EMU_LIB
    fmt, depth = "yuyv_16", 10
    small = [CM.picture(dw, dh, fmt, depth, t) for t in range(n)]
    big = [CM.picture(sw, sh, fmt, depth, t) for t in range(n)]
    want_plain = run_clip(lib, dw, dh, n, lambda ce: ce.upload(np.stack([CM.slot(f, fmt, depth) for f in small])))[1]
    want_scaled = run_clip(lib, dw, dh, n, lambda ce: ce.upload(np.stack([CM.slot(f, fmt, depth, dw, dh) for f in big])))[1]
    mem = DevMem(lib)
    ce = P.ClipEncoder(dw, dh, n, gop=GOP, qp=QP, lib=lib)
    try:
        marker = np.arange(n * dw * dh * 3 // 2, dtype=np.uint32).astype(np.uint8).reshape(n, -1)
        ce.upload(marker)                           # what the slots hold while calls are refused; a picture for the way out to refuse
        ce.encode()
        py, pu, pv = [put_plane(mem, p, False) for p in small[0]]                   # 16-bit planes: dw*2, dw, dw bytes per row
        qy, qu, qv = [put_plane(mem, p, False) for p in big[0]]
        pk = put_plane(mem, CM.layout(small[0], fmt)[0], False)                     # a packed plane: dw*4 bytes per row
        qk = put_plane(mem, CM.layout(big[0], fmt)[0], False)
        tall = put_plane(mem, np.zeros((dh * 8 + 2, dw * 2), np.uint8), False)      # enough for an 8-bit 4:2:2 window beyond 8:1 in height
        wide = put_plane(mem, np.zeros((dh, dw * 34), np.uint8), False)             # ... and beyond 16:1 in width
        whole = dict(src_size=(sw, sh))
        I420, NV12, RGB, RGBP, D10, D16 = P.DEV_FORMAT_I420, P.DEV_FORMAT_NV12, P.DEV_FORMAT_RGB, P.DEV_FORMAT_RGBP, P.DEV_DEPTH(10), P.DEV_DEPTH(16)
        C422, C444, YUYV, UYVY = P.DEV_CHROMA_422, P.DEV_CHROMA_444, P.DEV_PACK_YUYV, P.DEV_PACK_UYVY
        cases = [
            # (planes, format, window, what the message holds)
            ([py, pu, pv], 0x2000, {}, "unknown format 8192"),                      # a bit outside 0x5f3f: bit 13 stays unassigned
            ([py, pu, pv], C422 | 0x40, {}, "unknown format 16448"),
            ([qy, qu, qv], C422 | 0x8000, whole, "unknown format 49152"),
            # 4:2:2 together with 4:4:4
            ([py, py, py], I420 | C422 | C444, {}, r"format 20480 asks for both 4:2:2 chroma \(0x4000\) and 4:4:4 chroma \(0x1000\)"),
            ([qy, qy, qy], I420 | C422 | C444 | D10, whole, r"format 20992 asks for both 4:2:2 chroma \(0x4000\) and 4:4:4 chroma \(0x1000\)"),
            # 4:2:2 or a pack bit on RGB / RGBP, or together with a float sample type
            ([py, pu, pv], RGB | C422, {}, r"format 16386 asks for 4:2:2 chroma of RGB \(format 2\)"),
            ([py, pu, pv], RGBP | C422, {}, r"format 16387 asks for 4:2:2 chroma of RGBP \(format 3\)"),
            ([qy, qu, qv], RGBP | C422, whole, r"format 16387 asks for 4:2:2 chroma of RGBP \(format 3\)"),
            ([pk, pk, pk], RGB | C422 | YUYV, {}, r"format 16390 asks for packed 4:2:2 samples of RGB \(format 2\)"),
            ([pk, pk, pk], RGBP | C422 | UYVY, {}, r"format 16395 asks for packed 4:2:2 samples of RGBP \(format 3\)"),
            ([py, pu, pv], I420 | C422 | P.DEV_SAMPLE_F16, {}, r"format 16400 asks for 4:2:2 chroma \(0x4000\) of f16 samples \(0x10\)"),
            ([py, pu, pv], RGBP | C422 | P.DEV_SAMPLE_F32, {}, r"format 16435 asks for 4:2:2 chroma \(0x4000\) of f32 samples \(0x30\)"),
            ([qy, qu, qv], NV12 | C422 | P.DEV_SAMPLE_BF16, whole, r"format 16417 asks for 4:2:2 chroma \(0x4000\) of bf16 samples \(0x20\)"),
            # both pack bits
            ([pk, pk, pk], I420 | C422 | YUYV | UYVY, {}, r"format 16396 sets both pack bits \(0xc\)"),
            ([qk, qk, qk], I420 | C422 | YUYV | UYVY | D10, whole, r"format 16908 sets both pack bits \(0xc\)"),
            # a pack bit without 0x4000, or on the NV12 base
            ([pk, pk, pk], I420 | YUYV, {}, r"unknown format 4: packed YUYV samples \(0x4\) come with 4:2:2 chroma \(0x4000\)"),
            ([pk, pk, pk], I420 | UYVY | D10, {}, r"unknown format 520: packed UYVY samples \(0x8\) come with 4:2:2 chroma \(0x4000\)"),
            ([qk, qk, qk], NV12 | UYVY, whole, r"unknown format 9: packed UYVY samples \(0x8\) come with 4:2:2"),
            ([pk, pk, pk], NV12 | C422 | YUYV, {}, r"format 16389 asks for packed YUYV samples \(0x4\) of NV12 \(format 1\)"),
            ([qk, qk, qk], NV12 | C422 | UYVY | D16, whole, r"format 18441 asks for packed UYVY samples \(0x8\) of NV12 \(format 1\)"),
            # 16-bit planes whose pointer or stride is not a multiple of 2
            ([py, (pu[0] + 1, pu[1]), pv], I420 | C422 | D10, {}, r"plane 1 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes of a u16 sample"),
            ([py, (pu[0], pu[1] + 1), pv], NV12 | C422 | D16, {}, "stride %d of plane 1 is not a multiple of the 2 bytes of a u16 sample" % (pu[1] + 1)),
            ([(pk[0] + 1, pk[1])], I420 | C422 | YUYV | D10, {}, r"plane 0 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes of a u16 sample"),
            ([(qk[0], qk[1] + 3)], I420 | C422 | UYVY | D16, whole, "stride %d of plane 0 is not a multiple of the 2 bytes of a u16 sample" % (qk[1] + 3)),
            ([qy, qu, (qv[0] + 1, qv[1])], I420 | C422 | D10, whole, r"plane 2 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes"),
            # a stride below the row's bytes; a packed row is 2 * width * sample_bytes
            ([(py[0], 2 * dw - 2), pu, pv], I420 | C422 | D10, {}, "stride 126 of plane 0 is below its 128 row bytes"),
            ([py, (pu[0], dw - 2), pv], I420 | C422 | D10, {}, "stride 62 of plane 1 is below its 64 row bytes"),
            ([py, pu, (pv[0], dw // 2 - 1)], I420 | C422, {}, "stride 31 of plane 2 is below its 32 row bytes"),
            ([py, (py[0], 2 * dw - 2)], NV12 | C422 | D10, {}, "stride 126 of plane 1 is below its 128 row bytes"),
            ([(pk[0], 4 * dw - 2)], I420 | C422 | YUYV | D10, {}, "stride 254 of plane 0 is below its 256 row bytes"),
            ([(pk[0], 2 * dw - 1)], I420 | C422 | UYVY, {}, "stride 127 of plane 0 is below its 128 row bytes"),
            ([qy, (qu[0], sw - 2), qv], I420 | C422 | D10, whole, "stride 126 of plane 1 is below the 128 bytes of a source row"),
            ([qy, (qy[0], 2 * sw - 2)], NV12 | C422 | D10, whole, "stride 254 of plane 1 is below the 256 bytes of a source row"),
            ([(qk[0], 4 * sw - 2)], I420 | C422 | YUYV | D10, whole, "stride 510 of plane 0 is below the 512 bytes of a source row"),
            ([(qk[0], 2 * sw - 1)], I420 | C422 | UYVY, whole, "stride 255 of plane 0 is below the 256 bytes of a source row"),
            # a 4:2:2 window beyond 8 times the picture in height (its chroma would go beyond 16:1), or 16 times in width
            ([tall, tall, tall], I420 | C422, dict(src_size=(dw, dh * 8 + 2)), "4:2:2 window height 386 is more than 8 times the picture's 48 .*at most 16 to 1"),
            ([tall], I420 | C422 | UYVY, dict(src_size=(dw, dh * 8 + 2)), "4:2:2 window height 386 is more than 8 times the picture's 48 .*at most 16 to 1"),
            ([wide, wide, wide], NV12 | C422, dict(src_size=(dw * 16 + 2, dh)), "window width 1026 is more than 16 times the picture's 64"),
            ([wide], I420 | C422 | YUYV, dict(src_size=(dw * 16 + 2, dh)), "window width 1026 is more than 16 times the picture's 64"),
        ]
        for planes, code, kw, msg in cases:
            d = P.DevFrame(format=code, pixel_bytes=3)
            for k, (ptr, stride) in enumerate(planes):
                d.plane[k], d.stride[k] = ptr, stride
            win = P.dev_window(kw.get("src_size"), kw.get("crop"), dw, dh)[0]
            e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
            data, size = C.c_void_p(), C.c_int()
            if win is not None:
                assert ce.L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(win)) != 0, msg
                text = ce.L.H264E_last_error().decode()
                assert e.L.H264E_encode_device_scaled(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(win), C.byref(data), C.byref(size)) != 0
            else:
                assert ce.L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) != 0, msg
                text = ce.L.H264E_last_error().decode()
                assert e.L.H264E_encode_device(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(data), C.byref(size)) != 0
            assert re.search(msg, text), (msg, text)
            assert re.search(msg, e.L.H264E_last_error().decode()), (msg, e.L.H264E_last_error().decode())
            assert np.array_equal(ce.download(), marker), "a refused call wrote the slot: " + msg       # nothing was launched
            e.close()
        # the limits themselves are taken: 8:1 in height, 16:1 in width
        for planes, code, size in (([tall, tall, tall], I420 | C422, (dw, dh * 8)), ([wide], I420 | C422 | YUYV, (dw * 16, dh))):
            d = P.DevFrame(format=code, pixel_bytes=0)
            for k, (ptr, stride) in enumerate(planes):
                d.plane[k], d.stride[k] = ptr, stride
            win = P.dev_window(size, None, dw, dh)[0]
            assert ce.L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(win)) == 0, ce.L.H264E_last_error().decode()
        ce.upload(marker)
        # the way out accepts none of the new bits: its refusal is the one it had
        out = mem.block(np.full(4 * dw * dh * 3, SENTINEL, np.uint8))
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
        e.encode(marker[0])
        for code in (I420 | C422, NV12 | C422, I420 | C422 | YUYV, I420 | C422 | UYVY, P.DEV_FORMAT_P210, P.DEV_FORMAT_Y216, I420 | C422 | D10, YUYV, UYVY):
            d = P.DevFrame(format=code, pixel_bytes=0)
            for k in range(3):
                d.plane[k], d.stride[k] = out + k * 4 * dw * dh, 4 * dw
            assert ce.L.H264E_clip_read_recon_device(ce.c, 0, C.byref(d)) != 0
            assert ce.L.H264E_last_error().decode().endswith("egress: unknown format %d" % code)
            assert e.L.H264E_read_recon_device(e.persist, C.byref(d)) != 0
            assert e.L.H264E_last_error().decode().endswith("egress: unknown format %d" % code)
        e.close()
        host = np.empty(4 * dw * dh * 3, np.uint8)
        assert ce.L.H264E_dev_memcpy(host.ctypes.data, out, host.size, 0) == 0 and (host == SENTINEL).all()
        for name in ("i422", "nv16", "yuyv", "uyvy", "p210", "y210"):
            with pytest.raises(P.H264EError, match="unknown format"):
                ce.read_recon_device(0, name, out=[(out, 4 * dw)] * {"i422": 3, "nv16": 2, "p210": 2}.get(name, 1))
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
