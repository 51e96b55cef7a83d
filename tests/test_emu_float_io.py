"""CPU: float planar RGB device frames (H264E_DEV_FORMAT_RGBP | H264E_DEV_SAMPLE_F16 / _BF16 / _F32) in the lane-loop emulation of the
kernels (tests/emu), both lane orders.  The emulation's "device" memory is what H264E_dev_malloc hands out -- its global-memory accessors
abort on any other address, and every source block here ends with the last byte of the plane's last row, so a read beyond it would abort
the test.

  - way in: the input slot holds exactly rgbp_model.to_i420 / scale_to_i420 of the QUANTISED frame (tests/float_model.py), and the clip
    stream and the frame-at-a-time stream are the oracle's for that I420 -- ragged groups, a row that crosses the 256-lane block, all
    65536 bit patterns of the 16-bit types, the float32 edge set, windows, and every layout;
  - way out: bit for bit the model's table applied to the 8-bit planar RGB of the same picture, for every colour setting, on pictures
    whose 8-bit planes hold all 256 values; nothing outside the rows is written;
  - what is refused is refused with a message that names the value, and the encoders go on working.  (A plane that leaves its
    allocation is refused by the product alone -- the emulation has no allocator to ask: tests/test_gpu_float_io.py.)

Every comparison is equality of bytes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clips
import float_model as FM
import oracle_lib
import pkg
import rgbp_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}
SENTINEL, GUARD = 0xA5, 16
COLORS = [None, "bt709", "bt601-full", "bt709-full"]
LAYOUTS = ["chw", "slice", "padded", "separate"]
GOP, QP = 30, 26


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

    def read(self, ptr, n):
        host = np.empty(n, np.uint8)
        assert self.L.H264E_dev_memcpy(host.ctypes.data, ptr, n, 0) == 0
        return host

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def place(layout, kind, h, w):
    """where the three planes of a (3, h, w) frame lie: [(block index, byte offset, row stride in bytes)] and the size of every block.
    Every block ends with the last byte of its last row; "padded" starts at an address that is a multiple of the sample size and of
    nothing larger, with rows apart by an odd number of samples"""
    sb = FM.BYTES[kind]
    rb = w * sb
    if layout == "chw":
        return [(0, c * h * rb, rb) for c in range(3)], [3 * h * rb]
    if layout == "slice":                   # channels 1..3 of a block of five
        return [(0, (c + 1) * h * rb, rb) for c in range(3)], [4 * h * rb]
    if layout == "padded":                  # one block, rows and planes padded
        stride = rb + 5 * sb
        plane = stride * h + 3 * sb
        return [(0, sb + c * plane, stride) for c in range(3)], [sb + 2 * plane + stride * (h - 1) + rb]
    if layout == "separate":
        return [(c, (0, sb, 3 * sb)[c], rb + c * sb) for c in range(3)], [(0, sb, 3 * sb)[c] + (rb + c * sb) * (h - 1) + rb for c in range(3)]
    raise ValueError(layout)


def describe(kind, ptrs, strides, h, w, layout):
    """what the binding takes for planes at ptrs: an array with __cuda_array_interface__ where the type has a typestr and the planes
    are evenly spaced, else three (pointer, stride) pairs"""
    if FM.TYPESTR[kind] and layout != "separate":
        return DevArray(ptrs[0], (3, h, w), (ptrs[1] - ptrs[0], strides[0], FM.BYTES[kind]), FM.TYPESTR[kind])
    if FM.TYPESTR[kind]:
        return [DevArray(p, (h, w), (s, FM.BYTES[kind]), FM.TYPESTR[kind]) for p, s in zip(ptrs, strides)]
    return [(p, s) for p, s in zip(ptrs, strides)]


def source(mem, bits, kind, layout):
    """the (3, h, w) bit patterns in device memory, as upload_device(..., "rgbp_<kind>") takes them"""
    _, h, w = bits.shape
    planes, sizes = place(layout, kind, h, w)
    host = [np.full(n, SENTINEL, np.uint8) for n in sizes]
    raw = np.ascontiguousarray(bits, FM.BITS[kind]).view(np.uint8).reshape(3, h, -1)
    for c, (b, off, stride) in enumerate(planes):
        for y in range(h):
            host[b][off + y * stride: off + y * stride + raw.shape[2]] = raw[c, y]
    base = [mem.block(hb) for hb in host]
    return describe(kind, [base[b] + off for b, off, _ in planes], [s for _, _, s in planes], h, w, layout)


def clip_stream(lib, w, h, n, put, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, lib=lib, **kw)
    try:
        put(ce)
        slots = ce.download()
        out, sizes, _ = ce.encode()
        return slots, out, sizes
    finally:
        ce.close()


def check_way_in(lib, kind, frames, layout, dw, dh, src_size=None, crop=None, stream=True):
    """slot bytes, the clip stream and the frame-at-a-time stream of float frames against the model of the quantised frames"""
    P = pkg.load_pkg()
    n = len(frames)
    quantised = [FM.quantise(f, kind) for f in frames]
    model = np.stack([M.to_i420(q) if src_size is None else M.scale_to_i420(q, dw, dh, crop) for q in quantised])
    fmt = FM.FORMAT[kind]
    mem = DevMem(lib)
    try:
        slots, got, sizes = clip_stream(lib, dw, dh, n, lambda ce: ce.upload_device([source(mem, f, kind, layout) for f in frames], fmt, src_size=src_size, crop=crop),
                                        gop=GOP, qp=QP)
        assert np.array_equal(slots, model), "%s %s: slot contents differ from the model of the quantised frame" % (kind, layout)
        if not stream:
            return
        want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=GOP, qp=QP)
        assert got == want and sizes == want_sizes, "%s %s: the clip stream differs from the oracle's for the quantised frames" % (kind, layout)
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=lib)
        parts = [e.encode_device(source(mem, f, kind, layout), fmt, src_size=src_size, crop=crop) for f in frames]
        e.close()
        assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes, "%s %s: the frame-at-a-time stream differs" % (kind, layout)
    finally:
        mem.close()


# ---------------------------------------------------------------- way in, at the picture's size


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("w,h", [(2, 2), (6, 4), (1030, 4)])
def test_plain_slot_and_streams(w, h, kind):
    """2 x 2: one ragged group; 6 x 4: a whole and a ragged group, 3 chroma samples; 1030 x 4: 258 groups, the row crosses the 256-lane block"""
    i = FM.KINDS.index(kind) + (w // 2)
    frames = [FM.ramp_picture(w, h, kind, t) for t in range(2)]
    check_way_in(LIBS["rev" if i & 1 else "fwd"], kind, frames, LAYOUTS[i % 4], w, h)


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plain_layouts(layout, kind):
    frames = [FM.ramp_picture(22, 6, kind, 5)]
    check_way_in(LIBS["fwd"], kind, frames, layout, 22, 6, stream=False)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_all_16_bit_patterns(kind):
    """a 256 x 256 picture whose channels each hold all 65536 bit patterns, in different orders: NaNs, infinities, denormals, negatives"""
    pic = FM.all_patterns_picture()
    for c in range(3):
        assert np.array_equal(np.sort(pic[c].reshape(-1)), np.arange(65536))
    check_way_in(LIBS["fwd"], kind, [pic], "chw", 256, 256)


def test_f32_edge_set():
    pic = FM.f32_edge_picture()
    assert np.isin(FM.f32_edge_bits(), pic[0]).all()
    check_way_in(LIBS["rev"], "f32", [pic], "padded", pic.shape[2], pic.shape[1])


# ---------------------------------------------------------------- way in, through a window

WINDOWS = {"2to1": ((128, 96), (64, 48), None), "crop_and_scale": ((200, 120), (66, 50), (2, 4, 198, 116)), "pure_crop": ((128, 96), (64, 48), (64, 48, 64, 48))}


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_slot_and_streams(name, kind):
    (sw, sh), (dw, dh), crop = WINDOWS[name]
    i = FM.KINDS.index(kind) + sorted(WINDOWS).index(name)
    frames = [FM.ramp_picture(sw, sh, kind, t) for t in range(2)]
    check_way_in(LIBS["rev" if i & 1 else "fwd"], kind, frames, LAYOUTS[(i + 1) % 4], dw, dh, (sw, sh), crop)
    if name == "pure_crop":                 # ... which is the plain ingest of the cropped region
        q = FM.quantise(frames[0], kind)
        assert np.array_equal(M.scale_to_i420(q, dw, dh, crop), M.to_i420(q[:, 48:, 64:]))


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_window_layouts(layout, kind):
    frames = [FM.ramp_picture(40, 24, kind, 9)]
    check_way_in(LIBS["fwd"], kind, frames, layout, 18, 10, (40, 24), (2, 2, 36, 20), stream=False)


# ---------------------------------------------------------------- way out


class FloatDest:
    """a float (3, h, w) destination in sentinel-filled device memory; result() reads the bit patterns back and asserts that every byte
    outside the rows still holds the sentinel"""

    def __init__(self, mem, kind, w, h, layout):
        self.mem, self.kind, self.w, self.h = mem, kind, w, h
        planes, sizes = place(layout, kind, h, w)
        self.planes = [(b, off + GUARD, stride) for b, off, stride in planes]
        self.blocks = [(mem.block(np.full(n + 2 * GUARD, SENTINEL, np.uint8)), n + 2 * GUARD) for n in sizes]
        self.out = describe(kind, [self.blocks[b][0] + off for b, off, _ in self.planes], [s for _, _, s in self.planes], h, w, layout)

    def result(self):
        rb = self.w * FM.BYTES[self.kind]
        host = [self.mem.read(p, n) for p, n in self.blocks]
        got = []
        for b, off, stride in self.planes:
            got.append(np.stack([host[b][off + y * stride: off + y * stride + rb] for y in range(self.h)]).copy())
            for y in range(self.h):
                host[b][off + y * stride: off + y * stride + rb] = SENTINEL
        for b, hb in enumerate(host):
            bad = np.flatnonzero(hb != SENTINEL)
            assert bad.size == 0, "%s: %d bytes outside the rows were written, the first at offset %d of block %d" % (self.kind, bad.size, bad[0], b)
        return np.stack(got).view(FM.BITS[self.kind]).reshape(3, self.h, self.w)

    def untouched(self):
        return all((self.mem.read(p, n) == SENTINEL).all() for p, n in self.blocks)


def eight_bit(mem, read, w, h):
    """the 8-bit planar RGB of a picture through read(fmt, out)"""
    base = mem.block(np.full(3 * h * w, SENTINEL, np.uint8))
    read("rgbp", DevArray(base, (3, h, w), (h * w, w, 1), "|u1"))
    return mem.read(base, 3 * h * w).reshape(3, h, w)


def check_way_out(mem, read, w, h, what):
    u8 = eight_bit(mem, read, w, h)
    for i, kind in enumerate(FM.KINDS):
        for layout in LAYOUTS:
            d = FloatDest(mem, kind, w, h, layout)
            read(FM.FORMAT[kind], d.out)
            assert np.array_equal(d.result(), FM.dequantise(u8, kind)), "%s %s %s: the destination differs from the model of the 8-bit planes" % (what, kind, layout)
    return u8


def full_range_frames(w, h, n):
    """noise over the whole byte range: at a low QP its reconstruction, converted to RGB, holds every value"""
    return clips.noise(w, h, n)


@pytest.mark.parametrize("color", COLORS, ids=lambda c: c or "default")
def test_clip_way_out(color):
    P = pkg.load_pkg()
    w, h, n = 70, 36, 3                      # 70: a ragged group of two; the coded size is larger than the picture
    lib = LIBS["rev" if COLORS.index(color) & 1 else "fwd"]
    mem = DevMem(lib)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=4, lib=lib, color=color)
    try:
        ce.upload(full_range_frames(w, h, n))
        ce.encode()
        seen = np.zeros(256, bool)
        for f in range(n):
            u8 = check_way_out(mem, lambda fmt, out: ce.read_recon_device(f, fmt, out=out), w, h, "frame %d colour %s" % (f, color))
            seen[np.unique(u8)] = True
        assert seen.all(), "the 8-bit planes of these pictures miss the values %s: the tables were not exercised whole" % np.flatnonzero(~seen)
    finally:
        ce.close()
        mem.close()


@pytest.mark.parametrize("w,h", [(2, 2), (1030, 4)])
def test_frame_at_a_time_way_out(w, h):
    P = pkg.load_pkg()
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=GOP, qp=4, lib=pkg.EMU_LIB, color="bt601-full")
    try:
        for t, frame in enumerate(full_range_frames(w, h, 2)):
            e.encode(frame)
            check_way_out(mem, lambda fmt, out: e.read_recon_device(fmt, out=out), w, h, "frame %d" % t)
    finally:
        e.close()
        mem.close()


# ---------------------------------------------------------------- the binding


def test_binding_names_and_codes():
    P = pkg.load_pkg()
    assert (P.DEV_SAMPLE_U8, P.DEV_SAMPLE_F16, P.DEV_SAMPLE_BF16, P.DEV_SAMPLE_F32) == (0x00, 0x10, 0x20, 0x30)
    assert (P.DEV_FORMAT_RGBP_F16, P.DEV_FORMAT_RGBP_BF16, P.DEV_FORMAT_RGBP_F32) == (19, 35, 51)
    assert [P.dev_format(FM.FORMAT[k]) for k in FM.KINDS] == [19, 35, 51]
    a = DevArray(4096, (3, 4, 6), (96, 24, 4), "<f4")
    assert P.dev_format("rgbpf", a) == 51 and P.dev_format("rgbpf", DevArray(4096, (3, 4, 6), (48, 12, 2), "<f2")) == 19
    d, _ = P.dev_frame(a, "rgbpf", 6, 4)
    assert d.format == 51 and list(d.plane) == [4096, 4192, 4288] and list(d.stride) == [24, 24, 24]
    for bad, name in ((DevArray(4096, (3, 4, 6), (24, 6, 1), "|u1"), r"\|u1"), (DevArray(4096, (3, 4, 6), (192, 48, 8), "<f8"), "<f8"), ([(4096, 24)] * 3, "pair")):
        with pytest.raises(P.H264EError, match="float16, bfloat16 or float32 samples.*" + name):
            P.dev_frame(bad, "rgbpf", 6, 4)
    with pytest.raises(P.H264EError, match="takes float16 samples, not <f4"):
        P.dev_frame(a, "rgbp_f16", 6, 4)
    with pytest.raises(P.H264EError, match="uint8 samples, not <f4"):           # today's refusal keeps its text
        P.dev_frame(a, "rgbp", 6, 4)
    with pytest.raises(P.H264EError, match="last axis is contiguous"):
        P.dev_frame(DevArray(4096, (3, 4, 6), (4, 72, 12), "<f4"), "rgbp_f32", 6, 4)


# ---------------------------------------------------------------- refusals


def test_refusals_name_the_value_and_leave_the_encoders_usable():
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), n = (128, 96), (64, 48), 2
    lib = pkg.EMU_LIB
    kind, sb = "f16", 2
    small = [FM.ramp_picture(dw, dh, kind, t) for t in range(n)]
    big = [FM.ramp_picture(sw, sh, kind, t) for t in range(n)]
    want_plain = oracle_lib.encode_clip(np.stack([M.to_i420(FM.quantise(f, kind)) for f in small]), dw, dh, gop=GOP, qp=QP)[0]
    want_scaled = oracle_lib.encode_clip(np.stack([M.scale_to_i420(FM.quantise(f, kind), dw, dh) for f in big]), dw, dh, gop=GOP, qp=QP)[0]
    mem = DevMem(lib)
    ce = P.ClipEncoder(dw, dh, n, gop=GOP, qp=QP, lib=lib)
    try:
        ce.upload(np.zeros((n, dw * dh * 3 // 2), np.uint8))         # a picture for the way out to refuse
        ce.encode()
        r, g, b = source(mem, small[0], kind, "separate")
        R, G, B = source(mem, big[0], kind, "separate")
        pr, pg, pb = [(a.__cuda_array_interface__["data"][0], a.__cuda_array_interface__["strides"][0]) for a in (r, g, b)]
        qr, qg, qb = [(a.__cuda_array_interface__["data"][0], a.__cuda_array_interface__["strides"][0]) for a in (R, G, B)]
        f32 = source(mem, FM.ramp_picture(dw, dh, "f32", 0), "f32", "separate")
        fr, fg, fb = [(a.__cuda_array_interface__["data"][0], a.__cuda_array_interface__["strides"][0]) for a in f32]
        whole = dict(src_size=(sw, sh))
        y8 = (pr[0], dw)
        cases = [
            # (planes, format, window, what the message holds)
            ([pr, (pg[0] + 1, pg[1]), pb], "rgbp_f16", {}, r"plane 1 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes of a f16 sample"),
            ([fr, fg, (fb[0] + 2, fb[1])], "rgbp_f32", {}, r"plane 2 \(0x[0-9a-f]+\) is not a multiple of the 4 bytes of a f32 sample"),
            ([pr, pg, (pb[0], pb[1] + 1)], "rgbp_bf16", {}, "stride %d of plane 2 is not a multiple of the 2 bytes of a bf16 sample" % (pb[1] + 1)),
            ([fr, (fg[0], fg[1] + 2), fb], "rgbp_f32", {}, "stride %d of plane 1 is not a multiple of the 4 bytes" % (fg[1] + 2)),
            ([pr, pg, (pb[0], dw * sb - 2)], "rgbp_f16", {}, "stride 126 of plane 2 is below its 128 row bytes"),
            ([fr, (fg[0], dw * 2), fb], "rgbp_f32", {}, "stride 128 of plane 1 is below its 256 row bytes"),
            ([(qr[0] + 1, qr[1]), qg, qb], "rgbp_f16", whole, r"plane 0 \(0x[0-9a-f]+\) is not a multiple of the 2 bytes"),
            ([qr, (qg[0], qg[1] + 1), qb], "rgbp_f16", whole, "stride %d of plane 1 is not a multiple of the 2 bytes" % (qg[1] + 1)),
            ([qr, qg, (qb[0], sw * sb - 2)], "rgbp_f16", whole, "stride 254 of plane 2 is below the 256 bytes of a source row"),
            # a sample type on the other layouts, and bits that mean nothing
            ([y8, y8, y8], P.DEV_FORMAT_I420 | P.DEV_SAMPLE_F16, {}, r"format 16 asks for f16 samples \(0x10\) of I420"),
            ([y8, y8, y8], P.DEV_FORMAT_NV12 | P.DEV_SAMPLE_F32, {}, r"format 49 asks for f32 samples \(0x30\) of NV12"),
            ([y8, y8, y8], P.DEV_FORMAT_RGB | P.DEV_SAMPLE_BF16, {}, r"format 34 asks for bf16 samples \(0x20\) of RGB"),
            ([y8, y8, y8], P.DEV_FORMAT_NV12 | P.DEV_SAMPLE_F16, whole, r"format 17 asks for f16 samples \(0x10\) of NV12"),
            ([pr, pg, pb], 0x43, {}, "unknown format 67"),
            ([qr, qg, qb], 0x43, whole, "unknown format 67"),
        ]
        for planes, fmt, kw, msg in cases:
            d = P.DevFrame(format=P.dev_format(fmt), pixel_bytes=3)
            for k, (ptr, stride) in enumerate(planes):
                d.plane[k], d.stride[k] = ptr, stride
            win = P.dev_window(kw.get("src_size"), None, dw, dh)[0]
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
            # the way out refuses the same descriptions (a window has no meaning there), and writes nothing
            if not kw:
                assert ce.L.H264E_clip_read_recon_device(ce.c, 0, C.byref(d)) != 0
                out_text = ce.L.H264E_last_error().decode()
                assert re.search(msg, out_text) and out_text.startswith("egress"), (msg, out_text)
            # ... and the next frames are taken: the stream of a fresh encoder, from both
            if kw:
                ce.upload_device([source(mem, f, kind, "padded") for f in big], "rgbp_f16", **whole)
                parts = [e.encode_device(source(mem, f, kind, "chw"), "rgbpf", **whole) for f in big]
            else:
                ce.upload_device([source(mem, f, kind, "padded") for f in small], "rgbp_f16")
                parts = [e.encode_device(source(mem, f, kind, "chw"), "rgbpf") for f in small]
            e.close()
            assert ce.encode()[0] == (want_scaled if kw else want_plain), msg
            assert b"".join(parts) == (want_scaled if kw else want_plain), msg
    finally:
        ce.close()
        mem.close()


def test_refused_way_out_leaves_the_destination_untouched():
    P = pkg.load_pkg()
    w, h = 64, 48
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, 1, gop=GOP, qp=QP, lib=pkg.EMU_LIB)
    try:
        ce.upload(clips.noise(w, h, 1))
        ce.encode()
        for kind in FM.KINDS:
            sb = FM.BYTES[kind]
            d = FloatDest(mem, kind, w, h, "separate")
            ptrs = [(d.blocks[b][0] + off, s) for b, off, s in d.planes]
            for planes, msg in (([ptrs[0], (ptrs[1][0] + 1, ptrs[1][1]), ptrs[2]], "plane 1 .* is not a multiple of the %d bytes" % sb),
                                ([ptrs[0], ptrs[1], (ptrs[2][0], ptrs[2][1] + sb - 1)], "stride %d of plane 2 is not a multiple" % (ptrs[2][1] + sb - 1)),
                                ([(ptrs[0][0], w * sb - sb), ptrs[1], ptrs[2]], "stride %d of plane 0 is below its %d row bytes" % (w * sb - sb, w * sb))):
                with pytest.raises(P.H264EError, match=msg):
                    ce.read_recon_device(0, FM.FORMAT[kind], out=planes)
                assert d.untouched()
            ce.read_recon_device(0, FM.FORMAT[kind], out=d.out)
            assert np.array_equal(d.result(), FM.dequantise(eight_bit(mem, lambda fmt, out: ce.read_recon_device(0, fmt, out=out), w, h), kind))
    finally:
        ce.close()
        mem.close()
