"""CPU: device input of another size (H264E_clip_upload_device_scaled / H264E_encode_device_scaled, enc_scale.h) in the lane-loop emulation
of the kernels (tests/emu), both lane orders.  The emulation's "device" memory is what H264E_dev_malloc hands out -- its global-memory
accessors abort on any other address, and every source block here ends with the last byte of the plane's last row, so a read beyond the
window's last byte would abort the test.

  - the model (tests/scale_model.py) has the properties the definition promises;
  - the input slots hold exactly the model's bytes: I420 packed, with padded odd strides at odd addresses and in separate planes, NV12;
    ratios 1:1 (a crop) to 16:1, uneven per axis, ragged tiles, the 4096 x 4096 bound of the 32-bit arithmetic;
  - the streams are the oracle's for the model's frames, and those of upload() of the model's frames, through both entry points and with
    slices, rate control, a bounded ring and the denoiser;
  - what is refused is refused with a message, and the encoder goes on working;
  - encode_ladder gives per rung the stream of a standalone encoder.

The issue's geometry "34x50 -> 2x2" is 17:1 and 25:1, beyond the 16:1 cap the same issue sets and wants refused; it is covered as the far
32 x 32 corner of a 34 x 50 source -> 2x2 (16:1 in both axes), and the whole 34 x 50 source is asserted to be refused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clips
import oracle_lib
import pkg
import scale_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


class DevMem:
    """device memory of one library (H264E_dev_malloc), freed by close()"""

    def __init__(self, lib):
        self.L = pkg.load_pkg().load(lib)
        self.blocks = []

    def put(self, arr, stride=None, offset=0):
        """rows of the 2-D `arr` `stride` bytes apart, starting `offset` bytes into a fresh block, as a (pointer, stride) pair; the
        padding holds 0xA5 and the block ends with the last row's last byte"""
        arr = np.ascontiguousarray(arr, np.uint8)
        rows, rb = arr.shape
        stride = stride or rb
        host = np.full(offset + stride * (rows - 1) + rb, 0xA5, np.uint8)
        for y in range(rows):
            host[offset + y * stride: offset + y * stride + rb] = arr[y]
        base = self.L.H264E_dev_malloc(0, host.size)
        assert base
        self.blocks.append(base)
        assert self.L.H264E_dev_memcpy(base, host.ctypes.data, host.size, 1) == 0
        return (base + offset, stride)

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def source(mem, frame, w, h, layout):
    """(what upload_device takes, format name) for one packed I420 frame of w x h"""
    y, u, v = M.split(frame, w, h)
    if layout == "packed":                  # one block, planes behind each other, rows packed
        return mem.put(np.asarray(frame).reshape(h * 3 // 2, w)), "i420"
    if layout == "padded":                  # odd strides
        return [mem.put(y, w + 13), mem.put(u, w // 2 + 7), mem.put(v, w // 2 + 1)], "i420"
    if layout == "oddbase":                 # odd start addresses (and strides that keep every row odd or even by turns)
        return [mem.put(y, w + 3, 1), mem.put(u, w // 2 + 2, 3), mem.put(v, w // 2 + 5, 1)], "i420"
    if layout == "separate":                # three allocations, rows packed
        return [mem.put(y), mem.put(u), mem.put(v)], "i420"
    if layout == "nv12":
        yy, uv = M.nv12_planes(frame, w, h)
        return (mem.put(yy), mem.put(uv)), "nv12"
    if layout == "nv12_padded":
        yy, uv = M.nv12_planes(frame, w, h)
        return (mem.put(yy, w + 5, 3), mem.put(uv, w + 9, 1)), "nv12"
    raise ValueError(layout)


def feed(ce, mem, frames, sw, sh, layout, crop, first=0):
    srcs = [source(mem, f, sw, sh, layout) for f in frames]
    ce.upload_device([s[0] for s in srcs], srcs[0][1], first=first, src_size=(sw, sh), crop=crop)


def model_frames(frames, sw, sh, dw, dh, crop):
    return np.stack([M.scale_frame(f, sw, sh, dw, dh, crop) for f in frames])


# ---------------------------------------------------------------- the model


def test_model_is_the_stated_definition():
    rng = np.random.default_rng(1)
    for sw, sh, dw, dh, cx, cy in ((6, 4, 6, 4, 0, 0), (8, 6, 4, 3, 2, 2), (9, 7, 6, 2, 1, 0), (10, 6, 6, 4, 0, 2), (16, 16, 1, 1, 0, 0), (17, 5, 2, 5, 1, 1), (7, 9, 5, 4, 0, 0)):
        src = rng.integers(0, 256, (cy + sh + 1, cx + sw + 2), dtype=np.uint8)
        assert np.array_equal(M.scale_plane(src, cx, cy, sw, sh, dw, dh), M.scale_plane_direct(src, cx, cy, sw, sh, dw, dh)), (sw, sh, dw, dh)


def test_model_properties():
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (96, 128), dtype=np.uint8)
    # equal sizes copy: a pure crop gives exactly the source samples
    assert np.array_equal(M.scale_plane(src, 10, 6, 64, 48, 64, 48), src[6:54, 10:74])
    # 2:1 in both axes is the rounded mean of each 2 x 2 block
    s = src.astype(np.int64)
    assert np.array_equal(M.scale_plane(src, 0, 0, 128, 96, 64, 48), (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2)
    # the weights of every destination column sum to Sw
    for sw, dw in ((128, 64), (100, 36), (96, 64), (256, 16), (4096, 256), (4095, 4094)):
        k, i = np.arange(sw)[None, :], np.arange(dw)[:, None]
        wx = np.maximum(0, np.minimum((i + 1) * sw, (k + 1) * dw) - np.maximum(i * sw, k * dw))
        assert (wx.sum(axis=1) == sw).all() and (wx > 0).sum(axis=1).max() <= 17
    # a constant plane stays constant at every ratio, 0 and 255 included: nothing to clamp
    for val in (0, 1, 127, 254, 255):
        for sw, sh, dw, dh in ((128, 96, 64, 48), (100, 52, 36, 20), (128, 96, 8, 6), (97, 61, 96, 60), (128, 96, 128, 96)):
            assert (M.scale_plane(np.full((96, 128), val, np.uint8), 0, 0, sw, sh, dw, dh) == val).all()
    # random planes stay inside the range of their samples
    for sw, sh, dw, dh in ((128, 96, 64, 48), (100, 52, 36, 20), (128, 96, 9, 7)):
        lo = rng.integers(0, 200)
        pl = rng.integers(lo, lo + 56, (96, 128), dtype=np.uint8)
        out = M.scale_plane(pl, 0, 0, sw, sh, dw, dh)
        assert out.min() >= pl.min() and out.max() <= pl.max()


# ---------------------------------------------------------------- slot bytes

# (source w, h) -> (picture w, h), crop
GEOMETRIES = {
    "2to1": ((128, 96), (64, 48), None),
    "3to2": ((96, 72), (64, 48), None),
    "5to3": ((100, 60), (60, 36), None),
    "ragged": ((100, 52), (36, 20), None),
    "one_axis": ((128, 48), (64, 48), None),
    "crop_far_corner": ((100, 80), (64, 48), (36, 32, 64, 48)),
    "16to1": ((256, 64), (16, 4), None),
    "corner_of_34x50_to_2x2": ((34, 50), (2, 2), (2, 18, 32, 32)),
    "crop_and_scale": ((200, 120), (68, 36), (14, 6, 180, 108)),
    "two_tiles_wide": ((300, 160), (150, 80), None),
}
CASES = [("2to1", "packed", "fwd"), ("2to1", "nv12_padded", "rev"), ("3to2", "padded", "fwd"), ("3to2", "nv12", "rev"), ("5to3", "oddbase", "rev"), ("5to3", "separate", "fwd"),
         ("ragged", "oddbase", "fwd"), ("ragged", "nv12_padded", "fwd"), ("ragged", "packed", "rev"), ("one_axis", "separate", "rev"), ("one_axis", "padded", "fwd"),
         ("crop_far_corner", "packed", "fwd"), ("crop_far_corner", "oddbase", "rev"), ("crop_far_corner", "nv12", "fwd"), ("crop_far_corner", "separate", "fwd"),
         ("16to1", "padded", "fwd"), ("16to1", "nv12", "rev"), ("corner_of_34x50_to_2x2", "oddbase", "fwd"), ("corner_of_34x50_to_2x2", "nv12_padded", "rev"),
         ("corner_of_34x50_to_2x2", "packed", "fwd"), ("crop_and_scale", "oddbase", "fwd"), ("crop_and_scale", "nv12_padded", "rev"),
         ("two_tiles_wide", "padded", "rev"), ("two_tiles_wide", "nv12", "fwd")]


@pytest.mark.parametrize("geom,layout,lib", CASES)
def test_slot_holds_the_models_bytes(geom, layout, lib):
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    frames = M.source_clip(sw, sh, 2)
    want = model_frames(frames, sw, sh, dw, dh, crop)
    mem = DevMem(LIBS[lib])
    ce = P.ClipEncoder(dw, dh, 2, gop=30, qp=26, lib=LIBS[lib])
    try:
        feed(ce, mem, frames, sw, sh, layout, crop)
        got = ce.download()
    finally:
        ce.close()
        mem.close()
    assert np.array_equal(got, want), "slot contents differ from the model"


@pytest.mark.parametrize("kind,lib", [("all255", "fwd"), ("random", "rev")])
def test_4096_square_to_256_square_stays_inside_32_bits(kind, lib):
    """16:1 from the largest window: 255 * 2^24 + 2^23 is the largest numerator.  Luma decides (2048 x 2048 chroma is far from the bound);
    compared on the slot only"""
    P = pkg.load_pkg()
    s, d = 4096, 256
    rng = np.random.default_rng(5)
    y = np.full((s, s), 255, np.uint8) if kind == "all255" else rng.integers(0, 256, (s, s), dtype=np.uint8)
    if kind == "random":
        y[: s // 2] |= 0xF0                 # bright half: sums close to the bound next to sums that are not
    u = np.full((s // 2, s // 2), 255, np.uint8) if kind == "all255" else rng.integers(0, 256, (s // 2, s // 2), dtype=np.uint8)
    v = u[::-1].copy()
    want = M.scale_i420(y, u, v, d, d)
    if kind == "all255":
        assert (want == 255).all()
    mem = DevMem(LIBS[lib])
    ce = P.ClipEncoder(d, d, 1, gop=30, qp=26, lib=LIBS[lib])
    try:
        ce.upload_device([[mem.put(y), mem.put(u), mem.put(v)]], "i420", src_size=(s, s))
        got = ce.download()[0]
    finally:
        ce.close()
        mem.close()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- streams


def clip_stream(lib, w, h, n, put, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, lib=lib, **kw)
    try:
        put(ce)
        out, sizes, _ = ce.encode()
        return out, sizes
    finally:
        ce.close()


@pytest.mark.parametrize("geom,n,layout,lib", [("2to1", 4, "padded", "fwd"), ("5to3", 3, "nv12_padded", "rev"), ("crop_far_corner", 3, "oddbase", "fwd")])
def test_streams_match_the_oracle_for_the_models_frames(geom, n, layout, lib):
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, crop)
    want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)
    mem = DevMem(LIBS[lib])
    try:
        got, sizes = clip_stream(LIBS[lib], dw, dh, n, lambda ce: feed(ce, mem, frames, sw, sh, layout, crop), gop=30, qp=26)
        up, up_sizes = clip_stream(LIBS[lib], dw, dh, n, lambda ce: ce.upload(model), gop=30, qp=26)
    finally:
        mem.close()
    assert got == up and sizes == up_sizes, "scaled device input and upload() of the model's frames give different streams"
    assert got == want and sizes == want_sizes, "scaled device input differs from the oracle"


@pytest.mark.parametrize("kw", [dict(), dict(slices=2), dict(kbps=200), dict(denoise=True)], ids=lambda k: "_".join(sorted(k)) or "plain")
def test_per_frame_entry_point_and_options(kw):
    """H264E_encode_device_scaled and the clip encoder with slices, rate control and the denoiser (which reads the slot after the scaler)"""
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), crop = GEOMETRIES["2to1"]
    n = 4
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, crop)
    mem = DevMem(pkg.EMU_LIB)
    try:
        got, sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: feed(ce, mem, frames, sw, sh, "padded", crop), gop=3, qp=28, **kw)
        up, up_sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: ce.upload(model), gop=3, qp=28, **kw)
        a = P.Encoder(dw, dh, gop=3, qp=28, lib=pkg.EMU_LIB, **kw)
        b = P.Encoder(dw, dh, gop=3, qp=28, lib=pkg.EMU_LIB, **kw)
        dev = []
        for f in frames:
            s, fmt = source(mem, f, sw, sh, "nv12_padded")
            dev.append(a.encode_device(s, fmt, src_size=(sw, sh)))
        host = [b.encode(f) for f in model]
        a.close()
        b.close()
    finally:
        mem.close()
    assert got == up and sizes == up_sizes
    assert dev == host
    if "kbps" not in kw and "denoise" not in kw:
        assert got == oracle_lib.encode_clip(model, dw, dh, gop=3, qp=28, **kw)[0]
        assert b"".join(dev) == got


@pytest.mark.parametrize("denoise", [False, True])
def test_bounded_ring_rewind_and_reupload(denoise):
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), crop = GEOMETRIES["3to2"]
    n = 7
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, crop)
    whole, _ = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: ce.upload(model), gop=30, qp=26, denoise=denoise)
    mem = DevMem(pkg.EMU_LIB)
    try:
        ring = P.ClipEncoder(dw, dh, n, gop=30, qp=26, lib=pkg.EMU_LIB, resident=3, denoise=denoise)
        with pytest.raises(P.H264EError):                               # four frames do not fit a ring of three
            feed(ring, mem, frames[:4], sw, sh, "packed", crop)
        parts = []
        for f0 in range(0, n, 3):
            feed(ring, mem, frames[f0:f0 + 3], sw, sh, "padded", crop, first=f0)
            pos, up = C.c_int(), C.c_int()
            ring.L.H264E_clip_position(ring.c, C.byref(pos), C.byref(up))
            assert (pos.value, up.value) == (f0, min(f0 + 3, n))
            parts.append(ring.encode(rewind=(f0 == 0))[0])
        ring.close()
        assert b"".join(parts) == whole
        # whole-clip residency: a rewind keeps the frames; uploading frames 4.. again makes them (and their denoised pictures) new
        ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26, lib=pkg.EMU_LIB, denoise=denoise)
        feed(ce, mem, frames, sw, sh, "nv12", crop)
        first = ce.encode()[0]
        assert ce.encode()[0] == first == whole
        frames2 = frames.copy()
        frames2[4:] = M.source_clip(sw, sh, n, seed=99)[4:]
        feed(ce, mem, frames2[4:], sw, sh, "oddbase", crop, first=4)
        changed = ce.encode()[0]
        ce.close()
    finally:
        mem.close()
    model2 = model_frames(frames2, sw, sh, dw, dh, crop)
    want, _ = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda e: e.upload(model2), gop=30, qp=26, denoise=denoise)
    assert changed == want and changed != first


# ---------------------------------------------------------------- refusals


def test_refusals_leave_the_encoders_usable():
    P = pkg.load_pkg()
    dw, dh, n = 64, 48, 2
    sw, sh = 128, 96
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, None)
    want, _ = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)
    plain = clips.make("scene", dw, dh, n)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26, lib=pkg.EMU_LIB)
    e = P.Encoder(dw, dh, gop=30, qp=26, lib=pkg.EMU_LIB)
    L = ce.L
    try:
        (yp, up, vp), _ = source(mem, frames[0], sw, sh, "separate")
        big = mem.put(np.zeros((8, 4100), np.uint8))                   # rows for the windows that are wide on paper only: all refused before a launch
        rgb = mem.put(np.zeros((sh, sw * 3), np.uint8))

        def refused(planes, strides, win, fmt=P.DEV_FORMAT_I420, pb=0, what=""):
            d = P.DevFrame(format=fmt, pixel_bytes=pb)
            for k, (q, s) in enumerate(zip(planes, strides)):
                d.plane[k], d.stride[k] = q, s
            w = P.DevWindow(*win) if win is not None else None
            assert L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(w) if w is not None else None) == -1, what
            msg = L.H264E_last_error()
            assert msg, what
            data, nb = C.c_void_p(), C.c_int()
            assert L.H264E_encode_device_scaled(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(w) if w is not None else None,
                                                C.byref(data), C.byref(nb)) == P.STATUS_BAD_ARGUMENT, what
            assert L.H264E_last_error(), what
            return msg.decode()

        good_p, good_s = [yp[0], up[0], vp[0]], [yp[1], up[1], vp[1]]
        assert "62" in refused(good_p, good_s, (sw, sh, 0, 0, 62, 96), what="upscale in x")
        assert "46" in refused(good_p, good_s, (sw, sh, 0, 0, 128, 46), what="upscale in y")
        assert "62" in refused(good_p, good_s, (62, sh, 0, 0, 0, 0), what="a whole source narrower than the picture")
        assert "crop_x 3" in refused(good_p, good_s, (sw, sh, 3, 0, 64, 48), what="odd crop_x")
        assert "crop_y 5" in refused(good_p, good_s, (sw, sh, 0, 5, 64, 48), what="odd crop_y")
        assert "65" in refused(good_p, good_s, (sw, sh, 0, 0, 65, 48), what="odd crop_width")
        assert "49" in refused(good_p, good_s, (sw, sh, 0, 0, 64, 49), what="odd crop_height")
        assert "-2" in refused(good_p, good_s, (sw, sh, -2, 0, 64, 48), what="negative crop_x")
        assert "leave the source" in refused(good_p, good_s, (sw, sh, 66, 0, 64, 48), what="window beyond the source, x")
        assert "leave the source" in refused(good_p, good_s, (sw, sh, 0, 50, 64, 48), what="window beyond the source, y")
        assert "1088" in refused([big[0]] * 3, [big[1]] * 3, (4100, 96, 0, 0, 1088, 48), what="17:1")       # 1088 = 17 * 64
        assert "4098" in refused([big[0]] * 3, [big[1]] * 3, (4100, 96, 0, 0, 4098, 48), what="crop_width 4098")
        assert "RGB" in refused([rgb[0]], [rgb[1]], (sw, sh, 0, 0, 0, 0), fmt=P.DEV_FORMAT_RGB, pb=3, what="RGB with a window")
        assert "format" in refused(good_p, good_s, (sw, sh, 0, 0, 0, 0), fmt=9, what="unknown format")
        assert "null" in refused(good_p, good_s, None, what="NULL window")
        assert "NULL" in refused([yp[0], 0, vp[0]], good_s, (sw, sh, 0, 0, 0, 0), what="NULL plane")
        assert "NULL" in refused([0, up[0], vp[0]], good_s, (sw, sh, 0, 0, 0, 0), what="NULL plane")
        assert "stride 127" in refused(good_p, [sw - 1, up[1], vp[1]], (sw, sh, 0, 0, 0, 0), what="short luma stride")
        assert "stride 63" in refused(good_p, [yp[1], up[1], sw // 2 - 1], (sw, sh, 0, 0, 0, 0), what="short chroma stride")
        # ... a stride that holds the window's bytes but not the source's row
        assert "stride 64" in refused(good_p, [64, up[1], vp[1]], (sw, sh, 0, 0, 64, 48), what="stride below the source row")
        assert "stride 126" in refused(good_p[:2], [yp[1], sw - 2], (sw, sh, 0, 0, 0, 0), fmt=P.DEV_FORMAT_NV12, what="short NV12 chroma stride")
        assert L.H264E_clip_upload_device_scaled(ce.c, 0, 1, None, C.byref(P.DevWindow(sw, sh, 0, 0, 0, 0))) == -1 and L.H264E_last_error()
        # the issue's 34 x 50 -> 2 x 2: 17:1 and 25:1
        tiny = P.ClipEncoder(2, 2, 1, gop=30, qp=26, lib=pkg.EMU_LIB)
        src34, fmt = source(mem, M.source_clip(34, 50, 1)[0], 34, 50, "separate")
        with pytest.raises(P.H264EError, match="more than 16 times"):
            tiny.upload_device([src34], fmt, src_size=(34, 50))
        tiny.close()
        # the binding's keywords reach the same checks
        with pytest.raises(P.H264EError, match="crop_x 1"):
            ce.upload_device([[yp, up, vp]], "i420", src_size=(sw, sh), crop=(1, 0, 64, 48))
        with pytest.raises(P.H264EError, match="status 1"):
            e.encode_device([yp, up, vp], "i420", src_size=(sw, sh), crop=(0, 0, 64, 50 + 48))
        pos, upl = C.c_int(), C.c_int()
        L.H264E_clip_position(ce.c, C.byref(pos), C.byref(upl))
        assert (pos.value, upl.value) == (0, 0)                         # nothing was counted
        # a plain encode on the same encoders, then a scaled one
        ce.upload(plain)
        assert ce.encode()[0] == oracle_lib.encode_clip(plain, dw, dh, gop=30, qp=26)[0]
        assert b"".join(e.encode(f) for f in plain) == oracle_lib.encode_clip(plain, dw, dh, gop=30, qp=26)[0]
        feed(ce, mem, frames, sw, sh, "separate", None)
        assert ce.encode()[0] == want
    finally:
        ce.close()
        e.close()
        mem.close()


def test_struct_mirror_and_exports():
    P = pkg.load_pkg()
    assert C.sizeof(P.DevWindow) == 24 and P.DevWindow.crop_width.offset == 16
    for lib in LIBS.values():
        L = P.load(lib)
        assert L.H264E_struct_size(2) == C.sizeof(P.DevFrame) == 56 and L.H264E_struct_size(3) == -1
        assert L.H264E_clip_upload_device_scaled and L.H264E_encode_device_scaled


# ---------------------------------------------------------------- ladder


def test_ladder_gives_each_rung_the_stream_of_a_standalone_encoder():
    P = pkg.load_pkg()
    sw, sh, n = 128, 96, 4
    frames = M.source_clip(sw, sh, n)
    rungs = [(64, 48, dict(qp=26)), (64, 48, dict(qp=34)), (32, 24, dict(qp=28, gop=2))]
    mem = DevMem(pkg.EMU_LIB)
    try:
        srcs = [source(mem, f, sw, sh, "padded")[0] for f in frames]
        got = P.encode_ladder(srcs, "i420", (sw, sh), rungs, gop=30, lib=pkg.EMU_LIB)
    finally:
        mem.close()
    assert len(got) == len(rungs)
    for (w, h, opts), (out, sizes, _) in zip(rungs, got):
        model = model_frames(frames, sw, sh, w, h, None)
        want, want_sizes = clip_stream(pkg.EMU_LIB, w, h, n, lambda ce: ce.upload(model), **dict(dict(gop=30), **opts))
        assert (out, sizes) == (want, want_sizes)
        assert out == oracle_lib.encode_clip(model, w, h, **dict(dict(gop=30), **opts))[0]
