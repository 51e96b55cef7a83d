"""CPU: planar RGB device input (H264E_DEV_FORMAT_RGBP: enc_ingest.h at the picture's size, enc_scale_rgb.h with a window) in the
lane-loop emulation of the kernels (tests/emu), both lane orders.  The emulation's "device" memory is what H264E_dev_malloc hands out --
its global-memory accessors abort on any other address, and every source block here ends with the last byte of the plane's last row, so
a read beyond it would abort the test.

  - the model (tests/rgbp_model.py) is the stated definition and has the properties it promises;
  - the input slots hold exactly the model's bytes, at the picture's size and through a window: separate, padded, odd-address planes and
    one CHW block; ratios 1:1 (a crop) to 16:1, uneven per axis, partial tiles in both axes, the 4096 x 4096 bound;
  - the streams are the oracle's for the model's frames, and those of upload() of the model's frames, through both entry points and with
    slices, rate control, a bounded ring, the denoiser and the scene-cut detector;
  - what is refused is refused with a message that names the value, and the encoder goes on working;
  - encode_ladder gives per rung the stream of a standalone encoder.

Everything is integer arithmetic: every comparison is byte equality."""
import os
import subprocess

import numpy as np
import pytest

import ingest_model
import oracle_lib
import pkg
import rgbp_model as M
import scale_model

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


class DevArray:
    """an array in device memory, described the way GPU array libraries do"""

    def __init__(self, ptr, shape, strides, typestr="|u1"):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), strides=tuple(strides), typestr=typestr, data=(ptr, False), version=3)


class DevMem:
    """device memory of one library (H264E_dev_malloc), freed by close()"""

    def __init__(self, lib):
        self.L = pkg.load_pkg().load(lib)
        self.blocks = []

    def _block(self, host):
        base = self.L.H264E_dev_malloc(0, host.size)
        assert base
        self.blocks.append(base)
        assert self.L.H264E_dev_memcpy(base, host.ctypes.data, host.size, 1) == 0
        return base

    def put(self, arr, stride=None, offset=0):
        """rows of the 2-D `arr` `stride` bytes apart, starting `offset` bytes into a fresh block, as a (pointer, stride) pair; the
        padding holds 0xA5 and the block ends with the last row's last byte"""
        arr = np.ascontiguousarray(arr, np.uint8)
        rows, rb = arr.shape
        stride = stride or rb
        host = np.full(offset + stride * (rows - 1) + rb, 0xA5, np.uint8)
        for y in range(rows):
            host[offset + y * stride: offset + y * stride + rb] = arr[y]
        return (self._block(host) + offset, stride)

    def put_chw(self, chw, stride=None, plane_stride=None, offset=0):
        """the (3, h, w) `chw` as ONE block described as a (3, h, w) array: rows `stride`, planes `plane_stride` bytes apart; the block
        ends with the last byte of the last plane's last row"""
        chw = np.ascontiguousarray(chw, np.uint8)
        _, rows, rb = chw.shape
        stride = stride or rb
        plane_stride = plane_stride or stride * rows
        host = np.full(offset + 2 * plane_stride + stride * (rows - 1) + rb, 0xA5, np.uint8)
        for c in range(3):
            for y in range(rows):
                o = offset + c * plane_stride + y * stride
                host[o: o + rb] = chw[c, y]
        return DevArray(self._block(host) + offset, chw.shape, (plane_stride, stride, 1))

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def source(mem, chw, layout):
    """what upload_device(..., "rgbp") takes for one (3, h, w) frame"""
    w = chw.shape[2]
    if layout == "separate":                # three allocations, rows packed
        return [mem.put(chw[0]), mem.put(chw[1]), mem.put(chw[2])]
    if layout == "padded":                  # odd strides and odd start addresses per plane
        return [mem.put(chw[0], w + 13, 1), mem.put(chw[1], w + 7, 3), mem.put(chw[2], w + 1, 2)]
    if layout == "chw":                     # one contiguous CHW block
        return mem.put_chw(chw)
    if layout == "chw_padded":              # ... with padded rows, planes an odd number of bytes apart, at an odd address
        return mem.put_chw(chw, w + 5, (w + 5) * chw.shape[1] + 3, 1)
    raise ValueError(layout)


def feed(ce, mem, frames, layout, src_size=None, crop=None, first=0):
    ce.upload_device([source(mem, f, layout) for f in frames], "rgbp", first=first, src_size=src_size, crop=crop)


def clip_stream(lib, w, h, n, put, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, lib=lib, **kw)
    try:
        put(ce)
        out, sizes, _ = ce.encode()
        return out, sizes
    finally:
        ce.close()


# ---------------------------------------------------------------- the model


def test_model_is_the_stated_definition():
    """a 6 x 4 window at (2, 2) of a 10 x 8 source -> 4 x 2, pixel by pixel in plain Python integers: the area filter per channel, rounded,
    then Y per pixel and U, V from the rounded 2 x 2 mean of the rounded samples"""
    H, W, cx, cy, sw, sh, dw, dh = 8, 10, 2, 2, 6, 4, 4, 2
    src = M.noisy_clip(W, H, 1)[0]
    rgb = [[[0] * dw for _ in range(dh)] for _ in range(3)]
    for c in range(3):
        for j in range(dh):
            for i in range(dw):
                acc = 0
                for l in range(sh):
                    wy = max(0, min((j + 1) * sh, (l + 1) * dh) - max(j * sh, l * dh))
                    for k in range(sw):
                        wx = max(0, min((i + 1) * sw, (k + 1) * dw) - max(i * sw, k * dw))
                        acc += wy * wx * int(src[c, cy + l, cx + k])
                rgb[c][j][i] = (acc + ((sw * sh) >> 1)) // (sw * sh)
    want = [((66 * rgb[0][j][i] + 129 * rgb[1][j][i] + 25 * rgb[2][j][i] + 128) >> 8) + 16 for j in range(dh) for i in range(dw)]
    for mat in ((-38, -74, 112), (112, -94, -18)):
        for j in range(0, dh, 2):
            for i in range(0, dw, 2):
                m = [(rgb[c][j][i] + rgb[c][j][i + 1] + rgb[c][j + 1][i] + rgb[c][j + 1][i + 1] + 2) >> 2 for c in range(3)]
                want.append(((mat[0] * m[0] + mat[1] * m[1] + mat[2] * m[2] + 128) >> 8) + 128)
    assert list(M.scale_to_i420(src, dw, dh, (cx, cy, sw, sh))) == want


def test_model_properties():
    w, h = 64, 48
    hwc = ingest_model.rgb_clip(w, h, 2, 3)
    chw = M.clip(w, h, 2)
    # planar is what interleaved RGB gives for the same pixels
    for t in range(2):
        assert np.array_equal(chw[t], hwc[t].transpose(2, 0, 1))
        assert np.array_equal(M.to_i420(chw[t]), ingest_model.rgb_to_i420(hwc[t]))
    # S == D is the plain conversion of the cropped region
    big = M.noisy_clip(128, 96, 1)[0]
    assert np.array_equal(M.scale_to_i420(big, w, h, (64, 48, w, h)), M.to_i420(big[:, 48:96, 64:128]))
    assert np.array_equal(M.scale_to_i420(big, 128, 96), M.to_i420(big))
    # a constant colour stays that colour's Y, U, V through any ratio
    for colour in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255), (17, 200, 99)):
        const = np.empty((3, 96, 128), np.uint8)
        for c in range(3):
            const[c] = colour[c]
        y, u, v = (int(x) for x in M.to_i420(const[:, :2, :2])[[0, 4, 5]])
        for (sw, sh), (dw, dh) in (((128, 96), (64, 48)), ((100, 52), (36, 20)), ((128, 96), (8, 6)), ((128, 96), (128, 96))):
            out = M.scale_to_i420(const, dw, dh, (0, 0, sw, sh))
            assert (out[: dw * dh] == y).all() and (out[dw * dh: dw * dh * 5 // 4] == u).all() and (out[dw * dh * 5 // 4:] == v).all()
    assert list(M.to_i420(np.full((3, 2, 2), 255, np.uint8))) == [235] * 4 + [128, 128]


# ---------------------------------------------------------------- slot bytes, at the picture's size

PLAIN = [(2, 2, "separate", "fwd"), (2, 2, "chw_padded", "rev"),       # 6-byte frames: the second frame's slot is not dword aligned
         (202, 122, "separate", "fwd"), (202, 122, "padded", "rev"),   # 101-byte chroma rows, a ragged last group
         (64, 48, "padded", "fwd"), (64, 48, "chw", "rev"), (64, 48, "chw_padded", "fwd"), (64, 48, "chw", "fwd")]


@pytest.mark.parametrize("w,h,layout,lib", PLAIN)
def test_plain_slot_holds_the_models_bytes(w, h, layout, lib):
    P = pkg.load_pkg()
    n = 3
    frames = M.clip(w, h, n)
    want = np.stack([M.to_i420(f) for f in frames])
    mem = DevMem(LIBS[lib])
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=LIBS[lib])
    try:
        feed(ce, mem, frames, layout)
        got = ce.download()
    finally:
        ce.close()
        mem.close()
    assert np.array_equal(got, want), "slot contents differ from the model"


def test_planar_equals_packed_rgb_of_the_same_image():
    """byte for byte what H264E_DEV_FORMAT_RGB leaves in the slot for the same pixels"""
    P = pkg.load_pkg()
    w, h, n = 64, 48, 2
    hwc = ingest_model.rgb_clip(w, h, n, 3)
    mem = DevMem(pkg.EMU_LIB)
    a = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB)
    b = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB)
    try:
        feed(a, mem, M.clip(w, h, n), "padded")
        b.upload_device([DevArray(mem.put(f.reshape(h, w * 3))[0], (h, w, 3), (w * 3, 3, 1)) for f in hwc], "rgb")
        assert np.array_equal(a.download(), b.download())
    finally:
        a.close()
        b.close()
        mem.close()


# ---------------------------------------------------------------- slot bytes, through a window

# (source w, h) -> (picture w, h), crop
GEOMETRIES = {
    "2to1": ((128, 96), (64, 48), None),
    "5to3": ((160, 80), (96, 48), None),
    "crop_far_corner": ((128, 96), (64, 48), (64, 48, 64, 48)),
    "16to1": ((32, 32), (2, 2), None),
    "partial_tiles": ((200, 102), (80, 34), None),                      # 80 = 64 + 16 columns; th = 26, so row tiles of 26 and 8
    "crop_and_scale": ((200, 120), (68, 36), (14, 6, 180, 108)),
}
SCALED = [("2to1", "separate", "fwd"), ("2to1", "chw", "rev"), ("5to3", "padded", "rev"), ("5to3", "chw_padded", "fwd"),
          ("crop_far_corner", "separate", "fwd"), ("crop_far_corner", "chw", "rev"), ("16to1", "padded", "fwd"), ("16to1", "separate", "rev"),
          ("partial_tiles", "separate", "fwd"), ("partial_tiles", "padded", "rev"), ("crop_and_scale", "padded", "fwd"), ("crop_and_scale", "chw_padded", "rev")]


@pytest.mark.parametrize("geom,layout,lib", SCALED)
def test_scaled_slot_holds_the_models_bytes(geom, layout, lib):
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    frames = M.noisy_clip(sw, sh, 2)
    want = np.stack([M.scale_to_i420(f, dw, dh, crop) for f in frames])
    mem = DevMem(LIBS[lib])
    ce = P.ClipEncoder(dw, dh, 2, gop=30, qp=26, lib=LIBS[lib])
    try:
        feed(ce, mem, frames, layout, (sw, sh), crop)
        got = ce.download()
    finally:
        ce.close()
        mem.close()
    assert np.array_equal(got, want), "slot contents differ from the model"
    if geom == "crop_far_corner":           # a pure crop is the plain ingest of the cropped region
        assert np.array_equal(want, np.stack([M.to_i420(f[:, 48:, 64:]) for f in frames]))


def test_4096_square_to_256_square_all_255():
    """16:1 from the largest window, every channel at the bound of the 32-bit sums: Y 235, U = V = 128.  One plane serves as R, G and B"""
    P = pkg.load_pkg()
    s, d = 4096, 256
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(d, d, 1, gop=30, qp=26, lib=pkg.EMU_LIB)
    try:
        white = mem.put(np.full((s, s), 255, np.uint8))
        ce.upload_device([[white, white, white]], "rgbp", src_size=(s, s))
        got = ce.download()[0]
    finally:
        ce.close()
        mem.close()
    assert (got[: d * d] == 235).all() and (got[d * d:] == 128).all()


# ---------------------------------------------------------------- streams

STREAMS = {"plain": ((64, 48), (64, 48), None), "scaled": ((128, 96), (64, 48), None), "cropped": ((128, 96), (64, 48), (32, 24, 96, 72))}


def stream_case(name, n):
    (sw, sh), (dw, dh), crop = STREAMS[name]
    frames = M.noisy_clip(sw, sh, n)
    src_size = None if name == "plain" else (sw, sh)
    model = np.stack([M.to_i420(f) if name == "plain" else M.scale_to_i420(f, dw, dh, crop) for f in frames])
    return frames, model, dw, dh, src_size, crop


@pytest.mark.parametrize("name,n,layout,lib", [("plain", 4, "padded", "fwd"), ("plain", 3, "chw", "rev"), ("scaled", 4, "chw_padded", "fwd"),
                                               ("scaled", 3, "separate", "rev"), ("cropped", 3, "padded", "fwd")])
def test_streams_match_the_oracle_for_the_models_frames(name, n, layout, lib):
    P = pkg.load_pkg()
    frames, model, dw, dh, src_size, crop = stream_case(name, n)
    want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)
    mem = DevMem(LIBS[lib])
    try:
        got, sizes = clip_stream(LIBS[lib], dw, dh, n, lambda ce: feed(ce, mem, frames, layout, src_size, crop), gop=30, qp=26)
        up, up_sizes = clip_stream(LIBS[lib], dw, dh, n, lambda ce: ce.upload(model), gop=30, qp=26)
        e = P.Encoder(dw, dh, gop=30, qp=26, lib=LIBS[lib])
        parts = [e.encode_device(source(mem, f, layout), "rgbp", src_size=src_size, crop=crop) for f in frames]
        e.close()
    finally:
        mem.close()
    assert got == up and sizes == up_sizes, "planar RGB device input and upload() of the model's frames give different streams"
    assert got == want and sizes == want_sizes, "planar RGB device input differs from the oracle"
    assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes


@pytest.mark.parametrize("name", ["plain", "scaled"])
@pytest.mark.parametrize("kw", [dict(slices=2), dict(kbps=200), dict(denoise=True)], ids=lambda k: "_".join(sorted(k)))
def test_both_entry_points_with_options(name, kw):
    """slices, rate control and the denoiser (which reads the slot after the ingest / the scaler): both encoders"""
    P = pkg.load_pkg()
    n = 4
    frames, model, dw, dh, src_size, crop = stream_case(name, n)
    mem = DevMem(pkg.EMU_LIB)
    try:
        got, sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: feed(ce, mem, frames, "padded", src_size, crop), gop=3, qp=28, **kw)
        up, up_sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: ce.upload(model), gop=3, qp=28, **kw)
        a = P.Encoder(dw, dh, gop=3, qp=28, lib=pkg.EMU_LIB, **kw)
        b = P.Encoder(dw, dh, gop=3, qp=28, lib=pkg.EMU_LIB, **kw)
        dev = [a.encode_device(source(mem, f, "chw"), "rgbp", src_size=src_size, crop=crop) for f in frames]
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


@pytest.mark.parametrize("name", ["plain", "scaled"])
def test_scenecut_and_bounded_ring(name):
    """the scene-cut detector reads the slots the kernels wrote; a ring of three slots is fed in chunks"""
    P = pkg.load_pkg()
    n = 4
    frames, model, dw, dh, src_size, crop = stream_case(name, n)
    frames[2:] = 255 - frames[2:]                                       # a cut in front of frame 2
    model = np.stack([M.to_i420(f) if src_size is None else M.scale_to_i420(f, dw, dh, crop) for f in frames])
    mem = DevMem(pkg.EMU_LIB)
    try:
        for kw in (dict(scenecut=128), dict()):
            whole, whole_sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: ce.upload(model), gop=30, qp=26, **kw)
            got, sizes = clip_stream(pkg.EMU_LIB, dw, dh, n, lambda ce: feed(ce, mem, frames, "separate", src_size, crop), gop=30, qp=26, **kw)
            assert (got, sizes) == (whole, whole_sizes)
            ring = P.ClipEncoder(dw, dh, n, gop=30, qp=26, lib=pkg.EMU_LIB, resident=3, **kw)
            with pytest.raises(P.H264EError):                           # four frames do not fit a ring of three
                feed(ring, mem, frames, "chw", src_size, crop)
            parts = []
            for f0 in range(0, n, 3):
                feed(ring, mem, frames[f0:f0 + 3], "chw_padded", src_size, crop, first=f0)
                parts.append(ring.encode(rewind=(f0 == 0))[0])
            ring.close()
            assert b"".join(parts) == whole
        assert whole == oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)[0]
    finally:
        mem.close()


# ---------------------------------------------------------------- refusals


def test_refusals_name_the_value_and_leave_the_encoders_usable():
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), n = (128, 96), (64, 48), 2
    big = M.noisy_clip(sw, sh, n)
    small = M.noisy_clip(dw, dh, n)
    want_scaled = oracle_lib.encode_clip(np.stack([M.scale_to_i420(f, dw, dh) for f in big]), dw, dh, gop=30, qp=26)[0]
    want_plain = oracle_lib.encode_clip(np.stack([M.to_i420(f) for f in small]), dw, dh, gop=30, qp=26)[0]
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26, lib=pkg.EMU_LIB)
    try:
        r, g, b = source(mem, big[0], "separate")
        pr, pg, pb = source(mem, small[0], "separate")
        wide = mem.put(np.zeros((8, 4100), np.uint8))                   # rows for a window that is wide on paper only: refused before a launch
        whole = dict(src_size=(sw, sh))
        cases = [
            # at the picture's size
            ([pr, (0, dw), pb], {}, "plane 1 is NULL"),
            ([pr, pg, (pb[0], dw - 1)], {}, "stride 63 of plane 2"),
            # through a window
            ([(0, sw), g, b], whole, "plane 0 is NULL"),
            ([r, (g[0], sw - 1), b], whole, "stride 127 of plane 1"),
            ([r, g, (b[0], 64)], dict(src_size=(sw, sh), crop=(0, 0, 64, 48)), "stride 64 of plane 2"),    # holds the window's bytes, not the source's row
            ([r, g, b], dict(src_size=(sw, sh), crop=(66, 0, 64, 48)), "window columns 66..129 leave the source's 128"),
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 50, 64, 48)), "window rows 50..97 leave the source's 96"),
            ([r, g, b], dict(src_size=(sw, sh), crop=(3, 0, 64, 48)), "crop_x 3"),
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 5, 64, 48)), "crop_y 5"),
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 0, 65, 48)), "window width 65"),
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 0, 64, 49)), "window height 49"),
            ([wide] * 3, dict(src_size=(4100, 96), crop=(0, 0, 1088, 48)), "window width 1088 is more than 16 times"),     # 17:1
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 0, 62, 96)), "window width 62 below the picture's 64"),           # upscaling
            ([r, g, b], dict(src_size=(sw, sh), crop=(0, 0, 128, 46)), "window height 46 below the picture's 48"),
            # not uint8: float and signed samples, as a CHW array and as a plane
            (DevArray(pr[0], (3, dh, dw), (dw * dh * 4, dw * 4, 4), "<f4"), {}, "uint8 samples, not <f4"),
            ([r, DevArray(g[0], (sh, sw), (sw, 1), "|i1"), b], whole, r"uint8 samples, not \|i1"),
            # a CHW array of another size, and one whose elements are not next to each other
            (DevArray(pr[0], (3, dh, dw // 2), (dw * dh, dw, 1)), {}, "planar RGB must be a"),
            (DevArray(pr[0], (3, dh, dw), (1, dw * 3, 3)), {}, "planar RGB must be a"),
        ]
        for frame, kw, msg in cases:
            with pytest.raises(P.H264EError, match=msg):
                ce.upload_device([frame], "rgbp", **kw)
            e = P.Encoder(dw, dh, gop=30, qp=26, lib=pkg.EMU_LIB)
            with pytest.raises(P.H264EError, match=msg):                # (a refusal by the library comes as "... status 1: <its message>")
                e.encode_device(frame, "rgbp", **kw)
            # ... and the next frames are taken: the stream of a fresh encoder, from both
            if kw:
                feed(ce, mem, big, "padded", (sw, sh))
                parts = [e.encode_device(source(mem, f, "chw"), "rgbp", src_size=(sw, sh)) for f in big]
            else:
                feed(ce, mem, small, "padded")
                parts = [e.encode_device(source(mem, f, "chw"), "rgbp") for f in small]
            e.close()
            assert ce.encode()[0] == (want_scaled if kw else want_plain), msg
            assert b"".join(parts) == (want_scaled if kw else want_plain), msg
    finally:
        ce.close()
        mem.close()


def test_packed_rgb_with_a_window_stays_refused_and_unknown_formats_too():
    P = pkg.load_pkg()
    assert P.DEV_FORMAT_RGBP == 3
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(64, 48, 1, gop=30, qp=26, lib=pkg.EMU_LIB)
    try:
        rgb = mem.put(np.zeros((96, 128 * 3), np.uint8))
        with pytest.raises(P.H264EError, match="RGB"):
            ce.upload_device([DevArray(rgb[0], (96, 128, 3), (128 * 3, 3, 1))], "rgb", src_size=(128, 96))
        for fmt in (4, 7, 9, -1):
            with pytest.raises(P.H264EError, match="unknown format"):
                ce.upload_device([[rgb, rgb, rgb]], fmt)
    finally:
        ce.close()
        mem.close()


# ---------------------------------------------------------------- ladder


def test_ladder_gives_each_rung_the_stream_of_a_standalone_encoder():
    """the source's own size (the plain ingest), two rungs of one size (encoded together) and a smaller one, from the same CHW frames"""
    P = pkg.load_pkg()
    sw, sh, n = 128, 96, 3
    frames = M.noisy_clip(sw, sh, n)
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26)), (64, 48, dict(qp=34)), (32, 24, dict(qp=28, gop=2))]
    mem = DevMem(pkg.EMU_LIB)
    try:
        got = P.encode_ladder([source(mem, f, "chw_padded") for f in frames], "rgbp", (sw, sh), rungs, gop=30, lib=pkg.EMU_LIB)
    finally:
        mem.close()
    assert len(got) == len(rungs)
    for (w, h, opts), (out, sizes, _) in zip(rungs, got):
        model = np.stack([M.scale_to_i420(f, w, h) for f in frames])
        want, want_sizes = clip_stream(pkg.EMU_LIB, w, h, n, lambda ce: ce.upload(model), **dict(dict(gop=30), **opts))
        assert (out, sizes) == (want, want_sizes)
        assert out == oracle_lib.encode_clip(model, w, h, **dict(dict(gop=30), **opts))[0]
