"""CPU: device-resident input (H264E_clip_upload_device / H264E_encode_device, enc_ingest.h) in the lane-loop emulation of the kernels
(tests/emu).  The emulation's "device" memory is what H264E_dev_malloc hands out -- its global-memory accessors abort on any other
address -- so every source frame here is copied into such memory first.

  - I420 from the device gives the oracle's stream and the stream of upload() of the same clip: contiguous, padded and separately
    allocated planes, both encoders, slices / rate control / bounded ring / denoiser / encode_multi, tiny pictures against the reference's
    recorded streams (tests/golden/geometry.json);
  - NV12 and RGB (3 and 4 bytes per pixel) give the stream of upload(model(frames)) and leave exactly the model's bytes in the input
    slots (tests/ingest_model.py);
  - what is refused is refused with an error code, and the encoder goes on working."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import clips
import ingest_model as M
import oracle_lib
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GEOMETRY = {g["name"]: g for g in json.load(open(os.path.join(HERE, "golden", "geometry.json")))}
TINY = ["ramp_2x2_qp26", "ramp_4x4_gop1", "ramp_2x2_kbps50", "ramp_6x6_kbps50", "noise_14x10_qp26", "ramp_18x18_qp10", "noise_34x50_qp51", "ramp_34x50_thr2_kbps200"]
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


class DevArray:
    """a 2-D plane or (h, w, c) pixel array in device memory, described the way GPU array libraries do"""

    def __init__(self, ptr, shape, strides):
        self.ptr, self.shape, self.strides = ptr, tuple(shape), tuple(strides)
        self.__cuda_array_interface__ = dict(shape=self.shape, strides=self.strides, typestr="|u1", data=(ptr, False), version=3)

    def pair(self):
        return (self.ptr, self.strides[0])


class DevMem:
    """device memory of one library (H264E_dev_malloc), freed by close()"""

    def __init__(self, lib):
        self.L = pkg.load_pkg().load(lib)
        self.blocks = []

    def alloc(self, nbytes):
        p = self.L.H264E_dev_malloc(0, nbytes)
        assert p
        self.blocks.append(p)
        return p

    def write(self, ptr, host):
        host = np.ascontiguousarray(host, np.uint8)
        assert self.L.H264E_dev_memcpy(ptr, host.ctypes.data, host.size, 1) == 0

    def put(self, arr, stride=None, offset=0, base=None):
        """rows of `arr` (2-D, or 3-D pixels) `stride` bytes apart, starting `offset` bytes into a fresh block (or at `base`); the
        padding holds 0xA5 and the block ends with the last row's last byte"""
        arr = np.ascontiguousarray(arr, np.uint8)
        rows, rb = arr.shape[0], arr[0].size
        stride = stride or rb
        host = np.full(offset + stride * (rows - 1) + rb, 0xA5, np.uint8)
        for y in range(rows):
            host[offset + y * stride: offset + y * stride + rb] = arr[y].ravel()
        if base is None:
            base = self.alloc(host.size)
        self.write(base, host)
        return DevArray(base + offset, arr.shape, (stride,) + ((arr.shape[2], 1) if arr.ndim == 3 else (1,)))

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def i420_source(mem, frame, w, h, layout):
    y, u, v = M.split(frame, w, h)
    if layout == "packed":                  # one contiguous (h*3/2, w) array
        return mem.put(np.asarray(frame).reshape(h * 3 // 2, w))
    if layout == "packed_pair":             # ... as an explicit (pointer, stride)
        return mem.put(np.asarray(frame).reshape(h * 3 // 2, w)).pair()
    if layout == "padded":                  # odd strides and odd start addresses, as (pointer, stride) pairs
        return [mem.put(y, w + 13, 1).pair(), mem.put(u, w // 2 + 7, 3).pair(), mem.put(v, w // 2 + 1, 2).pair()]
    if layout == "separate":                # three allocations, rows packed
        return [mem.put(y), mem.put(u), mem.put(v)]
    raise ValueError(layout)


def flags(s):
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), speed=int(d.get("--speed", 0)), kbps=int(d.get("--kbps", 0)),
                slices=int(d.get("--threads", 0)))


def clip_stream(lib, w, h, frames, feed, **kw):
    """ClipEncoder stream of len(frames) frames; feed(ce) puts them in"""
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, len(frames), lib=lib, **kw)
    try:
        feed(ce)
        out, sizes, _ = ce.encode()
        return out, sizes, ce.download()
    finally:
        ce.close()


# ---------------------------------------------------------------- I420


@pytest.mark.parametrize("w,h,n,layout,lib", [
    (64, 48, 4, "packed", "fwd"), (64, 48, 4, "padded", "rev"), (64, 48, 3, "separate", "fwd"), (64, 48, 3, "packed_pair", "fwd"),
    (176, 144, 3, "padded", "fwd"), (176, 144, 3, "separate", "rev"),
    (200, 120, 3, "padded", "fwd"), (200, 120, 3, "packed", "rev"),
    (202, 122, 3, "packed", "fwd"), (202, 122, 3, "padded", "rev"), (202, 122, 3, "separate", "fwd"),
])
def test_i420_clip_encoder_matches_oracle_and_upload(w, h, n, layout, lib):
    c = clips.make("scene" if w >= 64 else "ramp", w, h, n)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)
    mem = DevMem(LIBS[lib])
    try:
        got, sizes, slots = clip_stream(LIBS[lib], w, h, c, lambda ce: ce.upload_device([i420_source(mem, f, w, h, layout) for f in c], "i420"), gop=30, qp=26)
        up, _, _ = clip_stream(LIBS[lib], w, h, c, lambda ce: ce.upload(c), gop=30, qp=26)
    finally:
        mem.close()
    assert np.array_equal(slots, c), "the input slots do not hold the source frames"
    assert got == up, "device input and upload() give different streams"
    assert got == want and sizes == want_sizes, "device input differs from the oracle"


@pytest.mark.parametrize("w,h,n,layout,lib", [(64, 48, 4, "padded", "fwd"), (176, 144, 3, "packed", "rev"), (200, 120, 3, "separate", "fwd"), (202, 122, 3, "padded", "fwd")])
def test_i420_per_frame_encoder_matches_oracle_and_encode(w, h, n, layout, lib):
    P = pkg.load_pkg()
    c = clips.make("scene", w, h, n)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)
    mem = DevMem(LIBS[lib])
    a = P.Encoder(w, h, gop=30, qp=26, lib=LIBS[lib])
    b = P.Encoder(w, h, gop=30, qp=26, lib=LIBS[lib])
    try:
        parts = [a.encode_device(i420_source(mem, f, w, h, layout), "i420") for f in c]
        host = [b.encode(f) for f in c]
    finally:
        a.close()
        b.close()
        mem.close()
    assert parts == host
    assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes


@pytest.mark.parametrize("name", TINY)
def test_i420_tiny_pictures_match_reference_streams(name):
    """2x2 ... 34x50 pictures (rows of 1, 2, 3, 7, 9, 17 chroma bytes), padded planes at odd addresses: the reference's recorded streams"""
    P = pkg.load_pkg()
    g = GEOMETRY[name]
    w, h, n = g["w"], g["h"], g["frames"]
    c = clips.make(g["clip"], w, h, n)
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    kw = flags(g["flags"])
    for lib, layout in (("fwd", "padded"), ("rev", "packed")):
        mem = DevMem(LIBS[lib])
        try:
            out, sizes, slots = clip_stream(LIBS[lib], w, h, c, lambda ce: ce.upload_device([i420_source(mem, f, w, h, layout) for f in c], "i420"), **kw)
            e = P.Encoder(w, h, lib=LIBS[lib], **kw)
            parts = [e.encode_device(i420_source(mem, f, w, h, layout), "i420") for f in c]
            e.close()
        finally:
            mem.close()
        assert np.array_equal(slots, c)
        assert sizes == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"]
        assert [len(p) for p in parts] == g["frame_bytes"] and hashlib.md5(b"".join(parts)).hexdigest() == g["md5"]


@pytest.mark.parametrize("kw", [dict(slices=3), dict(kbps=200), dict(denoise=True), dict(slices=2, kbps=300, denoise=True)], ids=lambda k: "_".join(sorted(k)))
def test_i420_options_give_the_upload_stream(kw):
    """slices, rate control and the denoiser pre-pass (which reads the slot after the ingest): both encoders"""
    P = pkg.load_pkg()
    w, h, n = 176, 144, 5
    c = clips.make("scene", w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    try:
        got, sizes, _ = clip_stream(pkg.EMU_LIB, w, h, c, lambda ce: ce.upload_device([i420_source(mem, f, w, h, "padded") for f in c], "i420"), gop=4, qp=28, **kw)
        up, up_sizes, _ = clip_stream(pkg.EMU_LIB, w, h, c, lambda ce: ce.upload(c), gop=4, qp=28, **kw)
        a = P.Encoder(w, h, gop=4, qp=28, lib=pkg.EMU_LIB, **kw)
        b = P.Encoder(w, h, gop=4, qp=28, lib=pkg.EMU_LIB, **kw)
        dev = [a.encode_device(i420_source(mem, f, w, h, "separate"), "i420") for f in c]
        host = [b.encode(f) for f in c]
        a.close()
        b.close()
    finally:
        mem.close()
    assert got == up and sizes == up_sizes
    assert dev == host
    if "kbps" not in kw and "denoise" not in kw:
        assert got == oracle_lib.encode_clip(c, w, h, gop=4, qp=28, **kw)[0]


@pytest.mark.parametrize("denoise", [False, True])
def test_bounded_ring_fed_in_chunks_rewind_and_reupload(denoise):
    P = pkg.load_pkg()
    w, h, n = 64, 48, 8
    c = clips.make("scene", w, h, n)
    whole, _, _ = clip_stream(pkg.EMU_LIB, w, h, c, lambda ce: ce.upload(c), gop=30, qp=26, denoise=denoise)
    mem = DevMem(pkg.EMU_LIB)
    try:
        ring = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB, resident=3, denoise=denoise)
        with pytest.raises(P.H264EError):                               # four frames do not fit a ring of three
            ring.upload_device([i420_source(mem, f, w, h, "packed") for f in c[:4]], "i420")
        parts = []
        for f0 in range(0, n, 3):
            ring.upload_device([i420_source(mem, f, w, h, "padded") for f in c[f0:f0 + 3]], "i420", first=f0)
            pos, up = C.c_int(), C.c_int()
            ring.L.H264E_clip_position(ring.c, C.byref(pos), C.byref(up))
            assert (pos.value, up.value) == (f0, min(f0 + 3, n))         # device frames count as uploaded
            parts.append(ring.encode(rewind=(f0 == 0))[0])
        ring.close()
        assert b"".join(parts) == whole
        # whole-clip residency: rewind keeps the frames; uploading frames 4.. again makes them (and their denoised pictures) new
        ce = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB, denoise=denoise)
        ce.upload_device([i420_source(mem, f, w, h, "separate") for f in c], "i420")
        first = ce.encode()[0]
        assert ce.encode()[0] == first == whole
        c2 = c.copy()
        c2[4:] = clips.make("synth", w, h, n)[4:]
        ce.upload_device([i420_source(mem, f, w, h, "packed") for f in c2[4:]], "i420", first=4)
        changed = ce.encode()[0]
        ce.close()
    finally:
        mem.close()
    want, _, _ = clip_stream(pkg.EMU_LIB, w, h, c2, lambda e: e.upload(c2), gop=30, qp=26, denoise=denoise)
    assert changed == want and changed != first


def test_encode_multi_with_device_input():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 5
    cs = [clips.make(name, w, h, n) for name in ("scene", "synth", "noise")]
    mem = DevMem(pkg.EMU_LIB)
    try:
        encs = [P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB) for _ in cs]
        for e, c, layout in zip(encs, cs, ("padded", "packed", "separate")):
            e.upload_device([i420_source(mem, f, w, h, layout) for f in c], "i420")
        outs = P.ClipEncoder.encode_multi(encs)
        for e in encs:
            e.close()
    finally:
        mem.close()
    for c, (out, sizes, _) in zip(cs, outs):
        assert (out, sizes) == oracle_lib.encode_clip(c, w, h, gop=30, qp=26)


# ---------------------------------------------------------------- NV12 and RGB against the model


def nv12_source(mem, frame, w, h, padded):
    y, uv = M.i420_to_nv12(frame, w, h)
    return (mem.put(y, w + 5, 3), mem.put(uv, w + 9, 1)) if padded else (mem.put(y), mem.put(uv))


@pytest.mark.parametrize("w,h,n,padded,lib", [(64, 48, 3, False, "fwd"), (64, 48, 3, True, "rev"), (202, 122, 3, True, "fwd"), (200, 120, 2, False, "fwd"),
                                              (2, 2, 3, True, "fwd"), (6, 6, 3, False, "rev"), (18, 34, 3, True, "fwd"), (34, 50, 2, True, "rev")])
def test_nv12_matches_model(w, h, n, padded, lib):
    P = pkg.load_pkg()
    c = clips.make("scene" if w >= 64 else "ramp", w, h, n)
    mem = DevMem(LIBS[lib])
    try:
        srcs = [nv12_source(mem, f, w, h, padded) for f in c]
        model = np.stack([M.nv12_to_i420(*M.i420_to_nv12(f, w, h)) for f in c])
        assert np.array_equal(model, c)                                  # de-interleaving undoes the interleaving
        got, sizes, slots = clip_stream(LIBS[lib], w, h, c, lambda ce: ce.upload_device(srcs, "nv12"), gop=30, qp=26)
        up, up_sizes, _ = clip_stream(LIBS[lib], w, h, c, lambda ce: ce.upload(model), gop=30, qp=26)
        e = P.Encoder(w, h, gop=30, qp=26, lib=LIBS[lib])
        parts = [e.encode_device(s, "nv12") for s in srcs]
        e.close()
    finally:
        mem.close()
    assert np.array_equal(slots, model), "slot contents differ from the model"
    assert got == up and sizes == up_sizes
    assert b"".join(parts) == up


@pytest.mark.parametrize("w,h,n,pb,stride_pad,offset,lib", [
    (64, 48, 3, 3, 0, 0, "fwd"), (64, 48, 3, 4, 0, 0, "rev"),
    (64, 48, 2, 3, 1, 1, "rev"),            # 3-byte pixels, odd row stride (193), odd start address
    (202, 122, 2, 3, 1, 0, "fwd"),          # 606-byte rows + 1: odd stride, rows not dword aligned
    (202, 122, 2, 4, 4, 2, "fwd"),          # 4-byte pixels that are not dword aligned
    (200, 120, 2, 4, 0, 0, "fwd"),
    (2, 2, 3, 3, 0, 0, "fwd"), (4, 4, 3, 4, 0, 0, "rev"), (6, 6, 3, 3, 5, 1, "fwd"), (18, 34, 2, 3, 1, 0, "rev"), (34, 50, 2, 4, 0, 0, "fwd"),
])
def test_rgb_matches_model(w, h, n, pb, stride_pad, offset, lib):
    P = pkg.load_pkg()
    rgb = M.rgb_clip(w, h, n, pb)
    model = np.stack([M.rgb_to_i420(f) for f in rgb])
    mem = DevMem(LIBS[lib])
    try:
        srcs = [mem.put(f, w * pb + stride_pad, offset) for f in rgb]
        got, sizes, slots = clip_stream(LIBS[lib], w, h, rgb, lambda ce: ce.upload_device(srcs, "rgb"), gop=30, qp=26)
        up, up_sizes, _ = clip_stream(LIBS[lib], w, h, rgb, lambda ce: ce.upload(model), gop=30, qp=26)
        e = P.Encoder(w, h, gop=30, qp=26, lib=LIBS[lib])
        parts = [e.encode_device(s, "rgb") for s in srcs]
        e.close()
    finally:
        mem.close()
    assert np.array_equal(slots, model), "slot contents differ from the model"
    assert got == up and sizes == up_sizes
    assert b"".join(parts) == up


def test_rgb_model_is_the_stated_definition():
    """the model against the definition written out pixel by pixel in plain Python integers"""
    w, h = 6, 4
    rgb = M.rgb_clip(w, h, 1, 4)[0]
    rgb[0, 0, :3], rgb[0, 1, :3], rgb[1, 0, :3], rgb[1, 1, :3] = (255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 255, 255)
    want = []
    for y in range(h):
        for x in range(w):
            r, g, b = (int(v) for v in rgb[y, x, :3])
            want.append(((66 * r + 129 * g + 25 * b + 128) >> 8) + 16)
    for mat, off in (((-38, -74, 112), 128), ((112, -94, -18), 128)):
        for y in range(0, h, 2):
            for x in range(0, w, 2):
                m = [(int(rgb[y, x, k]) + int(rgb[y, x + 1, k]) + int(rgb[y + 1, x, k]) + int(rgb[y + 1, x + 1, k]) + 2) >> 2 for k in range(3)]
                want.append(((mat[0] * m[0] + mat[1] * m[1] + mat[2] * m[2] + 128) >> 8) + off)
    assert list(M.rgb_to_i420(rgb)) == want
    assert list(M.rgb_to_i420(np.zeros((2, 2, 3), np.uint8))) == [16] * 4 + [128, 128]
    assert list(M.rgb_to_i420(np.full((2, 2, 3), 255, np.uint8))) == [235] * 4 + [128, 128]


# ---------------------------------------------------------------- refusals


def test_refusals_leave_the_encoders_usable():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    c = clips.make("scene", w, h, n)
    want, _ = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)
    mem = DevMem(pkg.EMU_LIB)
    try:
        good = [i420_source(mem, f, w, h, "separate") for f in c]
        yp, up, vp = (a.pair() for a in good[1])
        rgb = mem.put(M.rgb_clip(w, h, 1, 3)[0])
        bad = [
            ([good[0], [yp, (0, w // 2), vp]], "i420"),                 # a NULL plane
            ([good[0], [(0, w), up, vp]], "i420"),
            ([[yp, (up[0], w // 2 - 1), vp]], "i420"),                  # a short stride
            ([[(yp[0], w - 1), up, vp]], "i420"),
            ([(yp, (up[0], w - 2))], "nv12"),
        ]
        ce = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB)
        e = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB)
        for frames, fmt in bad:
            with pytest.raises(P.H264EError):
                ce.upload_device(frames, fmt)
            with pytest.raises(P.H264EError, match="status 1"):
                e.encode_device(frames[-1], fmt)
        # a format and RGB pixel sizes that do not exist, RGB strides below the row bytes (straight through the C structs)
        for fmt, pb, stride in ((7, 3, w * 3), (-1, 0, w * 3), (2, 2, w * 3), (2, 5, w * 5), (2, 0, w * 4), (2, 3, w * 3 - 1), (2, 4, w * 4 - 4)):
            d = P.DevFrame(format=fmt, pixel_bytes=pb)
            d.plane[0], d.stride[0] = rgb.ptr, stride
            assert ce.L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) == -1
            assert ce.L.H264E_last_error()
            data, nb = C.c_void_p(), C.c_int()
            assert e.L.H264E_encode_device(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(data), C.byref(nb)) == P.STATUS_BAD_ARGUMENT
        # frames outside the clip and outside the ring
        with pytest.raises(P.H264EError):
            ce.upload_device(good, "i420", first=1)
        with pytest.raises(P.H264EError):
            ce.upload_device(good[:1], "i420", first=-1)
        pos, upl = C.c_int(), C.c_int()
        ce.L.H264E_clip_position(ce.c, C.byref(pos), C.byref(upl))
        assert (pos.value, upl.value) == (0, 0)                         # nothing was counted
        # P before any key frame: the reference's status, from the device entry point too
        with pytest.raises(P.H264EError, match="status %d" % P.STATUS_BAD_FRAME_TYPE):
            e.encode_device(good[0], "i420", frame_type=P.FRAME_TYPE_P)
        # const_input_flag = 0: the reconstruction cannot go back to the device
        e0 = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB, const_input=0)
        with pytest.raises(P.H264EError, match="status %d" % P.STATUS_BAD_PARAMETER):
            e0.encode_device(good[0], "i420")
        assert e0.encode(c[0].copy()) == oracle_lib.encode_clip(c[:1], w, h, gop=30, qp=26)[0]      # ... and the host path still works
        e0.close()
        # after all that, both encoders give the stream of a fresh one
        ce.upload_device(good, "i420")
        assert ce.encode()[0] == want
        assert b"".join(e.encode_device(f, "i420") for f in good) == want
        ce.close()
        e.close()
    finally:
        mem.close()


def test_struct_mirror_and_exports():
    P = pkg.load_pkg()
    L = P.load(pkg.EMU_LIB)
    assert L.H264E_struct_size(2) == C.sizeof(P.DevFrame) == 56
    assert P.DevFrame.plane.offset == 8 and P.DevFrame.stride.offset == 32 and P.DevFrame.producer_stream.offset == 48
    assert L.H264E_struct_size(3) == -1
