"""CPU: device-resident output (H264E_clip_read_recon_device / H264E_read_recon_device: enc_egress.h) in the lane-loop emulation of the
kernels (tests/emu), both lane orders.  The emulation's "device" memory is what H264E_dev_malloc hands out -- its global-memory accessors
abort on any other address.  Every destination lies in blocks pre-filled with a sentinel, a few bytes larger than the planes: whatever
the rows do not cover must still hold the sentinel afterwards.

  - the destination holds exactly what the model (tests/egress_model.py) makes of read_recon(frame): I420, NV12, RGB of 3 and 4 bytes and
    planar RGB, every colour setting, plain, cropped and tiny pictures, through the clip encoder and the frame-at-a-time encoder;
  - layouts: a packed I420 array, a CHW block, a CHW slice of a larger block, separate planes, odd addresses with odd strides;
  - the window of frames is read_recon's, every refusal with a text;
  - bad arguments are refused with a message that names the value and leave the destination untouched.

Everything is integer arithmetic: every comparison is byte equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clips
import egress_model as EM
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}
SENTINEL, GUARD = 0xA5, 16
COLORS = [None, "bt709", "bt601-full", "bt709-full"]
# (format, pixel_bytes): what a destination can be
KINDS = [("i420", 0), ("nv12", 0), ("rgb", 3), ("rgb", 4), ("rgbp", 0)]
LAYOUTS = {"i420": ["one", "separate", "odd"], "nv12": ["separate", "odd"], "rgb": ["one", "odd"], "rgbp": ["one", "slice", "separate", "odd"]}
# width, height, frames: the first has coded size = picture size, the others are cropped (202 x 2: 101-byte chroma rows)
PICTURES = [(64, 48, 3), (18, 18, 2), (2, 160, 2), (202, 2, 2), (2, 2, 2)]
GOP, QP = 30, 26


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def coded(v):
    return (v + 15) // 16 * 16


class DevArray:
    """an array in device memory, described the way GPU array libraries do"""

    def __init__(self, ptr, shape, strides, typestr="|u1"):
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


def plane_sizes(fmt, pb, w, h):
    """(rows, row bytes) of every plane of a destination"""
    return {"i420": [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "nv12": [(h, w), (h // 2, w)], "rgb": [(h, w * pb)], "rgbp": [(h, w)] * 3}[fmt]


class Dest:
    """a destination in sentinel-filled device memory: `out` is what read_recon_device takes; result() reads it back in the model's
    shape and asserts that every byte outside the rows still holds the sentinel"""

    def __init__(self, mem, fmt, pb, w, h, layout):
        self.mem, self.fmt, self.pb, self.w, self.h = mem, fmt, pb, w, h
        sizes = plane_sizes(fmt, pb, w, h)
        self.blocks, self.planes = [], []           # (pointer, bytes); (block index, offset, stride, rows, row bytes)
        if layout in ("one", "slice"):              # every plane behind the one before it, rows packed; "slice": behind a plane that is not ours
            lead = GUARD + (h * w if layout == "slice" else 0)
            at = lead
            for rows, rb in sizes:
                self.planes.append((0, at, rb, rows, rb))
                at += rows * rb
            self._alloc(at + GUARD)
        else:
            for k, (rows, rb) in enumerate(sizes):
                offset, stride = (GUARD + (1, 3, 2)[k], (rb + 12) | 1) if layout == "odd" else (GUARD, rb)
                self.planes.append((k, offset, stride, rows, rb))
                self._alloc(offset + stride * (rows - 1) + rb + GUARD)
        ptr = [self.blocks[b][0] + off for b, off, _, _, _ in self.planes]
        stride = [p[2] for p in self.planes]
        if fmt == "rgb":
            self.out = DevArray(ptr[0], (h, w, pb), (stride[0], pb, 1))
        elif fmt == "rgbp" and layout in ("one", "slice"):
            self.out = DevArray(ptr[0], (3, h, w), (h * w, w, 1))
        elif fmt == "i420" and layout == "one":
            self.out = (ptr[0], w)
        else:
            self.out = [(p, s) for p, s in zip(ptr, stride)]

    def _alloc(self, n):
        self.blocks.append((self.mem.block(np.full(n, SENTINEL, np.uint8)), n))

    def result(self):
        host = [self.mem.read(p, n) for p, n in self.blocks]
        got = []
        for b, off, stride, rows, rb in self.planes:
            got.append(np.stack([host[b][off + y * stride: off + y * stride + rb] for y in range(rows)]).copy())
            for y in range(rows):
                host[b][off + y * stride: off + y * stride + rb] = SENTINEL
        for b, hb in enumerate(host):
            bad = np.flatnonzero(hb != SENTINEL)
            assert bad.size == 0, "%s: %d bytes outside the rows were written, the first at offset %d of block %d" % (self.fmt, bad.size, bad[0], b)
        if self.fmt == "i420":
            return np.concatenate([g.reshape(-1) for g in got])
        if self.fmt == "nv12":
            return tuple(got)
        if self.fmt == "rgb":
            return got[0].reshape(self.h, self.w, self.pb)
        return np.stack(got)

    def untouched(self):
        return all((self.mem.read(p, n) == SENTINEL).all() for p, n in self.blocks)


def same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    return np.array_equal(got, want)


def check_all(read, mem, packed, w, h, color, kinds=KINDS, what=""):
    """every kind and layout of destination through read(fmt, out) against the model of the packed coded picture"""
    for fmt, pb in kinds:
        want = EM.recon_to(fmt, packed, coded(w), coded(h), w, h, color, pb or 3)
        for layout in LAYOUTS[fmt]:
            d = Dest(mem, fmt, pb, w, h, layout)
            read(fmt, d.out)
            assert same(d.result(), want), "%s %dx%d %s/%d %s colour %s: the destination differs from the model" % (what, w, h, fmt, pb, layout, color)


def clip_frames(w, h, n):
    return clips.ramp(w, h, n) if (w, h) != (64, 48) else clips.make("scene", w, h, n)


# ---------------------------------------------------------------- the clip encoder


@pytest.mark.parametrize("color", COLORS, ids=lambda c: c or "default")
@pytest.mark.parametrize("w,h,n", PICTURES)
def test_clip_destination_holds_the_models_bytes(w, h, n, color):
    P = pkg.load_pkg()
    lib = LIBS["rev" if (PICTURES.index((w, h, n)) + COLORS.index(color)) % 2 else "fwd"]
    # colour only matters for the RGB formats: the copies are checked once per picture
    kinds = KINDS if color is None else [k for k in KINDS if k[0] in ("rgb", "rgbp")]
    mem = DevMem(lib)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=lib, color=color)
    try:
        ce.upload(clip_frames(w, h, n))
        ce.encode()
        for f in range(n):
            packed = ce.read_recon(f)
            check_all(lambda fmt, out: ce.read_recon_device(f, fmt, out=out), mem, packed, w, h, color, kinds, "frame %d" % f)
    finally:
        ce.close()
        mem.close()


def test_clip_recon_is_not_the_input_and_p_frames_differ():
    """the pictures compared above are reconstructions: lossy, and one per frame"""
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    frames = clip_frames(w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=pkg.EMU_LIB)
    try:
        ce.upload(frames)
        ce.encode()
        got = []
        for f in range(n):
            d = Dest(mem, "i420", 0, w, h, "one")
            ce.read_recon_device(f, "i420", out=d.out)
            got.append(d.result())
            assert np.array_equal(got[-1], ce.read_recon(f))
            assert not np.array_equal(got[-1], frames[f])
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    finally:
        ce.close()
        mem.close()


# ---------------------------------------------------------------- the frame-at-a-time encoder


def clip_recons(P, lib, frames, w, h, color=None):
    ce = P.ClipEncoder(w, h, len(frames), gop=GOP, qp=QP, lib=lib, color=color)
    try:
        ce.upload(frames)
        ce.encode()
        return [ce.read_recon(f) for f in range(len(frames))]
    finally:
        ce.close()


@pytest.mark.parametrize("w,h,n,color,lib", [(64, 48, 3, None, "fwd"), (18, 18, 2, "bt709-full", "rev"), (202, 2, 2, "bt709", "fwd"), (2, 2, 2, "bt601-full", "rev")])
def test_per_frame_encoder_after_encode_and_after_encode_device(w, h, n, color, lib):
    """the same stream from the clip encoder gives the pictures to compare with: after every frame, host input and device input"""
    P = pkg.load_pkg()
    frames = clip_frames(w, h, n)
    recons = clip_recons(P, LIBS[lib], frames, w, h, color)
    mem = DevMem(LIBS[lib])
    a = P.Encoder(w, h, gop=GOP, qp=QP, lib=LIBS[lib], color=color)
    b = P.Encoder(w, h, gop=GOP, qp=QP, lib=LIBS[lib], color=color)
    try:
        for f in range(n):
            a.encode(frames[f])
            check_all(lambda fmt, out: a.read_recon_device(fmt, out=out), mem, recons[f], w, h, color, what="encode, frame %d" % f)
            src = (mem.block(frames[f]), w)
            b.encode_device(src, "i420")
            check_all(lambda fmt, out: b.read_recon_device(fmt, out=out), mem, recons[f], w, h, color, what="encode_device, frame %d" % f)
    finally:
        a.close()
        b.close()
        mem.close()


def test_per_frame_i420_equals_what_const_input_0_writes_back():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    frames = clip_frames(w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=GOP, qp=QP, lib=pkg.EMU_LIB, const_input=0)
    try:
        for f in range(n):
            y, u, v = (p.copy() for p in EM.planes(frames[f], w, h, w, h))
            e.encode_planes(y, u, v)
            back = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
            assert not np.array_equal(back, frames[f])
            d = Dest(mem, "i420", 0, w, h, "odd")
            e.read_recon_device("i420", out=d.out)
            assert np.array_equal(d.result(), back), "frame %d" % f
            check_all(lambda fmt, out: e.read_recon_device(fmt, out=out), mem, back, w, h, None, [("rgbp", 0), ("nv12", 0)], "const_input=0, frame %d" % f)
    finally:
        e.close()
        mem.close()


# ---------------------------------------------------------------- the window of frames


def refusal(call):
    P = pkg.load_pkg()
    with pytest.raises(P.H264EError) as ei:
        call()
    return str(ei.value)


def readable(ce, f):
    try:
        ce.read_recon(f)
        return True
    except pkg.load_pkg().H264EError:
        return False


def test_frames_outside_the_window_are_refused_with_text():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 5
    frames = clip_frames(w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=pkg.EMU_LIB, max_chains=2)          # a ring of three pictures: the last two frames stay
    try:
        d = Dest(mem, "rgbp", 0, w, h, "one")
        ce.upload(frames[:3])
        assert "frame 0 has not been encoded" in refusal(lambda: ce.read_recon_device(0, "rgbp", out=d.out))
        ce.encode()
        for f, msg in ((3, "frame 3 has not been encoded"), (7, "frame 7 has not been encoded"), (-1, "frame -1 has not been encoded"), (0, "picture of frame 0 has been overwritten")):
            assert not readable(ce, f)
            assert msg in refusal(lambda: ce.read_recon_device(f, "rgbp", out=d.out))
        assert d.untouched()
        ce.upload(frames[3:], first=3)
        ce.encode(rewind=False)
        for f in range(n + 1):
            assert readable(ce, f) == (f in (3, 4))
            if f in (3, 4):
                check_all(lambda fmt, out: ce.read_recon_device(f, fmt, out=out), mem, ce.read_recon(f), w, h, None, [("rgbp", 0)], "frame %d" % f)
            else:
                assert "frame %d" % f in refusal(lambda: ce.read_recon_device(f, "rgbp", out=d.out))
        assert d.untouched()
    finally:
        ce.close()
        mem.close()


def test_rate_control_keeps_read_recons_floor():
    """with kbps the frames below the floor are refused, exactly those read_recon refuses; the others hold the model's bytes"""
    P = pkg.load_pkg()
    w, h, n = 64, 48, 8
    frames = clips.make("scene", w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=pkg.EMU_LIB, kbps=100)
    try:
        ce.upload(frames)
        ce.encode()
        d = Dest(mem, "rgbp", 0, w, h, "one")
        ok = [readable(ce, f) for f in range(n)]
        assert ok[n - 1] and not all(ok), ok
        for f in range(n):
            if ok[f]:
                check_all(lambda fmt, out: ce.read_recon_device(f, fmt, out=out), mem, ce.read_recon(f), w, h, None, [("rgbp", 0)], "frame %d" % f)
            else:
                assert "frame %d may have been overwritten" % f in refusal(lambda: ce.read_recon_device(f, "rgbp", out=d.out))
        assert d.untouched()
    finally:
        ce.close()
        mem.close()


def test_per_frame_encoder_is_refused_before_its_first_frame():
    P = pkg.load_pkg()
    w, h = 64, 48
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=GOP, qp=QP, lib=pkg.EMU_LIB)
    try:
        d = Dest(mem, "rgbp", 0, w, h, "one")
        assert "no frame has been encoded yet" in refusal(lambda: e.read_recon_device("rgbp", out=d.out))
        assert d.untouched()
        e.encode(clip_frames(w, h, 1)[0])
        e.read_recon_device("rgbp", out=d.out)
        assert not d.untouched()
    finally:
        e.close()
        mem.close()


# ---------------------------------------------------------------- bad arguments


def test_bad_arguments_name_the_value_and_leave_the_destination_untouched():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 2
    frames = clip_frames(w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=GOP, qp=QP, lib=pkg.EMU_LIB)
    try:
        ce.upload(frames)
        ce.encode()
        for f in frames:
            e.encode(f)
        dests = []

        def dest(fmt, pb=0, layout="separate"):
            dests.append(Dest(mem, fmt, pb, w, h, layout))
            return dests[-1]

        planar, i420, nv12 = dest("rgbp").out, dest("i420").out, dest("nv12").out
        rgb5 = dest("rgb", 5, "one").out                                # room for 5-byte pixels, so that nothing but the value is wrong
        cases = [
            ("rgb", rgb5, "RGB pixels of 5 bytes"),
            ("rgbp", [planar[0], (0, w), planar[2]], "plane 1 is NULL"),
            ("i420", [(0, w), i420[1], i420[2]], "plane 0 is NULL"),
            ("nv12", [nv12[0], (0, w)], "plane 1 is NULL"),
            ("rgbp", [planar[0], planar[1], (planar[2][0], w - 1)], "stride 63 of plane 2 is below its 64 row bytes"),
            ("i420", [i420[0], (i420[1][0], w // 2 - 1), i420[2]], "stride 31 of plane 1 is below its 32 row bytes"),
            ("nv12", [nv12[0], (nv12[1][0], w - 1)], "stride 63 of plane 1 is below its 64 row bytes"),
            ("rgb", DevArray(dests[-1].out.__cuda_array_interface__["data"][0], (h, w, 3), (w * 3 - 1, 3, 1)), "stride 191 of plane 0 is below its 192 row bytes"),
        ]
        for fmt, out, msg in cases:
            assert msg in refusal(lambda: ce.read_recon_device(1, fmt, out=out)), msg
            assert msg in refusal(lambda: e.read_recon_device(fmt, out=out)), msg
        # a format the binding does not know either: straight through the C API
        for bad in (7, -1, 4):
            d = P.DevFrame(format=bad, pixel_bytes=3)
            for k in range(3):
                d.plane[k], d.stride[k] = planar[k]
            assert ce.L.H264E_clip_read_recon_device(ce.c, 1, C.byref(d)) == -1
            assert ("unknown format %d" % bad) in ce.L.H264E_last_error().decode()
            assert e.L.H264E_read_recon_device(e.persist, C.byref(d)) == P.STATUS_BAD_ARGUMENT
            assert ("unknown format %d" % bad) in e.L.H264E_last_error().decode()
            assert "unknown format" in refusal(lambda: ce.read_recon_device(1, bad, out=planar))
        assert ce.L.H264E_clip_read_recon_device(ce.c, 1, None) == -1 and "null destination" in ce.L.H264E_last_error().decode()
        assert e.L.H264E_read_recon_device(e.persist, None) == P.STATUS_BAD_ARGUMENT and "null destination" in e.L.H264E_last_error().decode()
        assert all(d.untouched() for d in dests)
        # ... and both go on working
        packed = ce.read_recon(1)
        check_all(lambda fmt, out: ce.read_recon_device(1, fmt, out=out), mem, packed, w, h, None, [("rgbp", 0)])
        check_all(lambda fmt, out: e.read_recon_device(fmt, out=out), mem, packed, w, h, None, [("rgb", 4)])
    finally:
        ce.close()
        e.close()
        mem.close()


def test_recon_out_refuses_an_unknown_format_before_anything_is_allocated():
    P = pkg.load_pkg()
    with pytest.raises(P.H264EError, match="unknown format"):
        P.recon_out("yuy2", 64, 48)
