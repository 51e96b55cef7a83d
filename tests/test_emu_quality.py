"""CPU: the quality metrics (H264E_clip_set_ssim_output / H264E_clip_set_ssd_output / H264E_read_quality / H264E_ssim_planes: enc_ssim.h)
in the lane-loop emulation of the kernels (tests/emu), both lane orders.  tests/ssim_model.py is the definition.

SSIM tolerance (derived in ssim_model.py, not measured): |got - model| <= (N + 8) 2^-52 for a plane of N windows, the model's mean taken with
math.fsum.  The sums of squared differences are integers: equality.  The emulation's "device" memory is what H264E_dev_malloc hands out; the
planes of the plane-pair cases lie a few bytes inside their blocks, the accessors abort on any address outside a block."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import clips
import pkg
import rgbp_model
import scale_model
import ssim_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
GUARD = 16
PLANE_SIZES = [(8, 8), (9, 17), (18, 34), (272, 272)]          # one window; ragged; several windows, odd pitch; more than one tile both ways
CONTENTS = ["noise", "noise_inverse", "0_255", "checker_inverse", "255_255"]
LAYOUTS = ["packed", "padded", "odd"]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def noise(w, h, salt):
    return clips._hash_bytes(w * h, salt).reshape(h, w)


def pair(name, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    chk = (((xx + yy) & 1) * 255).astype(np.uint8)
    return {"noise": (noise(w, h, 1), noise(w, h, 2)), "noise_inverse": (noise(w, h, 1), 255 - noise(w, h, 1)),
            "0_255": (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)), "checker_inverse": (chk, 255 - chk),
            "255_255": (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8))}[name]


class DevArray:
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

    def plane(self, a, layout, k=0):
        """a 2-D array in a block of its own that ends GUARD bytes behind its last row: packed rows at the block's start + GUARD, rows
        padded to a multiple of 4 + 12, or an odd stride at an odd address"""
        h, w = a.shape
        offset, stride = {"packed": (GUARD, w), "padded": (GUARD, (w + 15) // 4 * 4), "odd": (GUARD + (1, 3)[k], (w + 12) | 1)}[layout]
        host = np.full(offset + stride * (h - 1) + w + GUARD, 0xA5, np.uint8)
        for y in range(h):
            host[offset + y * stride: offset + y * stride + w] = a[y]
        return DevArray(self.block(host) + offset, (h, w), (stride, 1))

    def close(self):
        for p in self.blocks:
            self.L.H264E_dev_free(p)
        self.blocks = []


def refusal(f):
    P = pkg.load_pkg()
    with pytest.raises(P.H264EError) as e:
        f()
    return str(e.value)


_plane_values = {}


def plane_value(lib, name, w, h, layout):
    key = (lib, name, w, h, layout)
    if key not in _plane_values:
        P = pkg.load_pkg()
        mem = DevMem(LIBS[lib])
        try:
            a, b = pair(name, w, h)
            _plane_values[key] = P.ssim_planes(mem.plane(a, layout, 0), mem.plane(b, layout, 1), lib=LIBS[lib])
        finally:
            mem.close()
    return _plane_values[key]


_model_values = {}


def model_value(name, w, h):
    if (name, w, h) not in _model_values:
        _model_values[(name, w, h)] = SM.plane(*pair(name, w, h))
    return _model_values[(name, w, h)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("w,h", PLANE_SIZES)
@pytest.mark.parametrize("lib", sorted(LIBS))
def test_plane_pair_matches_the_model(lib, w, h, name, layout):
    got, want = plane_value(lib, name, w, h, layout), model_value(name, w, h)
    print("%s %dx%d %s %s: got %r model %r diff %.3g bound %.3g" % (lib, w, h, name, layout, got, want, abs(got - want), SM.tolerance(w, h)))
    assert abs(got - want) <= SM.tolerance(w, h)
    if name == "255_255":
        assert got == 1.0
    if name == "0_255" and (w, h) == (8, 8):
        assert got == 416 / 266342816


@pytest.mark.parametrize("w,h", PLANE_SIZES)
def test_identical_planes_give_exactly_one_and_lane_orders_agree_bit_for_bit(w, h):
    P = pkg.load_pkg()
    for lib in sorted(LIBS):
        mem = DevMem(LIBS[lib])
        try:
            a = noise(w, h, 9)
            assert P.ssim_planes(mem.plane(a, "odd", 0), mem.plane(a, "padded", 1), lib=LIBS[lib]) == 1.0
        finally:
            mem.close()
    for name in CONTENTS:
        for layout in LAYOUTS:
            assert plane_value("fwd", name, w, h, layout).hex() == plane_value("rev", name, w, h, layout).hex(), (name, layout)
        assert len({plane_value("fwd", name, w, h, layout).hex() for layout in LAYOUTS}) == 1, name      # the layout changes the loads, not the value


def test_plane_pair_refusals_name_the_value():
    P = pkg.load_pkg()
    L = P.load(pkg.EMU_LIB)
    mem = DevMem(pkg.EMU_LIB)
    try:
        a = mem.block(np.zeros(64 * 64, np.uint8))
        out = C.c_double(-5.0)

        def call(pa, sa, pb, sb, w, h, o=out):
            rc = L.H264E_ssim_planes(0, pa, sa, pb, sb, w, h, C.byref(o) if o is not None else None)
            return rc, L.H264E_last_error().decode()

        for args, msg in (((None, 64, a, 64, 64, 64), "null argument"), ((a, 64, None, 64, 64, 64), "null argument"),
                          ((a, 64, a, 64, 7, 64), "width 7 (8 to"), ((a, 64, a, 64, 64, 4), "height 4 (8 to"), ((a, 64, a, 64, 40000, 8), "width 40000"),
                          ((a, 15, a, 64, 16, 16), "stride 15 of plane a is below its 16 row bytes"), ((a, 64, a, -3, 16, 16), "stride -3 of plane b is below its 16 row bytes")):
            rc, err = call(*args)
            assert rc == -1 and msg in err, (args, err)
        assert call(a, 64, a, 64, 64, 64, None) == (-1, "ssim_planes: null argument")
        assert out.value == -5.0
        t = DevArray(a, (16, 16), (16, 1))
        assert "two 2-D uint8 arrays of one shape" in refusal(lambda: P.ssim_planes(t, DevArray(a, (16, 8), (16, 1)), lib=pkg.EMU_LIB))
        assert "8-bit samples" in refusal(lambda: P.ssim_planes(t, DevArray(a, (16, 16), (64, 4), "<f4"), lib=pkg.EMU_LIB))
        assert "height 4" in refusal(lambda: P.ssim_planes(DevArray(a, (4, 16), (16, 1)), DevArray(a, (4, 16), (16, 1)), lib=pkg.EMU_LIB))
    finally:
        mem.close()


# ---- the clip encoder

CLIP_SIZES = [(16, 16, 3), (18, 34, 4), (272, 144, 3)]


def check_frames(ce, frames, w, h, first, ssd, ssim, what, readable_only=False):
    """the metrics of frames first.. against the model applied to the inputs and read_recon"""
    assert ssd.shape == ssim.shape == (ssd.shape[0], 3) and ssd.dtype == np.uint64 and ssim.dtype == np.float64
    checked = 0
    for i in range(ssd.shape[0]):
        f = first + i
        try:
            rec = ce.read_recon(f)
        except pkg.load_pkg().H264EError:
            assert readable_only, "%s: frame %d cannot be read" % (what, f)
            continue
        want = SM.frame(frames[f], rec, w, h)
        assert [int(v) for v in ssd[i]] == SM.frame_ssd(frames[f], rec, w, h), "%s: SSD of frame %d" % (what, f)
        for k in range(3):
            pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
            print("%s frame %d plane %d: got %r model %r diff %.3g bound %.3g" % (what, f, k, ssim[i][k], want[k], abs(ssim[i][k] - want[k]), SM.tolerance(pw, ph)))
            assert abs(ssim[i][k] - want[k]) <= SM.tolerance(pw, ph), "%s: SSIM of frame %d plane %d" % (what, f, k)
        checked += 1
    return checked


@pytest.mark.parametrize("qp", [10, 51])
@pytest.mark.parametrize("content", ["noise", "ramp"])
@pytest.mark.parametrize("w,h,n", CLIP_SIZES)
@pytest.mark.parametrize("lib", sorted(LIBS))
def test_clip_metrics_match_the_model(lib, w, h, n, content, qp):
    P = pkg.load_pkg()
    frames = clips.make(content, w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=qp, lib=LIBS[lib], quality=True)
    try:
        ce.upload(frames)
        out, sizes, _ = ce.encode()
        assert len(sizes) == n
        inputs = ce.download()
        assert (inputs == frames).all()
        ssd, ssim = ce.read_quality()
        assert check_frames(ce, inputs, w, h, 0, ssd, ssim, "%s %dx%d %s qp %d" % (lib, w, h, content, qp)) == n
        if qp == 10 and content == "ramp":
            assert float(ssim.min()) > 0.9
    finally:
        ce.close()


_solo = {}


def solo(lib, w, h, n, content, **kw):
    """(stream, ssd, ssim) of a clip encoded alone with the metrics on"""
    key = (lib, w, h, n, content, tuple(sorted(kw.items())))
    if key not in _solo:
        P = pkg.load_pkg()
        ce = P.ClipEncoder(w, h, n, lib=LIBS[lib], quality=True, **kw)
        try:
            ce.upload(clips.make(content, w, h, n))
            out, _, _ = ce.encode()
            _solo[key] = (out,) + ce.read_quality()
        finally:
            ce.close()
    return _solo[key]


def test_stream_does_not_change_and_the_metrics_can_be_chosen():
    P = pkg.load_pkg()
    w, h, n = 48, 32, 4
    frames = clips.make("scene", w, h, n)
    want = solo("fwd", w, h, n, "scene", gop=30, qp=26)
    for q in (None, dict(ssd=True, ssim=False), dict(ssd=False, ssim=True)):
        ce = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB, quality=q)
        try:
            ce.upload(frames)
            out, _, _ = ce.encode()
            assert out == want[0]
            ssd, ssim = ce.read_quality()
            assert (ssd is None) == (not q or not q["ssd"]) and (ssim is None) == (not q or not q["ssim"])
            if ssd is not None:
                assert (ssd == want[1]).all()
            if ssim is not None:
                assert ssim.tobytes() == want[2].tobytes()
        finally:
            ce.close()


def test_rate_control_hedge_leaves_are_measured_after_their_picture_has_moved():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 8
    frames = clips.make("scene", w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26, lib=pkg.EMU_LIB, kbps=100, quality=True)
    try:
        ce.upload(frames)
        _, sizes, st = ce.encode()
        assert len(sizes) == n
        ssd, ssim = ce.read_quality()
        assert ssd.shape == (n, 3)
        # frames whose pictures the later launches' hedge leaves have overwritten cannot be read back; those that can are checked, the last one always
        assert check_frames(ce, frames, w, h, 0, ssd, ssim, "kbps", readable_only=True) >= 1
        ce.read_recon(n - 1)
        assert (ssim > 0).all() and (ssim <= 1).all() and (ssd[:, 0] > 0).all()
    finally:
        ce.close()
    # frame by frame the same stream has the same pictures: the per-frame encoder's metrics are the clip's, for EVERY frame
    e = P.Encoder(w, h, gop=30, kbps=100, lib=pkg.EMU_LIB)
    try:
        for f in range(n):
            e.encode(frames[f])
            d, s = e.read_quality()
            assert (d == ssd[f]).all() and s.tobytes() == ssim[f].tobytes(), "frame %d" % f
    finally:
        e.close()


def test_denoiser_is_measured_against_the_raw_input():
    P = pkg.load_pkg()
    w, h, n = 48, 32, 4
    frames = clips.noise(w, h, n) // 8 + clips.make("ramp", w, h, n) // 2
    ce = P.ClipEncoder(w, h, n, gop=30, qp=20, lib=pkg.EMU_LIB, denoise=True, quality=True)
    try:
        ce.upload(frames)
        ce.encode()
        ssd, ssim = ce.read_quality()
        assert check_frames(ce, frames, w, h, 0, ssd, ssim, "denoise") == n
    finally:
        ce.close()


def test_two_consecutive_calls_index_from_their_first_frame():
    P = pkg.load_pkg()
    w, h, n = 48, 32, 5
    frames = clips.make("ramp", w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=30, lib=pkg.EMU_LIB, quality=True)
    try:
        ce.upload(frames[:2])
        ce.encode()
        ssd, ssim = ce.read_quality()
        assert ssd.shape == (2, 3) and check_frames(ce, frames, w, h, 0, ssd, ssim, "first call") == 2
        ce.upload(frames[2:], first=2)
        ce.encode(rewind=False)
        ssd, ssim = ce.read_quality()
        assert ssd.shape == (3, 3) and check_frames(ce, frames, w, h, 2, ssd, ssim, "second call") == 3
    finally:
        ce.close()


@pytest.mark.parametrize("lib", sorted(LIBS))
def test_encode_multi_equals_solo_bit_for_bit(lib):
    P = pkg.load_pkg()
    w, h, n = 48, 32, 4
    kw = dict(gop=30, qp=26)
    names = ["scene", "ramp"]
    encs = [P.ClipEncoder(w, h, n, lib=LIBS[lib], quality=True, **kw) for _ in names]
    try:
        for e, name in zip(encs, names):
            e.upload(clips.make(name, w, h, n))
        res = P.ClipEncoder.encode_multi(encs)
        for e, name, r in zip(encs, names, res):
            want = solo(lib, w, h, n, name, **kw)
            ssd, ssim = e.read_quality()
            assert r[0] == want[0] and (ssd == want[1]).all() and ssim.tobytes() == want[2].tobytes(), name
    finally:
        for e in encs:
            e.close()
    assert solo("fwd", w, h, n, "scene", **kw)[2].tobytes() == solo("rev", w, h, n, "scene", **kw)[2].tobytes()


def test_clip_refusals():
    P = pkg.load_pkg()
    for w, h in ((8, 16), (16, 14), (2, 2)):
        ce = P.ClipEncoder(w, h, 2, gop=30, qp=30, lib=pkg.EMU_LIB)
        try:
            assert ("a %d x %d picture has a chroma plane without an 8 x 8 window" % (w, h)) in refusal(lambda: ce.set_quality())
            ce.set_quality(ssim=False)                      # the sums work at every size
            frames = clips.make("ramp", w, h, 2)
            ce.upload(frames)
            ce.encode()
            ssd, ssim = ce.read_quality()
            assert ssim is None and [[int(v) for v in r] for r in ssd] == [SM.frame_ssd(frames[f], ce.read_recon(f), w, h) for f in range(2)]
        finally:
            ce.close()
    L = P.load(pkg.EMU_LIB)
    assert L.H264E_clip_set_ssim_output(None, None) == -1 and "null clip" in L.H264E_last_error().decode()


# ---- the frame-at-a-time encoder

def last_recon(e, mem, w, h):
    """the picture read_recon_device hands out, as packed I420 of the picture's size"""
    n = w * h * 3 // 2
    base = mem.block(np.zeros(n, np.uint8))
    e.read_recon_device("i420", out=(base, w))
    return mem.read(base, n)


def check_last(e, mem, slot, w, h, what):
    """read_quality against the model applied to what lies in the input slot and the last reconstruction"""
    ssd, ssim = e.read_quality()
    rec = last_recon(e, mem, w, h)
    ya, yb = SM.split_i420(slot, w, h), SM.split_i420(rec, w, h)
    assert [int(v) for v in ssd] == [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(ya, yb)], what
    for k in range(3):
        want = SM.plane(ya[k], yb[k])
        print("%s plane %d: got %r model %r diff %.3g bound %.3g" % (what, k, ssim[k], want, abs(ssim[k] - want), SM.tolerance(*ya[k].shape[::-1])))
        assert abs(ssim[k] - want) <= SM.tolerance(*ya[k].shape[::-1]), "%s plane %d" % (what, k)
    return ssd, ssim, rec


@pytest.mark.parametrize("const_input,w,h", [(0, 32, 48), (1, 18, 34)])       # const_input_flag = 0 asks for whole macroblocks, as the reference does
@pytest.mark.parametrize("lib", sorted(LIBS))
def test_per_frame_host_input(lib, const_input, w, h):
    P = pkg.load_pkg()
    n = 3
    frames = clips.make("ramp", w, h, n)
    mem = DevMem(LIBS[lib])
    e = P.Encoder(w, h, gop=30, qp=28, lib=LIBS[lib], const_input=const_input)
    try:
        for f in range(n):
            e.encode(frames[f].copy())
            check_last(e, mem, frames[f], w, h, "%s const_input %d frame %d" % (lib, const_input, f))
        d, s = e.read_quality(ssim=False)
        assert s is None and d is not None
        d, s = e.read_quality(ssd=False)
        assert d is None and s is not None
    finally:
        e.close()
        mem.close()


def test_per_frame_device_rgbp_and_scaled_input():
    P = pkg.load_pkg()
    w, h = 32, 48
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=30, qp=28, lib=pkg.EMU_LIB)
    try:
        chw = rgbp_model.clip(w, h, 1)[0]
        e.encode_device(DevArray(mem.block(chw), (3, h, w), (h * w, w, 1)), "rgbp")
        check_last(e, mem, rgbp_model.to_i420(chw), w, h, "rgbp")
        sw, sh = 80, 112
        src = scale_model.source_clip(sw, sh, 1)[0]
        base = mem.block(src)
        e.encode_device((base, sw), "i420", src_size=(sw, sh))
        check_last(e, mem, scale_model.scale_frame(src, sw, sh, w, h), w, h, "scaled")
    finally:
        e.close()
        mem.close()


def test_transparent_vbv_overflow_frame_is_measured_against_the_unchanged_picture():
    P = pkg.load_pkg()
    w, h = 48, 32
    frames = clips.make("scene", w, h, 3)
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=30, kbps=100, lib=pkg.EMU_LIB)
    try:
        e.encode(frames[0])
        _, _, rec0 = check_last(e, mem, frames[0], w, h, "frame 0")
        e.set_vbv_state(12500, 40000)
        coded = e.encode(frames[1])
        assert len(coded) < 32                                 # one slice that is a skip run over the picture
        ssd, ssim, rec1 = check_last(e, mem, frames[1], w, h, "transparent frame")
        assert (rec1 == rec0).all()
        e.encode(frames[2])                                    # the stream goes on from the same picture
        check_last(e, mem, frames[2], w, h, "frame 2")
    finally:
        e.close()
        mem.close()


def test_per_frame_refusals():
    P = pkg.load_pkg()
    e = P.Encoder(32, 32, gop=30, qp=30, lib=pkg.EMU_LIB)
    try:
        assert "no frame has been encoded yet" in refusal(lambda: e.read_quality())
        e.encode(clips.make("ramp", 32, 32, 1)[0])
        assert "both outputs are NULL" in refusal(lambda: e.read_quality(ssd=False, ssim=False))
        assert e.L.H264E_read_quality(e.persist, None, None) == P.STATUS_BAD_ARGUMENT
    finally:
        e.close()
    for w, h in ((2, 2), (14, 16)):
        frame = clips.make("ramp", w, h, 1)[0]
        mem = DevMem(pkg.EMU_LIB)
        e = P.Encoder(w, h, gop=30, qp=30, lib=pkg.EMU_LIB)
        try:
            e.encode(frame)
            assert ("a %d x %d picture has a chroma plane without an 8 x 8 window" % (w, h)) in refusal(lambda: e.read_quality())
            ssd, _ = e.read_quality(ssim=False)                 # the sums are still served
            rec = last_recon(e, mem, w, h)
            assert [int(v) for v in ssd] == [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(SM.split_i420(frame, w, h), SM.split_i420(rec, w, h))]
        finally:
            e.close()
            mem.close()


def test_psnr_from_ssd():
    P = pkg.load_pkg()
    got = P.psnr_from_ssd(np.array([[0, 16 * 16, 4], [255 * 255 * 64, 1, 0]], np.uint64), 8, 8)
    assert got.shape == (2, 3) and np.isinf(got[0, 0]) and np.isinf(got[1, 2])
    assert abs(got[1, 0] - 0.0) < 1e-12                         # every sample off by 255
    assert abs(got[0, 1] - 10 * np.log10(255 * 255 * 16 / 256)) < 1e-12 and abs(got[0, 2] - 10 * np.log10(255 * 255 * 16 / 4)) < 1e-12


# ---- the command line

def run_app(args, cwd):
    r = subprocess.run([APP] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    return r.stdout.decode().splitlines()


@pytest.mark.parametrize("extra", [[], ["--kbps", "150"]], ids=["cqp", "kbps"])
def test_cli_ssim_line(tmp_path, extra):
    P = pkg.load_pkg()
    w, h, n = 48, 32, 5
    frames = clips.make("scene", w, h, n)
    src = str(tmp_path / ("in_%dx%d.yuv" % (w, h)))
    frames.tofile(src)
    base = ["--input", src, "--gop", "30", "--qp", "28"] + extra
    out = {}
    for name, more in (("plain", []), ("clip", ["--ssim", "x", "--psnr", "x"]), ("frame", ["--ssim", "x", "--psnr", "x", "--clip", "0"]), ("psnr", ["--psnr", "x"]),
                       ("ssim_only", ["--ssim", "x"])):
        dst = str(tmp_path / (name + ".264"))
        out[name] = (run_app(base + ["--output", dst] + more, str(tmp_path)), hashlib.md5(open(dst, "rb").read()).hexdigest())
    assert len({v[1] for v in out.values()}) == 1                              # the stream does not change
    assert out["clip"][0][1:] == out["frame"][0][1:]                           # (line 0 is sizeof_persist, which --clip 0 with --psnr changes)
    assert out["clip"][0][-1].startswith("SSIM Y=") and out["clip"][0][-2] == out["psnr"][0][-1]       # the --psnr line stays, byte for byte
    assert out["ssim_only"][0] == [out["plain"][0][0], out["clip"][0][-1]] and out["plain"][0] == [out["plain"][0][0]]
    # ... and it is the line the model makes of the per-frame encoder's pictures
    mem = DevMem(pkg.EMU_LIB)
    e = P.Encoder(w, h, gop=30, qp=28, kbps=int(extra[1]) if extra else 0, lib=pkg.EMU_LIB)
    try:
        values = []
        for f in range(n):
            e.encode(frames[f])
            rec = last_recon(e, mem, w, h)
            values.append([SM.plane(a, b) for a, b in zip(SM.split_i420(frames[f], w, h), SM.split_i420(rec, w, h))])
        assert out["clip"][0][-1] == SM.line(values)
    finally:
        e.close()
        mem.close()
