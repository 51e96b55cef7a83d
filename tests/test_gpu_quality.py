"""GPU: the quality metrics on the MI355X (h264e_ssim_kernel / h264e_ssim_mean_kernel next to h264e_ssd_kernel) against tests/ssim_model.py:
plane pairs from torch tensors (contiguous, a channel slice, a row-strided view, odd addresses with odd strides), the clip encoder and the
frame-at-a-time encoder at small sizes, one 1920x1080 frame for the grid's real extent, the command line.

SSIM tolerance (derived in ssim_model.py, not measured): |got - model| <= (N + 8) 2^-52 for a plane of N windows.  The sums of squared
differences are integers: equality.  Two runs, and solo against encode_multi, must give the same doubles bit for bit: the order of the sum
is fixed by indices, never by which workgroup finishes first.

Noted, not asserted: the GPU's doubles equalled the emulation's bit for bit in every case tried on an MI355X (18 plane pairs of noise
against disturbed noise, 8x8 to 1920x1080, through H264E_ssim_planes of both libraries in one process) -- both add in the same order and
the kernel's float64 division is correctly rounded, like the host's.  Against the model (math.fsum) the largest difference seen in this
file's cases was 2.2e-16 (218 of 269 values equal the model's exactly), at bounds from 2.0e-15 (one window) to 2.9e-11 (1080p luma)."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import clips
import pkg
import ssim_model as SM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
APP = os.path.join(os.path.dirname(HERE), "h264-lab_amd", "lib", "encode_app")
PLANE_SIZES = [(8, 8), (9, 17), (18, 34), (272, 272)]
CONTENTS = ["noise", "noise_inverse", "0_255", "checker_inverse", "255_255"]
LAYOUTS = ["contiguous", "channel", "rows", "odd"]


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def noise(w, h, salt):
    return clips._hash_bytes(w * h, salt).reshape(h, w)


def pair(name, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    chk = (((xx + yy) & 1) * 255).astype(np.uint8)
    return {"noise": (noise(w, h, 1), noise(w, h, 2)), "noise_inverse": (noise(w, h, 1), 255 - noise(w, h, 1)),
            "0_255": (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)), "checker_inverse": (chk, 255 - chk),
            "255_255": (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8))}[name]


def view(torch, a, layout, k=0):
    """the 2-D array as a CUDA tensor view of that layout, holding a's samples"""
    h, w = a.shape
    src = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "contiguous":
        v = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    elif layout == "channel":                      # channel 1 of a (3, h, w) tensor
        v = torch.full((3, h, w), 0xA5, dtype=torch.uint8, device="cuda")[1]
    elif layout == "rows":                         # every other row of a tensor twice as high, columns 3.. of wider rows
        v = torch.full((2 * h, w + 5), 0xA5, dtype=torch.uint8, device="cuda")[::2, 3:3 + w]
    else:                                          # an odd address and an odd stride inside a flat buffer
        stride = (w + 12) | 1
        flat = torch.full((16 + stride * h + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        v = flat.as_strided((h, w), (stride, 1), 16 + (1, 3)[k])
    v.copy_(src)
    return v


_models = {}


def model_value(name, w, h):
    if (name, w, h) not in _models:
        _models[(name, w, h)] = SM.plane(*pair(name, w, h))
    return _models[(name, w, h)]


@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("w,h", PLANE_SIZES)
def test_plane_pair_matches_the_model(P, torch, w, h, name):
    a, b = pair(name, w, h)
    want, got = model_value(name, w, h), {}
    for layout in LAYOUTS:
        got[layout] = P.ssim_planes(view(torch, a, layout, 0), view(torch, b, layout, 1))
        print("%dx%d %s %s: got %r (%s) model %r diff %.3g bound %.3g" % (w, h, name, layout, got[layout], got[layout].hex(), want, abs(got[layout] - want), SM.tolerance(w, h)))
        assert abs(got[layout] - want) <= SM.tolerance(w, h), layout
    assert len({v.hex() for v in got.values()}) == 1              # the layout changes the loads, not the value
    assert P.ssim_planes(view(torch, a, "odd", 0), view(torch, a, "rows", 1)) == 1.0
    if name == "255_255":
        assert got["contiguous"] == 1.0
    if name == "0_255" and (w, h) == (8, 8):
        assert got["contiguous"] == 416 / 266342816


def test_plane_pair_refusals(P, torch):
    def refusal(f):
        with pytest.raises(P.H264EError) as e:
            f()
        return str(e.value)

    t = torch.zeros((32, 32), dtype=torch.uint8, device="cuda")
    L = P.load()
    import ctypes as C
    out = C.c_double(-5.0)
    host = np.zeros((32, 32), np.uint8)
    assert L.H264E_ssim_planes(0, host.ctypes.data, 32, t.data_ptr(), 32, 32, 32, C.byref(out)) == -1
    assert "plane a" in L.H264E_last_error().decode() and "is not memory of device 0" in L.H264E_last_error().decode()
    # an allocation of the runtime's own (torch hands out pieces of larger segments) that is one byte short of the plane's last row
    pitch = 4096
    short, fits = L.H264E_dev_malloc(0, 31 * pitch + 31), L.H264E_dev_malloc(0, 31 * pitch + 32)
    try:
        assert short and fits
        assert L.H264E_ssim_planes(0, fits, pitch, short, pitch, 32, 32, C.byref(out)) == -1
        assert "plane b" in L.H264E_last_error().decode() and "not inside one allocation" in L.H264E_last_error().decode()
        assert out.value == -5.0
        assert L.H264E_ssim_planes(0, fits, pitch, fits, pitch, 32, 32, C.byref(out)) == 0 and out.value == 1.0
    finally:
        L.H264E_dev_free(short)
        L.H264E_dev_free(fits)
    assert "width 4 (8 to" in refusal(lambda: P.ssim_planes(t[:, :4], t[:, :4]))
    assert "two 2-D uint8 arrays of one shape" in refusal(lambda: P.ssim_planes(t, t[:16]))
    assert "two 2-D uint8 arrays of one shape" in refusal(lambda: P.ssim_planes(t.t(), t.t()))             # the last axis is not contiguous
    assert "8-bit samples" in refusal(lambda: P.ssim_planes(t.float(), t.float()))


# ---- the clip encoder

def check_frames(P, ce, frames, w, h, first, ssd, ssim, what):
    for i in range(ssd.shape[0]):
        f = first + i
        rec = ce.read_recon(f)
        want = SM.frame(frames[f], rec, w, h)
        assert [int(v) for v in ssd[i]] == SM.frame_ssd(frames[f], rec, w, h), "%s: SSD of frame %d" % (what, f)
        for k in range(3):
            pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
            print("%s frame %d plane %d: got %r (%s) model %r diff %.3g bound %.3g" % (what, f, k, ssim[i][k], float(ssim[i][k]).hex(), want[k], abs(ssim[i][k] - want[k]), SM.tolerance(pw, ph)))
            assert abs(ssim[i][k] - want[k]) <= SM.tolerance(pw, ph), "%s: SSIM of frame %d plane %d" % (what, f, k)


def run_clip(P, frames, w, h, quality=True, **kw):
    n = len(frames)
    ce = P.ClipEncoder(w, h, n, quality=quality, **kw)
    try:
        ce.upload(frames)
        out, sizes, _ = ce.encode()
        assert len(sizes) == n
        return out, ce.read_quality(), ce
    except Exception:
        ce.close()
        raise


@pytest.mark.parametrize("qp", [10, 51])
@pytest.mark.parametrize("content", ["noise", "ramp"])
@pytest.mark.parametrize("w,h,n", [(16, 16, 3), (18, 34, 4), (272, 144, 3)])
def test_clip_metrics_match_the_model(P, w, h, n, content, qp):
    frames = clips.make(content, w, h, n)
    out, (ssd, ssim), ce = run_clip(P, frames, w, h, gop=30, qp=qp)
    try:
        assert (ce.download() == frames).all()
        check_frames(P, ce, frames, w, h, 0, ssd, ssim, "%dx%d %s qp %d" % (w, h, content, qp))
    finally:
        ce.close()
    # a second run in the same process: the same doubles; with the metrics off: the same stream
    out2, (ssd2, ssim2), ce = run_clip(P, frames, w, h, gop=30, qp=qp)
    ce.close()
    out3, (none_a, none_b), ce = run_clip(P, frames, w, h, quality=None, gop=30, qp=qp)
    ce.close()
    assert out2 == out and out3 == out and none_a is None and none_b is None
    assert (ssd2 == ssd).all() and ssim2.tobytes() == ssim.tobytes()


def test_denoiser_rate_control_and_two_calls(P):
    w, h, n = 64, 48, 6
    frames = clips.noise(w, h, n) // 8 + clips.make("ramp", w, h, n) // 2
    out, (ssd, ssim), ce = run_clip(P, frames, w, h, gop=30, qp=20, denoise=True)
    try:
        check_frames(P, ce, frames, w, h, 0, ssd, ssim, "denoise (raw input)")
    finally:
        ce.close()
    # rate control: the launches' hedge leaves overwrite older pictures, so the clip's values are checked through the per-frame encoder,
    # whose stream and pictures are the same, frame by frame
    frames = clips.make("scene", w, h, n)
    out, (ssd, ssim), ce = run_clip(P, frames, w, h, gop=30, qp=26, kbps=100)
    ce.close()
    e = P.Encoder(w, h, gop=30, kbps=100)
    try:
        got = b""
        for f in range(n):
            got += e.encode(frames[f])
            d, s = e.read_quality()
            assert (d == ssd[f]).all() and s.tobytes() == ssim[f].tobytes(), "frame %d" % f
        assert got == out
    finally:
        e.close()
    ce = P.ClipEncoder(w, h, n, gop=30, qp=30, quality=True)
    try:
        ce.upload(frames[:2])
        ce.encode()
        a = ce.read_quality()
        assert a[0].shape == (2, 3)
        check_frames(P, ce, frames, w, h, 0, a[0], a[1], "first call")
        ce.upload(frames[2:], first=2)
        ce.encode(rewind=False)
        b = ce.read_quality()
        assert b[0].shape == (n - 2, 3)
        check_frames(P, ce, frames, w, h, 2, b[0], b[1], "second call")
    finally:
        ce.close()


def test_encode_multi_equals_solo_bit_for_bit(P):
    w, h, n = 64, 48, 4
    names = ["scene", "ramp"]
    want = {}
    for name in names:
        out, q, ce = run_clip(P, clips.make(name, w, h, n), w, h, gop=30, qp=26)
        ce.close()
        want[name] = (out, q)
    encs = [P.ClipEncoder(w, h, n, gop=30, qp=26, quality=True) for _ in names]
    try:
        for e, name in zip(encs, names):
            e.upload(clips.make(name, w, h, n))
        res = P.ClipEncoder.encode_multi(encs)
        for e, name, r in zip(encs, names, res):
            ssd, ssim = e.read_quality()
            assert r[0] == want[name][0] and (ssd == want[name][1][0]).all() and ssim.tobytes() == want[name][1][1].tobytes(), name
    finally:
        for e in encs:
            e.close()


def test_clip_refused_below_16x16(P):
    ce = P.ClipEncoder(8, 16, 2, gop=30, qp=30)
    try:
        with pytest.raises(P.H264EError, match="a 8 x 16 picture has a chroma plane without an 8 x 8 window"):
            ce.set_quality()
        ce.set_quality(ssim=False)
        frames = clips.make("ramp", 8, 16, 2)
        ce.upload(frames)
        ce.encode()
        ssd, ssim = ce.read_quality()
        assert ssim is None and [[int(v) for v in r] for r in ssd] == [SM.frame_ssd(frames[f], ce.read_recon(f), 8, 16) for f in range(2)]
    finally:
        ce.close()


# ---- the frame-at-a-time encoder

def check_last(e, slot, w, h, what):
    ssd, ssim = e.read_quality()
    rec = e.read_recon_device("i420").cpu().numpy().reshape(-1)
    ya, yb = SM.split_i420(slot, w, h), SM.split_i420(rec, w, h)
    assert [int(v) for v in ssd] == [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(ya, yb)], what
    for k in range(3):
        want = SM.plane(ya[k], yb[k])
        print("%s plane %d: got %r (%s) model %r diff %.3g" % (what, k, ssim[k], float(ssim[k]).hex(), want, abs(ssim[k] - want)))
        assert abs(ssim[k] - want) <= SM.tolerance(*ya[k].shape[::-1]), "%s plane %d" % (what, k)
    return rec


def test_per_frame_encoder(P, torch):
    import rgbp_model
    import scale_model
    for const_input, w, h in ((0, 32, 48), (1, 18, 34)):
        frames = clips.make("ramp", w, h, 3)
        e = P.Encoder(w, h, gop=30, qp=28, const_input=const_input)
        try:
            with pytest.raises(P.H264EError, match="no frame has been encoded yet"):
                e.read_quality()
            for f in range(3):
                e.encode(frames[f].copy())
                check_last(e, frames[f], w, h, "host input, const_input %d, frame %d" % (const_input, f))
        finally:
            e.close()
    w, h = 32, 48
    e = P.Encoder(w, h, gop=30, qp=28)
    try:
        chw = rgbp_model.clip(w, h, 1)[0]
        e.encode_device(torch.from_numpy(np.ascontiguousarray(chw)).cuda(), "rgbp")
        check_last(e, rgbp_model.to_i420(chw), w, h, "rgbp")
        sw, sh = 80, 112
        src = scale_model.source_clip(sw, sh, 1)[0]
        e.encode_device(torch.from_numpy(np.ascontiguousarray(src)).cuda().reshape(sh * 3 // 2, sw), "i420", src_size=(sw, sh))
        check_last(e, scale_model.scale_frame(src, sw, sh, w, h), w, h, "scaled")
    finally:
        e.close()
    # the transparent frame after set_vbv_state: this call's input against the unchanged picture
    w, h = 48, 32
    frames = clips.make("scene", w, h, 2)
    e = P.Encoder(w, h, gop=30, kbps=100)
    try:
        e.encode(frames[0])
        rec0 = check_last(e, frames[0], w, h, "frame 0")
        e.set_vbv_state(12500, 40000)
        assert len(e.encode(frames[1])) < 32
        assert (check_last(e, frames[1], w, h, "transparent frame") == rec0).all()
    finally:
        e.close()
    e = P.Encoder(2, 2, gop=30, qp=30)
    try:
        frame = clips.make("ramp", 2, 2, 1)[0]
        e.encode(frame)
        with pytest.raises(P.H264EError, match="a 2 x 2 picture has a chroma plane without an 8 x 8 window"):
            e.read_quality()
        ssd, _ = e.read_quality(ssim=False)
        rec = e.read_recon_device("i420").cpu().numpy().reshape(-1)
        assert [int(v) for v in ssd] == [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(SM.split_i420(frame, 2, 2), SM.split_i420(rec, 2, 2))]
    finally:
        e.close()


def test_one_1080p_frame(P):
    """the grid's real extent: 576 luma tiles and 2 x 144 chroma tiles, more partials than the second launch has lanes"""
    w, h = 1920, 1080
    frames = clips.make("synth", w, h, 1)
    out, (ssd, ssim), ce = run_clip(P, frames, w, h, gop=30, qp=26)
    try:
        check_frames(P, ce, frames, w, h, 0, ssd, ssim, "1080p")
    finally:
        ce.close()


# ---- the command line

def test_cli_clip_mode_line_equals_frame_mode_line(tmp_path):
    assert os.path.exists(APP), "encode_app not built"
    w, h, n = 176, 144, 6
    src = str(tmp_path / ("in_%dx%d.yuv" % (w, h)))
    clips.make("scene", w, h, n).tofile(src)
    out = {}
    for name, more in (("plain", []), ("clip", ["--ssim", "x", "--psnr", "x"]), ("frame", ["--ssim", "x", "--psnr", "x", "--clip", "0"]), ("psnr", ["--psnr", "x"])):
        dst = str(tmp_path / (name + ".264"))
        r = subprocess.run([APP, "--input", src, "--output", dst, "--gop", "30", "--qp", "28"] + more, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        out[name] = (r.stdout.decode().splitlines(), hashlib.md5(open(dst, "rb").read()).hexdigest())
    assert len({v[1] for v in out.values()}) == 1
    assert out["clip"][0][1:] == out["frame"][0][1:] and out["clip"][0][-1].startswith("SSIM Y=0.")
    assert out["clip"][0][-2] == out["psnr"][0][-1] and len(out["plain"][0]) == 1
