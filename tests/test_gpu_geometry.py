"""GPU: extreme picture geometries on the MI355X against the reference's own streams (tests/golden/geometry.json) -- one macroblock cropped
to 2x2, one macroblock per row (the two-wavefront row pipeline) or one row per frame (frame lag, dispatch order), strips of 7680x16 and
16x2048, reference windows larger than the picture, 300 one-macroblock frames in one launch, the denoiser on 1x1 chroma planes, --qp 0 --
through the per-frame and the clip encoder, every kernel variant, launch groups, the reconstruction against the oracle's, and more
slices than macroblock rows.  A clip-encoder dependency wait that only resolved after its bounded spin expired would hide behind a
correct stream: spin_relaunches must stay 0."""
import hashlib
import json
import os

import numpy as np
import pytest

import clips
import denoise_model as M
import oracle_lib
import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "geometry.json")))
CASES = [g for g in GOLDEN if not g.get("diverges")]
BY_NAME = {g["name"]: g for g in GOLDEN}
LIB = os.path.join(HERE, "..", "h264-lab_amd", "lib", "libh264e_mi355x.so")


def flags(s):
    """encode_app options (every long option takes an argument) -> keyword arguments of Encoder / ClipEncoder"""
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), speed=int(d.get("--speed", 0)), kbps=int(d.get("--kbps", 0)),
                slices=int(d.get("--threads", 0)), denoise="--denoise" in d)


def frames(g):
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    return c


def check(g, data, sizes):
    assert sizes == g["frame_bytes"]
    assert hashlib.md5(data).hexdigest() == g["md5"]


def per_frame(P, g, **kw):
    c = frames(g)
    e = P.Encoder(g["w"], g["h"], **dict(flags(g["flags"]), **kw))
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    check(g, b"".join(parts), [len(p) for p in parts])


def clip_encoder(P, g, **kw):
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], **dict(flags(g["flags"]), **kw))
    ce.upload(frames(g))
    out, sizes, st = ce.encode()
    ce.close()
    check(g, out, sizes)
    assert st.spin_relaunches == 0


@pytest.mark.parametrize("g", CASES, ids=lambda g: g["name"])
def test_per_frame_encoder_matches_reference(g):
    per_frame(pkg.load_pkg(), g)


@pytest.mark.parametrize("g", CASES, ids=lambda g: g["name"])
def test_clip_encoder_matches_reference(g):
    clip_encoder(pkg.load_pkg(), g)


@pytest.mark.parametrize("variant", ["waves1", "waves2", "waves3", "waves4", "wide_window"])
@pytest.mark.parametrize("name", ["ramp_2x2_qp26", "ramp_16x16_qp26", "ramp_1920x16_qp26", "ramp_16x1080_qp30"])
def test_every_kernel_variant_matches_reference(monkeypatch, name, variant):
    """one wave per row, two at 3 and at 4 waves per SIMD, the four-wave variant (H264E_WAVES=1..4), and the 64x64 window with its 7-step
    frame lag (H264E_WIDE_WINDOW=1), on pictures of one macroblock, one row and one column"""
    if variant == "wide_window":
        monkeypatch.setenv("H264E_WIDE_WINDOW", "1")
    else:
        monkeypatch.setenv("H264E_WAVES", variant[-1])
    P = pkg.load_pkg()
    clip_encoder(P, BY_NAME[name])
    per_frame(P, BY_NAME[name])


@pytest.mark.parametrize("name,slices", [("noise_64x32_thr2", 3), ("noise_64x32_thr2", 16), ("ramp_16x64_thr4", 9), ("ramp_16x16_qp26", 4)])
def test_more_slices_than_rows_give_the_reference_stream_of_one_slice_per_row(name, slices):
    """N slices on a picture of R < N macroblock rows = the reference's --threads R stream (the reference itself codes rows twice there:
    DESIGN.md 4.6), per-frame API and clip encoder"""
    P = pkg.load_pkg()
    g = BY_NAME[name]
    per_frame(P, g, slices=slices)
    clip_encoder(P, g, slices=slices)


def test_launch_groups_of_tiny_geometries():
    """H264E_clip_encode_multi over clips of 2x2, 16x2048 and 7680x16, two of each size with different lengths: the clips of one size
    share a launch group, the sizes follow each other; every stream is the oracle's for its length (the full-length ones: the
    reference's)"""
    P = pkg.load_pkg()
    specs = [("ramp_2x2_qp26", 8), ("ramp_2x2_qp26", 5), ("ramp_16x2048_qp26", 5), ("ramp_16x2048_qp26", 3), ("ramp_7680x16_qp26", 4),
             ("ramp_7680x16_qp26", 2)]
    encs, want = [], []
    for name, n in specs:
        g = BY_NAME[name]
        kw = flags(g["flags"])
        kw.pop("denoise")
        c = frames(g)[:n]
        want.append(oracle_lib.encode_clip(c, g["w"], g["h"], **kw))
        ce = P.ClipEncoder(g["w"], g["h"], n, **kw)
        ce.upload(c)
        encs.append(ce)
    res = P.ClipEncoder.encode_multi(encs)
    for ce in encs:
        ce.close()
    for (name, n), (out, sizes, st), (wbytes, wsizes) in zip(specs, res, want):
        g = BY_NAME[name]
        assert sizes == wsizes == g["frame_bytes"][:n], (name, n)
        assert out == wbytes, (name, n)
        if n == g["frames"]:
            assert hashlib.md5(out).hexdigest() == g["md5"]
        assert st.spin_relaunches == 0


def _crop(buf, cw, ch, w, h):
    """the visible picture (w x h and its chroma) of a coded-size I420 buffer"""
    y = buf[: cw * ch].reshape(ch, cw)[:h, :w]
    u = buf[cw * ch: cw * ch * 5 // 4].reshape(ch // 2, cw // 2)[: h // 2, : w // 2]
    v = buf[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)[: h // 2, : w // 2]
    return y, u, v


@pytest.mark.parametrize("name", ["ramp_16x2048_qp26", "ramp_7680x16_qp26"])
def test_written_back_reconstruction_matches_oracle(name):
    """const_input_flag = 0 (the reference takes it only when both sizes are multiples of 16, h264-lab.h:6279): the deblocked
    reconstruction of a strip goes back into the caller's frame and equals the oracle's, frame by frame"""
    P = pkg.load_pkg()
    g = BY_NAME[name]
    w, h = g["w"], g["h"]
    kw = flags(g["flags"])
    kw.pop("denoise")
    c = frames(g)
    o = oracle_lib.Encoder(w, h, **kw)
    e = P.Encoder(w, h, const_input=0, **kw)
    parts = []
    for t in range(g["frames"]):
        f = c[t].copy()
        parts.append(e.encode(f))
        assert parts[-1] == o.encode(c[t]), "frame %d" % t
        rec, cw, ch = o.recon()
        assert (cw, ch) == (w, h)
        assert np.array_equal(f, rec), "frame %d: written-back reconstruction differs from the oracle's" % t
    e.close()
    o.close()
    check(g, b"".join(parts), [len(p) for p in parts])


@pytest.mark.parametrize("name", ["ramp_18x18_qp10", "ramp_2x160_qp26"])
def test_clip_reconstruction_matches_oracle(name):
    """H264E_clip_read_recon of cropped pictures (18x18: four macroblocks, mostly edge extension; 2x160: a column of ten macroblocks two
    samples wide) against the oracle's reconstruction, every plane cropped to the picture"""
    P = pkg.load_pkg()
    g = BY_NAME[name]
    w, h, n = g["w"], g["h"], g["frames"]
    kw = flags(g["flags"])
    kw.pop("denoise")
    c = frames(g)
    ce = P.ClipEncoder(w, h, n, **kw)
    ce.upload(c)
    out, sizes, st = ce.encode()
    recs = [ce.read_recon(t) for t in range(n)]
    ce.close()
    check(g, out, sizes)
    o = oracle_lib.Encoder(w, h, **kw)
    for t in range(n):
        o.encode(c[t])
        rec, cw, ch = o.recon()
        assert recs[t].size == rec.size
        for k, (a, b) in enumerate(zip(_crop(recs[t], cw, ch, w, h), _crop(rec, cw, ch, w, h))):
            assert np.array_equal(a, b), "frame %d plane %d" % (t, k)
    o.close()


@pytest.mark.parametrize("w,h,n,resident,chunk", [(2, 2, 5, 3, 1), (4, 4, 5, 5, None), (6, 6, 6, 2, 2), (2, 64, 4, 4, None), (202, 2, 4, 1, 1),
                                                  (18, 34, 6, 3, 3)])
def test_denoiser_tiny_planes_match_model(w, h, n, resident, chunk):
    """h264e_denoise_kernel on planes of 2x2 / 1x1, 4x4 / 2x2, 6x6 / 3x3, 2x64 / 1x32, 202x2 / 101x1 -- the "w <= 2 or h <= 2 keeps the
    state" branch -- and 18x34 (rows of 18 and 9 bytes: not dword aligned), against the numpy model"""
    c = clips.make("ramp", w, h, n)
    want = M.clip(c, w, h)
    got = M.device_planes(LIB, c, w, h, resident, chunk)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), "frame %d differs from the model" % i
