"""GPU: the temporal denoiser on the MI355X (h264e_denoise_kernel) -- the reference's own --denoise streams (tests/golden/denoise.json)
through the per-frame and the clip encoder, the kernel's planes against the numpy model, launch groups, and the raw-input SSD."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import clips
import denoise_model as M
import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "denoise.json")))
LIB = os.path.join(HERE, "..", "h264-lab_amd", "lib", "libh264e_mi355x.so")


def _flags(s):
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), speed=int(d.get("--speed", 0)), kbps=int(d.get("--kbps", 0)),
                slices=int(d.get("--threads", 0)))


def _frames(P, g):
    """the case's input frames; synth_v1 at 1080p comes from the device generator (numpy would take a minute)"""
    w, h, n = g["w"], g["h"], g["frames"]
    if g["clip"] != "synth" or w * h < 1920 * 1080:
        return clips.make(g["clip"], w, h, n)
    ce = P.ClipEncoder(w, h, n)
    ce.generate_synth()
    buf = np.empty((n, w * h * 3 // 2), np.uint8)
    ce.L.H264E_clip_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert ce.L.H264E_clip_download(ce.c, 0, n, buf.ctypes.data) == 0
    ce.close()
    return buf


@pytest.fixture(scope="module")
def inputs():
    P = pkg.load_pkg()
    cache = {}

    def get(g):
        key = (g["clip"], g["w"], g["h"], g["frames"])
        if key not in cache:
            cache[key] = _frames(P, g)
            assert hashlib.md5(cache[key].tobytes()).hexdigest() == g["input_md5"]
        return cache[key]
    return get


@pytest.mark.parametrize("g", GOLDEN, ids=lambda g: g["name"])
def test_per_frame_encoder_matches_reference(g, inputs):
    P = pkg.load_pkg()
    c = inputs(g)
    e = P.Encoder(g["w"], g["h"], denoise=True, **_flags(g["flags"]))
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    assert [len(p) for p in parts] == g["frame_bytes"]
    assert hashlib.md5(b"".join(parts)).hexdigest() == g["md5"]


@pytest.mark.parametrize("g", GOLDEN, ids=lambda g: g["name"])
def test_clip_encoder_matches_reference(g, inputs):
    P = pkg.load_pkg()
    c = inputs(g)
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], denoise=True, **_flags(g["flags"]))
    ce.upload(c)
    out, sizes, st = ce.encode()
    assert sizes == g["frame_bytes"]
    assert hashlib.md5(out).hexdigest() == g["md5"]
    assert st.spin_relaunches == 0
    again, _, _ = ce.encode()               # rewound: the kept denoised pictures give the same stream
    ce.close()
    assert again == out


def test_bench_geometry_from_device_input_with_bounded_ring():
    """1080p synth_v1 generated in HBM, fed through a 7-frame input ring in chunks"""
    P = pkg.load_pkg()
    g = next(x for x in GOLDEN if x["name"] == "synth_1080p_60")
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], denoise=True, resident=7, **_flags(g["flags"]))
    parts, sizes = [], []
    for f0 in range(0, g["frames"], 7):
        k = min(7, g["frames"] - f0)
        ce.generate_synth(first=f0, nframes=k, t0=f0)
        out, s, st = ce.encode(rewind=(f0 == 0))
        assert st.spin_relaunches == 0
        parts.append(out)
        sizes += s
    ce.close()
    assert sizes == g["frame_bytes"]
    assert hashlib.md5(b"".join(parts)).hexdigest() == g["md5"]


@pytest.mark.parametrize("name,w,h,n,resident,chunk", [
    ("synth", 1920, 1080, 4, 4, 2),
    ("scene", 352, 288, 6, 3, 3),
    ("synth", 200, 120, 5, 5, None),        # 100-byte chroma rows
    ("noise", 202, 122, 4, 2, 1),           # 101 x 61 chroma planes: rows that are not dword aligned
    ("noise", 64, 48, 3, 1, 1),             # single-slot pool: ping-pong
])
def test_kernel_planes_match_model(name, w, h, n, resident, chunk):
    frames = clips.make(name, w, h, n)
    want = M.clip(frames, w, h)
    got = M.device_planes(LIB, frames, w, h, resident, chunk)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), "frame %d differs from the model" % i


def test_two_denoising_clips_in_one_launch_group():
    P = pkg.load_pkg()
    gs = [next(x for x in GOLDEN if x["name"] == k) for k in ("synth_cif_30", "scene_cif_30")]
    encs = []
    for g in gs:
        ce = P.ClipEncoder(g["w"], g["h"], g["frames"], denoise=True, **_flags(g["flags"]))
        ce.upload(clips.make(g["clip"], g["w"], g["h"], g["frames"]))
        encs.append(ce)
    res = P.ClipEncoder.encode_multi(encs)
    for ce in encs:
        ce.close()
    for g, (out, sizes, st) in zip(gs, res):
        assert sizes == g["frame_bytes"]
        assert hashlib.md5(out).hexdigest() == g["md5"]
        assert st.spin_relaunches == 0


def test_ssd_compares_raw_input_with_reconstruction():
    P = pkg.load_pkg()
    w, h, n = 352, 288, 6
    c = clips.make("scene", w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26, denoise=True)
    ce.upload(c)
    ssd = np.zeros((n, 3), np.uint64)
    ce.L.H264E_clip_set_ssd_output(ce.c, ssd.ctypes.data)
    ce.encode()
    recs = [ce.read_recon(f) for f in range(n)]
    ce.L.H264E_clip_set_ssd_output(ce.c, None)
    ce.close()
    cw, chh = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    for f in range(n):
        raw, r = c[f].astype(np.int64), recs[f].astype(np.int64)
        planes = [(raw[: w * h].reshape(h, w), r[: cw * chh].reshape(chh, cw)[:h, :w])]
        o, ro = w * h, cw * chh
        for _ in range(2):
            planes.append((raw[o: o + w * h // 4].reshape(h // 2, w // 2), r[ro: ro + cw * chh // 4].reshape(chh // 2, cw // 2)[: h // 2, : w // 2]))
            o += w * h // 4
            ro += cw * chh // 4
        want = [int(((a - b) ** 2).sum()) for a, b in planes]
        assert [int(x) for x in ssd[f]] == want, "frame %d" % f
