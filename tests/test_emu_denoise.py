"""CPU: the temporal denoiser (H264E_set_denoise / H264E_clip_set_denoise, enc_denoise.h) in the lane-loop emulation of the kernels
(tests/emu): denoised planes against the numpy model, streams against the reference's own --denoise streams (tests/golden/denoise.json),
and the stream-level rules (speed >= 2 leaves the state alone, rewinds and bounded input rings, what is refused)."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import clips
import denoise_model as M
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "denoise.json")))
SMALL = [g for g in GOLDEN if g["w"] * g["h"] * g["frames"] <= 352 * 288 * 60]
REF_HEADER = os.path.join(os.environ.get("H264E_REF_SRC", "/root/reference/src"), "h264-lab.h")     # oracle/Makefile REF


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def _flags(s):
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), speed=int(d.get("--speed", 0)), kbps=int(d.get("--kbps", 0)),
                slices=int(d.get("--threads", 0)))


def _cut(w, h, n):
    """synth_v1, then a scene cut to different content half way"""
    a = clips.make("synth", w, h, n)
    b = clips.make("scene", w, h, n)
    return np.concatenate([a[: n // 2], b[n // 2:]])


@pytest.mark.parametrize("w,h,n,resident,chunk", [
    (176, 144, 6, 4, 2),        # zero-state first frame, then chained frames across a wrapping ring
    (200, 120, 5, 5, None),     # cropped picture, 100-byte chroma rows
    (202, 122, 6, 3, 3),        # 101 x 61 chroma planes: rows that are not dword aligned
    (64, 48, 4, 1, 1),          # single-slot pool (the per-frame API's): ping-pong
    (4, 6, 3, 2, 1),            # 2 x 3 chroma planes: degenerate, left unchanged
])
def test_denoised_planes_match_model(w, h, n, resident, chunk):
    frames = _cut(w, h, n) if w >= 16 else clips.make("noise", w, h, n)
    want = M.clip(frames, w, h)
    got = M.device_planes(pkg.EMU_LIB, frames, w, h, resident, chunk)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), "frame %d differs from the model" % i


def _table(text, name):
    m = re.search(name + r"\s*\[256\]\s*=\s*\{([^}]*)\}", text)
    return [int(x) for x in m.group(1).replace("\n", " ").split(",") if x.strip()]


def test_gain_table_matches_model_and_reference():
    t = _table(open(os.path.join(HERE, "..", "h264-lab_amd", "csrc", "tables.h")).read(), "k_denoise_gain")
    assert t == [int(x) for x in M.GAIN]
    if not os.path.exists(REF_HEADER):
        pytest.skip("reference sources not present")
    assert t == _table(open(REF_HEADER).read(), "g_diff_to_gainQ8")


def _check(g, parts):
    assert [len(p) for p in parts] == g["frame_bytes"]
    assert hashlib.md5(b"".join(parts)).hexdigest() == g["md5"]


@pytest.mark.parametrize("g", SMALL, ids=lambda g: g["name"])
def test_per_frame_encoder_matches_reference(g):
    P = pkg.load_pkg()
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    e = P.Encoder(g["w"], g["h"], lib=pkg.EMU_LIB, denoise=True, **_flags(g["flags"]))
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    _check(g, parts)


@pytest.mark.parametrize("g", SMALL, ids=lambda g: g["name"])
def test_clip_encoder_matches_reference(g):
    P = pkg.load_pkg()
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=pkg.EMU_LIB, denoise=True, **_flags(g["flags"]))
    ce.upload(c)
    out, sizes, _ = ce.encode()
    ce.close()
    assert sizes == g["frame_bytes"]
    assert hashlib.md5(out).hexdigest() == g["md5"]


def test_speed_switch_leaves_the_state_alone():
    """per-frame API: frames with encode_speed >= 2 are encoded raw and do not move the denoiser's state -- the same stream as encoding
    the model's pictures with the denoiser off"""
    P = pkg.load_pkg()
    w, h, n = 176, 144, 7
    speeds = [0, 2, 0, 1, 2, 2, 0]
    c = _cut(w, h, n)
    pics = M.clip(c, w, h, apply=[s < 2 for s in speeds])
    a = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB, denoise=True)
    b = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB)
    for t in range(n):
        a.rp.encode_speed = b.rp.encode_speed = speeds[t]
        assert a.encode(c[t]) == b.encode(pics[t]), "frame %d" % t
    a.close()
    b.close()


def test_reconstruction_goes_back_to_the_caller_and_input_is_denoised():
    """const_input_flag = 0: the reconstruction replaces the caller's planes, and the encoded picture is the denoised one"""
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    c = clips.make("noise", w, h, n)
    pics = M.clip(c, w, h)
    a = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB, denoise=True, const_input=0)
    b = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB, const_input=0)
    for t in range(n):
        fa, fb = c[t].copy(), pics[t].copy()
        assert a.encode(fa) == b.encode(fb)
        assert np.array_equal(fa, fb)
    a.close()
    b.close()


def test_bounded_ring_and_rewind_give_identical_bytes():
    P = pkg.load_pkg()
    g = next(x for x in GOLDEN if x["name"] == "noise_qcif_8")
    w, h, n = g["w"], g["h"], g["frames"]
    c = clips.make(g["clip"], w, h, n)
    whole = P.ClipEncoder(w, h, n, lib=pkg.EMU_LIB, denoise=True, **_flags(g["flags"]))
    whole.upload(c)
    first, _, _ = whole.encode()
    again, _, _ = whole.encode()            # rewound: the denoised pictures are kept
    assert hashlib.md5(first).hexdigest() == g["md5"] and again == first
    # re-uploading frames 4.. makes their denoised pictures again (the state in front of frame 4 is kept)
    c2 = c.copy()
    c2[4:] = clips.make("synth", w, h, n)[4:]
    whole.upload(c2[4:], first=4)
    changed, _, _ = whole.encode()
    whole.close()
    fresh = P.ClipEncoder(w, h, n, lib=pkg.EMU_LIB, denoise=True, **_flags(g["flags"]))
    fresh.upload(c2)
    want, _, _ = fresh.encode()
    fresh.close()
    assert changed == want and changed != first
    # a bounded input ring (3 frames), fed while the stream is encoded
    ring = P.ClipEncoder(w, h, n, lib=pkg.EMU_LIB, denoise=True, resident=3, **_flags(g["flags"]))
    parts = []
    for f0 in range(0, n, 3):
        ring.upload(c[f0:f0 + 3], first=f0)
        out, _, _ = ring.encode(rewind=(f0 == 0))
        parts.append(out)
    ring.close()
    assert b"".join(parts) == first


def test_refusals():
    P = pkg.load_pkg()
    with pytest.raises(P.H264EError):
        P.ClipEncoder(64, 48, 4, lib=pkg.EMU_LIB, keep_records=1, denoise=True)
    ce = P.ClipEncoder(64, 48, 4, lib=pkg.EMU_LIB)
    ce.upload(clips.make("synth", 64, 48, 4))
    ce.encode(rewind=False)
    with pytest.raises(P.H264EError):
        ce.set_denoise(True)                # not at frame 0
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise(True)                    # rewound: allowed
    ce.close()
    e = P.Encoder(64, 48, gop=30, qp=26, lib=pkg.EMU_LIB)
    e.encode(clips.make("synth", 64, 48, 1)[0])
    assert e.L.H264E_set_denoise(e.persist, 1) != 0      # after the first frame
    e.close()
