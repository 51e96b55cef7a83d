"""CPU: extreme picture geometries against the reference's own streams (tests/golden/geometry.json, make_golden_geometry.py) -- one
macroblock cropped down to 2x2, one macroblock row or column, strips of 7680x16 and 16x2048, reference windows larger than the picture,
300 one-macroblock frames in one launch, row-band slices of one row, the denoiser on 1x1 chroma planes, --qp 0 -- through the oracle
and the lane-loop emulation of the kernels (tests/emu): the per-frame API, and the clip encoder with its default ring and with 3
frames per launch.  Plus the one recorded departure from the reference: more slices than macroblock rows."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import clips
import denoise_model as M
import oracle_lib
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "geometry.json")))
CASES = [g for g in GOLDEN if not g.get("diverges")]
BY_NAME = {g["name"]: g for g in GOLDEN}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


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


@pytest.mark.parametrize("g", [g for g in CASES if "--denoise" not in g["flags"]], ids=lambda g: g["name"])
def test_oracle_matches_reference(g):
    kw = flags(g["flags"])
    kw.pop("denoise")
    data, sizes = oracle_lib.encode_clip(frames(g), g["w"], g["h"], **kw)
    check(g, data, sizes)


@pytest.mark.parametrize("g", CASES, ids=lambda g: g["name"])
def test_per_frame_encoder_matches_reference(g):
    P = pkg.load_pkg()
    c = frames(g)
    e = P.Encoder(g["w"], g["h"], lib=pkg.EMU_LIB, **flags(g["flags"]))
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    check(g, b"".join(parts), [len(p) for p in parts])


@pytest.mark.parametrize("chains", [0, 3], ids=["default_ring", "chains3"])
@pytest.mark.parametrize("g", CASES, ids=lambda g: g["name"])
def test_clip_encoder_matches_reference(g, chains):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=pkg.EMU_LIB, max_chains=chains, **flags(g["flags"]))
    ce.upload(frames(g))
    out, sizes, _ = ce.encode()
    ce.close()
    check(g, out, sizes)


@pytest.mark.parametrize("name,slices", [("noise_64x32_thr2", 3), ("noise_64x32_thr2", 16), ("ramp_16x64_thr4", 9), ("ramp_16x16_qp26", 4)])
def test_more_slices_than_rows_give_the_reference_stream_of_one_slice_per_row(name, slices):
    """the reference splits R macroblock rows into N bands as mby += (R - mby)/(N - i) (h264-lab.h:6526-6534): with N > R its first N - R
    bands have no rows, and each of them still codes row 0 as a complete slice -- a picture whose macroblocks are coded twice.  The
    product clamps N to R, and so does the oracle: the stream is the reference's --threads R stream (R = 1: the single-slice one).  The
    oracle, the per-frame API and the clip encoder"""
    P = pkg.load_pkg()
    g = BY_NAME[name]
    c = frames(g)
    kw = dict(flags(g["flags"]), slices=slices)
    kw.pop("denoise")
    check(g, *oracle_lib.encode_clip(c, g["w"], g["h"], **kw))
    e = P.Encoder(g["w"], g["h"], lib=pkg.EMU_LIB, **kw)
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    check(g, b"".join(parts), [len(p) for p in parts])
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=pkg.EMU_LIB, **kw)
    ce.upload(c)
    out, sizes, _ = ce.encode()
    ce.close()
    check(g, out, sizes)


def test_reference_stream_with_more_slices_than_rows_differs():
    """the recorded fact behind that clamp: the reference's own --threads 3 stream of a picture of two macroblock rows is not its
    --threads 2 stream, and it is longer (slices 0 and 1 both code row 0)"""
    a, b = BY_NAME["noise_64x32_thr3"], BY_NAME["noise_64x32_thr2"]
    assert a["input_md5"] == b["input_md5"]
    assert a["md5"] != b["md5"] and a["bytes"] > b["bytes"]


@pytest.mark.parametrize("w,h,n,resident,chunk", [(2, 2, 5, 3, 1), (4, 4, 5, 5, None), (6, 6, 6, 2, 2), (2, 64, 4, 4, None), (202, 2, 4, 1, 1),
                                                  (18, 34, 6, 3, 3)])
def test_denoised_tiny_planes_match_model(w, h, n, resident, chunk):
    """planes of 2x2 / 1x1, 4x4 / 2x2, 6x6 / 3x3, 2x64 / 1x32, 202x2 / 101x1 -- the "w <= 2 or h <= 2 keeps the state" branch -- and 18x34
    (rows of 18 and 9 bytes: not dword aligned)"""
    c = clips.make("ramp", w, h, n)
    want = M.clip(c, w, h)
    got = M.device_planes(pkg.EMU_LIB, c, w, h, resident, chunk)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), "frame %d differs from the model" % i
