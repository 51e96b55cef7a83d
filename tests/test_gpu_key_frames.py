"""GPU: the clip encoder's key-frame schedule and scene-cut detection (h264e_scenecut_kernel, enc_scenecut.h) on the MI355X: the
reference's recorded streams with forced key frames (tests/golden/key_frames.json), the detector against the numpy model
(tests/scenecut_model.py), 1080p with a hard cut in one and in eight slices, rate control, a launch group of two clips with different
schedules, and device input written on a producer stream."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import clips
import pkg
import run_param_cases as R
import scenecut_model as M
from test_emu_key_frames import check_case, clip_kw

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "key_frames.json")))


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


def encode(P, w, h, c, feed=None, **kw):
    ce = P.ClipEncoder(w, h, len(c), **kw)
    (feed or (lambda e: e.upload(c)))(ce)
    out, sizes, st = ce.encode()
    sc = ce.read_scenecut() if kw.get("scenecut") else None
    ce.close()
    return out, sizes, st, sc


@pytest.mark.parametrize("name", sorted(CASES))
def test_clip_encoder_with_key_frames_matches_reference(P, name):
    case = CASES[name]
    w, h = case["create"][:2]
    raw, _ = R.pictures(case)
    ce = P.ClipEncoder(w, h, len(raw), key_frames=case["forced"], **clip_kw(case))
    ce.upload(raw)
    out, sizes, st = ce.encode()
    again, _, _ = ce.encode()
    ce.close()
    check_case(case, out, sizes, name)
    assert again == out and st.spin_relaunches == 0
    assert st.next_idr_pic_id_state == sum(case["key"]) & 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_frame_encoder_matches_reference(P, name):
    R.compare(CASES[name], R.replay_product(P, CASES[name]), name + " (H264E_encode)")


@pytest.mark.parametrize("clip,w,h,n", [("scene", 352, 288, 12), ("synth", 352, 288, 8), ("pan", 352, 288, 8), ("noise", 352, 288, 4),
                                        ("scene", 64, 48, 10), ("ramp", 6, 6, 8), ("scene", 202, 122, 9)])
def test_scenecut_equals_model_and_the_explicit_list_stream(P, clip, w, h, n):
    """(6x6 and 202x122: slots that do not start on a dword, luma planes whose last dword reaches into the chroma)"""
    gop = 30
    c = clips.make(clip, w, h, n)
    thr = P.H264E_SCENECUT_DEFAULT if w >= 352 else 20
    dist, is_cut, merged = M.detect(c, w, h, gop, threshold=thr)
    out, sizes, st, (d, k) = encode(P, w, h, c, gop=gop, qp=30, scenecut=thr)
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut), (d, dist, k, is_cut)
    if (clip, w) == ("scene", 352):
        assert list(np.flatnonzero(k)) == [n // 2]
    want, want_sizes, _, _ = encode(P, w, h, c, gop=gop, qp=30, key_frames=merged)
    assert out == want and sizes == want_sizes and st.spin_relaunches == 0


def _oracle_with_keys(c, w, h, gop, qp, forced, slices=0):
    """the oracle, driven as tests/run_param_cases.py drives it: KEY on the forced frames, DEFAULT elsewhere"""
    import oracle_lib
    par = oracle_lib.Param(w, h, gop, 0, 0, 100000 // 8, 0, slices or 1)
    L = oracle_lib.lib()
    e = L.h264o_open(C.byref(par))
    assert e
    parts = []
    try:
        for t, f in enumerate(c):
            assert L.h264o_set_run_param(e, M.KEY if t in forced else M.DEFAULT, 0, 0, qp, qp, 0) == 0
            f = np.ascontiguousarray(f, np.uint8)
            base = f.ctypes.data
            p, n = C.c_void_p(), C.c_int()
            assert L.h264o_encode(e, (C.c_void_p * 3)(base, base + w * h, base + w * h * 5 // 4), (C.c_int * 3)(w, w // 2, w // 2), C.byref(p), C.byref(n)) == 0
            parts.append(C.string_at(p, n.value))
    finally:
        L.h264o_close(e)
    return b"".join(parts)


@pytest.mark.parametrize("slices", [0, 8])
def test_hd1080_scene_cut(P, slices):
    w, h, n, gop = 1920, 1080, 8, 30
    c = clips.make("scene", w, h, n)
    dist, is_cut, merged = M.detect(c, w, h, gop)
    assert list(np.flatnonzero(is_cut)) == [n // 2] and dist[n // 2] >= 300 and max(np.delete(dist, n // 2)) <= 10
    out, sizes, st, (d, k) = encode(P, w, h, c, gop=gop, qp=26, slices=slices, scenecut=P.H264E_SCENECUT_DEFAULT)
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut)
    assert st.spin_relaunches == 0
    want, want_sizes, st2, _ = encode(P, w, h, c, gop=gop, qp=26, slices=slices, key_frames=merged)
    assert out == want and sizes == want_sizes and st2.spin_relaunches == 0
    assert out == _oracle_with_keys(c, w, h, gop, 26, set(merged), slices), "the stream with the cut as a key frame differs from the oracle's"


def test_scenecut_under_rate_control_with_a_bounded_ring(P):
    w, h, n, gop = 352, 288, 18, 7
    c = np.concatenate([clips.make("scene", w, h, 10), clips.make("synth", w, h, 8)])
    dist, is_cut, merged = M.detect(c, w, h, gop)
    assert list(np.flatnonzero(is_cut)) == [5, 10]
    want, want_sizes, _, _ = encode(P, w, h, c, gop=gop, kbps=400, key_frames=merged)
    ce = P.ClipEncoder(w, h, n, gop=gop, kbps=400, resident=5, scenecut=128)
    parts, sizes = [], []
    for f0 in range(0, n, 4):
        ce.upload(c[f0:f0 + 4], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
    d, k = ce.read_scenecut()
    ce.close()
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut)
    assert b"".join(parts) == want and sizes == want_sizes


def test_launch_group_of_two_clips_with_different_schedules(P):
    w, h, n, gop = 352, 288, 16, 30
    a, b = clips.make("scene", w, h, n), clips.make("pan", w, h, n)
    _, cut_a, merged_a = M.detect(a, w, h, gop)
    want_a, _, _, _ = encode(P, w, h, a, gop=gop, qp=28, key_frames=merged_a)
    want_b, _, _, _ = encode(P, w, h, b, gop=gop, qp=28, key_frames=[3, 4, 11])
    ea = P.ClipEncoder(w, h, n, gop=gop, qp=28, scenecut=128)
    eb = P.ClipEncoder(w, h, n, gop=gop, qp=28, key_frames=[3, 4, 11])
    ea.upload(a)
    eb.upload(b)
    (oa, _, sa), (ob, _, sb) = P.ClipEncoder.encode_multi([ea, eb])
    d, k = ea.read_scenecut()
    ea.close()
    eb.close()
    assert np.array_equal(k, cut_a) and oa == want_a and ob == want_b
    assert want_a != want_b and sa.spin_relaunches == 0 and sb.spin_relaunches == 0


def test_device_input_with_a_producer_stream(P):
    """the frames are written by copies queued on a non-default torch stream and handed over at once: the histograms (made on the
    encoder's stream, behind the ingest on its copy stream) must see the finished frames"""
    import torch
    w, h, n, gop = 352, 288, 10, 30
    c = clips.make("scene", w, h, n)
    dist, is_cut, merged = M.detect(c, w, h, gop)
    want, _, _, _ = encode(P, w, h, c, gop=gop, qp=28, key_frames=merged)
    staged = torch.from_numpy(np.ascontiguousarray(c)).cuda().view(n, h * 3 // 2, w)
    frames = torch.zeros_like(staged)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ce = P.ClipEncoder(w, h, n, gop=gop, qp=28, scenecut=128)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        for i in range(n):
            frames[i].copy_(staged[i])
        ce.upload_device([frames[i] for i in range(n)], "i420")
    frames.zero_()
    out, _, st = ce.encode()
    d, k = ce.read_scenecut()
    ce.close()
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut) and out == want and st.spin_relaunches == 0
