"""GPU: per-frame QP schedules and the lookahead rate control (h264e_lookahead_kernel, enc_lookahead.h) on the MI355X: the reference's
recorded streams with a QP per frame (tests/golden/qp_schedule.json), the cost pass against the numpy model
(tests/lookahead_model.py), the controller against the model's plan and against its own stream under other call patterns and in a
launch group, and its bitrate against the target with the reference's own controller as the yardstick (tests/golden/lookahead.json)."""
import json
import os

import numpy as np
import pytest

import clips
import lookahead_model as M
import pkg
import run_param_cases as R
import scenecut_model
from test_emu_key_frames import check_case
from test_emu_lookahead import CTL, SHAPES, check_step_bound, clip_kw, same

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "qp_schedule.json")))
RATES = json.load(open(os.path.join(HERE, "golden", "lookahead.json")))


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("name", sorted(CASES))
def test_clip_encoder_with_qp_schedule_matches_reference(P, name):
    case = CASES[name]
    w, h = case["create"][:2]
    raw, _ = R.pictures(case)
    ce = P.ClipEncoder(w, h, len(raw), qp_schedule=case["qp"], **clip_kw(case))
    ce.upload(raw)
    out, sizes, st = ce.encode()
    again, _, _ = ce.encode()
    ce.close()
    check_case(case, out, sizes, name)
    assert again == out and st.spin_relaunches == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_frame_encoder_matches_reference(P, name):
    R.compare(CASES[name], R.replay_product(P, CASES[name]), name + " (H264E_encode)")


def analyse(P, w, h, c, **kw):
    kw = dict(dict(gop=4, qp=30, abr_kbps=100, lookahead=2), **kw)
    ce = P.ClipEncoder(w, h, len(c), **kw)
    ce.upload(c)
    out, sizes, st = ce.encode()
    rec, qp = ce.read_lookahead()
    ce.close()
    assert st.spin_relaunches == 0
    return rec, qp, out, sizes


GPU_SHAPES = SHAPES + [(352, 288, "synth", 6), (352, 288, "scene", 6), (352, 288, "noise", 4), (1920, 1080, "scene", 3)]


@pytest.mark.parametrize("w,h,clip,n", GPU_SHAPES, ids=["%dx%d_%s" % s[:3] for s in GPU_SHAPES])
def test_cost_records_equal_the_model_twice(P, w, h, clip, n):
    """(1920x1080: 8040 blocks, 252 workgroups adding to one record)"""
    c = clips.make(clip, w, h, n)
    model = M.costs(c, w, h)
    rec, qp, out, _ = analyse(P, w, h, c)
    assert same(rec, model), (rec, model)
    rec2, qp2, out2, _ = analyse(P, w, h, c)
    assert same(rec2, rec) and np.array_equal(qp, qp2) and out2 == out, "two runs give identical records"


def test_bounded_ring_and_reupload(P):
    w, h, n = 50, 38, 11
    c = clips.make("synth", w, h, n)
    rec1, qp1, want, want_sizes = analyse(P, w, h, c)
    ce = P.ClipEncoder(w, h, n, gop=4, qp=30, resident=4, abr_kbps=100, lookahead=2)
    parts, sizes, per_call = [], [], []
    for f0 in range(0, n, 3):
        ce.upload(c[f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
        per_call.append(len(s))
    rec, qp = ce.read_lookahead()
    ce.close()
    assert per_call == [2, 4, 2, 3]
    assert same(rec, M.costs(c, w, h)) and np.array_equal(qp, qp1) and b"".join(parts) == want and sizes == want_sizes
    c2 = c.copy()
    c2[3:] = clips.make("noise", w, h, n)[3:]
    ce = P.ClipEncoder(w, h, n, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload(c)
    ce.encode()
    ce.upload(c2[3:], first=3)
    changed, _, _ = ce.encode()
    rec, _ = ce.read_lookahead()
    ce.close()
    assert same(rec, M.costs(c2, w, h)) and changed == analyse(P, w, h, c2)[2]


def test_cost_records_on_device_input(P):
    import torch
    w, h, n = 50, 38, 5
    c = clips.make("synth", w, h, n)
    frames = torch.from_numpy(np.ascontiguousarray(c)).cuda().view(n, h * 3 // 2, w)
    ce = P.ClipEncoder(w, h, n, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload_device([frames[i] for i in range(n)], "i420")
    out, _, _ = ce.encode()
    rec, _ = ce.read_lookahead()
    ce.close()
    assert same(rec, M.costs(c, w, h)) and out == analyse(P, w, h, c)[2]


@pytest.fixture(scope="module")
def controlled(P):
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    c = clips.make("synth", w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=gop, qp=30, abr_kbps=kbps, lookahead=W)
    ce.upload(c)
    out, sizes, st = ce.encode()
    rec, qp = ce.read_lookahead()
    again, again_sizes, _ = ce.encode()
    ce.close()
    assert again == out and again_sizes == sizes and st.spin_relaunches == 0
    return dict(clip=c, out=out, sizes=sizes, rec=rec, qp=qp)


def test_controller_is_the_models_plan_and_the_schedules_stream(P, controlled):
    d = controlled
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    ce = P.ClipEncoder(w, h, 1, qp=26)
    ce.upload(d["clip"][:1])
    hdr = (40, 40 + 8 * M.parameter_set_bytes(ce.encode()[0]))
    ce.close()
    assert same(d["rec"], M.costs(d["clip"], w, h))
    assert np.array_equal(d["qp"], M.plan(d["rec"], kinds, hdr, [8 * s for s in d["sizes"]], kbps, W))
    ce = P.ClipEncoder(w, h, n, gop=gop, qp=30, qp_schedule=d["qp"])
    ce.upload(d["clip"])
    out, sizes, _ = ce.encode()
    ce.close()
    assert out == d["out"] and sizes == d["sizes"]


def test_controller_does_not_depend_on_the_call_pattern(P, controlled):
    d = controlled
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    ce = P.ClipEncoder(w, h, n, gop=gop, qp=30, abr_kbps=kbps, lookahead=W)
    parts, sizes = [], []
    for f0 in range(0, n, 3):
        ce.upload(d["clip"][f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
    assert b"".join(parts) == d["out"] and sizes == d["sizes"]
    ce.L.H264E_clip_rewind(ce.c)
    cap = max(d["sizes"]) + sorted(d["sizes"])[n // 2] + 64
    parts, sizes, calls = [], [], 0
    while len(sizes) < n:
        out, s, _ = ce.encode(rewind=False, cap=cap)
        assert s
        parts.append(out)
        sizes += s
        calls += 1
    ce.close()
    assert calls > n // W and b"".join(parts) == d["out"] and sizes == d["sizes"]


def test_a_windows_qp_stays_within_the_step_of_the_window_before(P):
    check_step_bound(P, None)


def test_launch_group_of_two_controlled_clips(P):
    w, h, n, gop, W = 352, 288, 16, 8, 4
    a, b = clips.make("synth", w, h, n), clips.make("pan", w, h, n)
    solo = [analyse(P, w, h, c, gop=gop, abr_kbps=k, lookahead=W) for c, k in ((a, 300), (b, 600))]
    ea = P.ClipEncoder(w, h, n, gop=gop, qp=30, abr_kbps=300, lookahead=W)
    eb = P.ClipEncoder(w, h, n, gop=gop, qp=30, abr_kbps=600, lookahead=W)
    ea.upload(a)
    eb.upload(b)
    (oa, za, sa), (ob, zb, sb) = P.ClipEncoder.encode_multi([ea, eb])
    qa, qb = ea.read_lookahead()[1], eb.read_lookahead()[1]
    ea.close()
    eb.close()
    assert oa == solo[0][2] and ob == solo[1][2] and za == solo[0][3] and zb == solo[1][3]
    assert np.array_equal(qa, solo[0][1]) and np.array_equal(qb, solo[1][1])
    assert sa.spin_relaunches == 0 and sb.spin_relaunches == 0


@pytest.mark.parametrize("g", RATES, ids=["%s_%dkbps" % (g["clip"], g["kbps"]) for g in RATES])
def test_bitrate_stays_within_one_window_of_the_target(P, g):
    """|actual - target| over the clip <= one window's budget (8*dfb*W bits) + the reference controller's own absolute deviation for
    the same clip and target: the carry corrects every window but the last, and where the reference itself cannot reach a target
    (every QP of the range codes `pan` below 1000 kbit/s) neither can this controller."""
    w, h, n, W = g["w"], g["h"], g["frames"], 16
    c = clips.make(g["clip"], w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=g["gop"], qp=30, abr_kbps=g["kbps"], lookahead=W)
    ce.upload(c)
    out, sizes, st = ce.encode()
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    dfb = g["kbps"] * 1000 // 8 // 30
    target, actual, ref = 8 * dfb * n, 8 * len(out), 8 * g["bytes"]
    bound = 8 * dfb * W + abs(ref - target)
    print("%s %d kbps: target %d bits, actual %d, reference %d, deviation %d, bound %d, QPs %s, %d launches" %
          (g["clip"], g["kbps"], target, actual, ref, abs(actual - target), bound, sorted(set(qp.tolist())), st.rounds))
    assert st.spin_relaunches == 0 and sizes and len(sizes) == n
    assert abs(actual - target) <= bound
