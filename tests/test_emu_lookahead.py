"""CPU: per-frame QP schedules (H264E_clip_set_qp_schedule) and the lookahead rate control (H264E_clip_set_lookahead, enc_lookahead.h) in
the lane-loop emulation of the kernels (tests/emu).

  - every case of tests/golden/qp_schedule.json -- streams of the REFERENCE with qp_min = qp_max = qp[f] on frame f -- through the clip
    encoder with that schedule, through H264E_encode frame by frame, and through the oracle: exact bytes and frame sizes;
  - the cost pass against the numpy model (tests/lookahead_model.py) on shapes that take every path of the kernel; device input,
    bounded input rings, re-uploads;
  - the controller: its QPs are the model's plan replayed with the stream's own frame sizes, its stream is the stream of those QPs as
    an explicit schedule, and neither depends on how the caller groups its calls;
  - what is refused is refused and leaves the encoder producing the plain stream;
  - a clip encoder on which neither call is made writes the reference's recorded bytes with the launches it took before;
  - the CLI's --qpfile / --kbps K --lookahead W."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import clips
import lookahead_model as M
import pkg
import run_param_cases as R
import scenecut_model
from test_emu_device_input import DevMem
from test_emu_key_frames import _dev_feed, check_case

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "qp_schedule.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
LIB = pkg.EMU_LIB


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def clip_kw(case):
    w, h, gop, _vbv, _cinp, den, slices = case["create"]
    return dict(gop=gop, qp=26, speed=case["clip"]["speed"], slices=slices if slices > 1 else 0, denoise=bool(den), key_frames=case["forced"])


def test_fixture_covers_what_it_is_for():
    assert {"tiny_gop4_every_frame", "qcif_gop5_forced", "qcif_2_slices", "qcif_denoise", "tiny_cropped_34x18"} <= set(CASES)
    for name, c in CASES.items():
        assert [l[3:5] for l in c["frames"]] == [[q, q] for q in c["qp"]] and all(l[2] == 0 for l in c["frames"]), name
        assert c["key"] == [int(k) for k in scenecut_model.kinds(len(c["qp"]), c["create"][2], c["forced"])], name
    t = CASES["tiny_gop4_every_frame"]
    assert t["create"][:3] == [64, 48, 4] and len(t["qp"]) == 12 and {10, 51} <= set(t["qp"])
    assert all(a != b for a, b in zip(t["qp"], t["qp"][1:])), "the QP moves every frame"
    key_qps = [q for q, k in zip(t["qp"], t["key"]) if k]
    assert min(key_qps) < 30 < max(key_qps)
    f = CASES["qcif_gop5_forced"]
    assert f["create"][:3] == [176, 144, 5] and len(f["qp"]) == 10 and f["forced"] and f["key"][f["forced"][0]]
    assert CASES["qcif_2_slices"]["create"][6] == 2 and CASES["qcif_denoise"]["create"][5] == 1 and CASES["tiny_cropped_34x18"]["create"][:2] == [34, 18]


@pytest.mark.parametrize("name", sorted(CASES))
def test_clip_encoder_with_qp_schedule_matches_reference(name):
    P = pkg.load_pkg()
    case = CASES[name]
    w, h = case["create"][:2]
    n = len(case["qp"])
    raw, _ = R.pictures(case)
    ce = P.ClipEncoder(w, h, n, lib=LIB, qp_schedule=case["qp"], **clip_kw(case))
    ce.upload(raw)
    out, sizes, st = ce.encode()
    again, _, _ = ce.encode()                   # a rewind keeps the schedule
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    check_case(case, out, sizes, name)
    assert again == out and qp.tolist() == case["qp"]
    assert (st.rounds, st.reencoded_gops) == (1, 0), "mixed QPs are per-task tables: one launch, nothing stops it"


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_frame_encoder_and_oracle_match_reference(name):
    P = pkg.load_pkg()
    case = CASES[name]
    R.compare(case, R.replay_product(P, case, lib=LIB), name + " (H264E_encode)")
    R.compare(case, R.replay_oracle(case), name + " (oracle)")


# ---- the cost pass

def analyse(P, w, h, c, feed=None, **kw):
    """(I, P, N) and the QPs the controller chose, for a clip fed in one piece"""
    kw = dict(dict(gop=4, qp=30, abr_kbps=100, lookahead=2), **kw)
    ce = P.ClipEncoder(w, h, len(c), lib=LIB, **kw)
    (feed or (lambda e: e.upload(c)))(ce)
    out, sizes, _ = ce.encode()
    rec, qp = ce.read_lookahead()
    ce.close()
    return rec, qp, out, sizes


def same(rec, model):
    return all(np.array_equal(a, b) for a, b in zip(rec, model))


SHAPES = [(16, 16, "synth", 4), (16, 16, "noise", 4), (18, 18, "scene", 6), (18, 18, "noise", 4), (50, 38, "noise", 5), (50, 38, "synth", 5),
          (640, 16, "synth", 4), (640, 16, "still", 4), (16, 640, "still", 4), (16, 640, "scene", 6),
          (176, 144, "synth", 6), (176, 144, "scene", 6), (176, 144, "still", 4), (176, 144, "noise", 4)]


@pytest.mark.parametrize("w,h,clip,n", SHAPES, ids=["%dx%d_%s" % s[:3] for s in SHAPES])
def test_cost_records_equal_the_model(w, h, clip, n):
    """16x16: a single block; 18x18: a remainder that must be excluded; 50x38: slots at addresses that are 2 mod 4, an odd half-resolution
    size; 640x16 / 16x640: strips over several tiles"""
    P = pkg.load_pkg()
    c = clips.make(clip, w, h, n)
    model = M.costs(c, w, h)
    rec, _, _, _ = analyse(P, w, h, c)
    assert same(rec, model), (rec, model)
    assert rec[0][0] == rec[1][0] and rec[2][0] == 0, "frame 0: inter = intra"
    if clip == "still":
        still = [f for f in range(1, n) if np.array_equal(c[f][: w * h], c[f - 1][: w * h])]
        assert still and all(rec[1][f] == 0 and rec[2][f] == 0 for f in still)


def test_cost_records_do_not_depend_on_lane_order():
    P = pkg.load_pkg()
    w, h, n = 50, 38, 4
    c = clips.make("synth", w, h, n)
    ce = P.ClipEncoder(w, h, n, lib=pkg.EMU_REV_LIB, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload(c)
    ce.encode()
    rec, _ = ce.read_lookahead()
    ce.close()
    assert same(rec, M.costs(c, w, h))


@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_cost_records_on_device_input(fmt):
    P = pkg.load_pkg()
    w, h, n = 50, 38, 5
    mem = DevMem(LIB)
    try:
        feed, model_clip = _dev_feed(mem, clips.make("synth", w, h, n), w, h, fmt)
        rec, _, _, _ = analyse(P, w, h, model_clip, feed=feed)
        assert same(rec, M.costs(model_clip, w, h))
    finally:
        mem.close()


def test_bounded_ring_partial_windows_and_reupload():
    """a ring of four fed three frames at a time, windows of two: a window whose frames are not all there is not started (the call
    returns with what it encoded), and the records of frames whose pictures have left the ring stay"""
    P = pkg.load_pkg()
    w, h, n = 50, 38, 11
    c = clips.make("synth", w, h, n)
    rec1, qp1, want, want_sizes = analyse(P, w, h, c)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, resident=4, abr_kbps=100, lookahead=2)
    parts, sizes, per_call = [], [], []
    for f0 in range(0, n, 3):
        ce.upload(c[f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
        per_call.append(len(s))
    rec, qp = ce.read_lookahead()
    ce.close()
    assert per_call == [2, 4, 2, 3], "frames 2, 8: their window's second frame had not arrived"
    assert same(rec, M.costs(c, w, h)) and same(rec, rec1) and np.array_equal(qp, qp1)
    assert b"".join(parts) == want and sizes == want_sizes
    # whole-clip residency: frames 3.. replaced after a first pass
    c2 = c.copy()
    c2[3:] = clips.make("noise", w, h, n)[3:]
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload(c)
    ce.encode()
    ce.upload(c2[3:], first=3)
    changed, changed_sizes, _ = ce.encode()
    rec, qp = ce.read_lookahead()
    ce.close()
    rec2, qp2, want2, want2_sizes = analyse(P, w, h, c2)
    assert same(rec, M.costs(c2, w, h)) and np.array_equal(qp, qp2) and changed == want2 and changed_sizes == want2_sizes
    assert all(np.array_equal(a[:3], b[:3]) for a, b in zip(rec, rec1))


# ---- the controller

CTL = dict(w=176, h=144, n=24, gop=8, W=4, kbps=120)


def header_bits(P, w, h, c, **kw):
    ce = P.ClipEncoder(w, h, 1, lib=LIB, qp=26, **kw)
    ce.upload(c[:1])
    out, _, _ = ce.encode()
    ce.close()
    return 40, 40 + 8 * M.parameter_set_bytes(out)


@pytest.fixture(scope="module")
def controlled():
    """the controller's stream in one call, with what it read and chose"""
    P = pkg.load_pkg()
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    c = clips.make("synth", w, h, n)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, abr_kbps=kbps, lookahead=W)
    ce.upload(c)
    out, sizes, st = ce.encode()
    rec, qp = ce.read_lookahead()
    again, again_sizes, _ = ce.encode()         # a rewind resets k and carry and keeps records and settings
    rec2, qp2 = ce.read_lookahead()
    ce.close()
    assert again == out and again_sizes == sizes and same(rec, rec2) and np.array_equal(qp, qp2)
    return dict(P=P, clip=c, out=out, sizes=sizes, rounds=st.rounds, rec=rec, qp=qp)


def test_controller_qps_are_the_models_plan(controlled):
    d = controlled
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    assert same(d["rec"], M.costs(d["clip"], w, h))
    plan = M.plan(d["rec"], kinds, header_bits(d["P"], w, h, d["clip"]), [8 * s for s in d["sizes"]], kbps, W)
    assert np.array_equal(d["qp"], plan), (d["qp"], plan)
    assert len(set(d["qp"].tolist())) > 1, "the clip and the target make the controller move"
    assert d["rounds"] == n // W, "one launch per window"


def test_controller_stream_is_the_schedules_stream(controlled):
    d = controlled
    w, h, n, gop = (CTL[k] for k in ("w", "h", "n", "gop"))
    ce = d["P"].ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, qp_schedule=d["qp"])
    ce.upload(d["clip"])
    out, sizes, _ = ce.encode()
    ce.close()
    assert out == d["out"] and sizes == d["sizes"]


def test_controller_does_not_depend_on_the_call_pattern(controlled):
    d = controlled
    P = d["P"]
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    # three frames at a time
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, abr_kbps=kbps, lookahead=W)
    parts, sizes = [], []
    for f0 in range(0, n, 3):
        ce.upload(d["clip"][f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
    _, qp = ce.read_lookahead(costs=False)
    assert b"".join(parts) == d["out"] and sizes == d["sizes"] and np.array_equal(qp, d["qp"])
    # an output buffer that fills inside a window, after a rewind
    ce.L.H264E_clip_rewind(ce.c)
    cap = max(d["sizes"]) + sorted(d["sizes"])[n // 2] + 64
    parts, sizes, calls = [], [], 0
    while len(sizes) < n:
        out, s, _ = ce.encode(rewind=False, cap=cap)
        assert s, "a buffer that holds the largest frame always makes progress"
        parts.append(out)
        sizes += s
        calls += 1
    ce.close()
    assert calls > n // W, "the buffer filled inside windows"
    assert b"".join(parts) == d["out"] and sizes == d["sizes"]


def step_clip(w, h, n, W):
    """a window of noise, then a still picture: the unconstrained choice for the second window lies far below the first window's QP"""
    c = clips.make("noise", w, h, n)
    c[W:] = clips.make("synth", w, h, 1)[0]
    return c


def check_step_bound(P, lib):
    """the QP of a window stays within 6 of the window before it: a clip whose unconstrained plan jumps further, against M.plan with
    and without the bound"""
    w, h, n, W, kbps = 176, 144, 16, 4, 400
    c = step_clip(w, h, n, W)
    ce = P.ClipEncoder(w, h, n, lib=lib, gop=30, qp=30, abr_kbps=kbps, lookahead=W)
    ce.upload(c)
    out, sizes, _ = ce.encode()
    rec, qp = ce.read_lookahead()
    ce.close()
    kinds = [1] + [0] * (n - 1)
    ce = P.ClipEncoder(w, h, 1, lib=lib, qp=26)
    ce.upload(c[:1])
    hdr = (40, 40 + 8 * M.parameter_set_bytes(ce.encode()[0]))
    ce.close()
    bits = [8 * s for s in sizes]
    assert same(rec, M.costs(c, w, h))
    assert np.array_equal(qp, M.plan(rec, kinds, hdr, bits, kbps, W)), (qp, M.plan(rec, kinds, hdr, bits, kbps, W))
    free = M.plan(rec, kinds, hdr, bits, kbps, W, qp_step=51)
    # up to the first window where the two plans part they have the same history, so there `free` is the unconstrained choice
    a = int(np.flatnonzero(free != qp)[0])
    assert a >= W and a % W == 0
    assert abs(int(free[a]) - int(qp[a - W])) > M.QP_STEP, "without the bound this window would jump: %r" % (free,)
    assert abs(int(qp[a]) - int(qp[a - W])) == M.QP_STEP and (qp[a] > free[a]) == (qp[a - W] > free[a]), "the bound was hit: %r" % (qp,)
    assert all(abs(int(qp[a]) - int(qp[a - W])) <= M.QP_STEP for a in range(W, n, W))


def test_a_windows_qp_stays_within_the_step_of_the_window_before():
    check_step_bound(pkg.load_pkg(), LIB)


def test_default_window_and_qp_range():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 6
    c = clips.make("synth", w, h, n)
    _, qp, out, _ = analyse(P, w, h, c, abr_kbps=1, lookahead=0, qp_range=(20, 31))
    assert qp.tolist() == [31] * n                                  # nothing fits one kbit/s: qp_max; one window (the default, bounded by the clip)
    _, qp, _, _ = analyse(P, w, h, c, abr_kbps=100000, lookahead=0, qp_range=(20, 31))
    assert qp.tolist() == [20] * n
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, qp_schedule=[31] * n)
    ce.upload(c)
    assert ce.encode()[0] == out
    ce.close()


# ---- refusals

def test_refusals_leave_the_plain_stream():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 6
    c = clips.make("synth", w, h, n)

    def plain_of(**kw):
        ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, **kw)
        ce.upload(c)
        out = ce.encode()[0]
        ce.close()
        return out

    good = [30] * n
    # the reference's controller is on (kbps, qp 0), GOP shards
    for kw, word in ((dict(kbps=100), "kbps = 100"), (dict(qp=0), "qp = 0"), (dict(qp=30, keep_records=1), "keep_records")):
        plain = plain_of(**kw)
        ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, **kw)
        ce.upload(c)
        for call in (lambda: ce.set_qp_schedule(good), lambda: ce.set_lookahead(100, 2)):
            with pytest.raises(P.H264EError) as e:
                call()
            assert word in str(e.value), str(e.value)
            assert ce.encode()[0] == plain
            ce.L.H264E_clip_rewind(ce.c)
        ce.close()
        for extra in (dict(qp_schedule=good), dict(abr_kbps=100, lookahead=2)):
            with pytest.raises(P.H264EError):
                P.ClipEncoder(w, h, n, lib=LIB, gop=4, **dict(kw, **extra))
    # bad schedules, bad windows and ranges
    plain = plain_of(qp=30)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30)
    ce.upload(c)
    for bad, word in ((good[:-1], "5 values"), (good + [30], "7 values"), ([30, 30, 9, 30, 30, 30], "QP 9 of frame 2"), ([30, 30, 30, 30, 30, 52], "QP 52 of frame 5"),
                      ([30, 300, 30, 30, 30, 30], "QP 300 of frame 1"), ([-1, 30, 30, 30, 30, 30], "QP -1 of frame 0")):
        with pytest.raises(P.H264EError) as e:
            ce.set_qp_schedule(bad)
        assert word in str(e.value), str(e.value)
        assert ce.encode()[0] == plain
        ce.L.H264E_clip_rewind(ce.c)
    for args, word in (((100, n + 1), "window of %d" % (n + 1)), ((100, 2, (9, 30)), "9..30"), ((100, 2, (30, 52)), "30..52"), ((100, 2, (31, 30)), "31..30"), ((-1, 2), "bad argument")):
        with pytest.raises(P.H264EError) as e:
            ce.set_lookahead(*args)
        assert word in str(e.value), str(e.value)
        assert ce.encode()[0] == plain
        ce.L.H264E_clip_rewind(ce.c)
    assert ce.encode()[0] == plain
    for kw in (dict(qp=False), dict(costs=False)):
        with pytest.raises(P.H264EError):
            ce.read_lookahead(**kw)                                 # nothing was analysed, no frame has a QP
    ce.L.H264E_clip_rewind(ce.c)
    # the two exclude each other; clearing one admits the other
    ce.set_qp_schedule(good)
    with pytest.raises(P.H264EError):
        ce.set_lookahead(100, 2)
    ce.set_qp_schedule([])
    assert ce.encode()[0] == plain
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_lookahead(100, 2)
    with pytest.raises(P.H264EError):
        ce.set_qp_schedule(good)
    ce.set_lookahead(0)
    assert ce.encode()[0] == plain
    ce.close()
    # a window above a bounded input ring
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, resident=3)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead(100, 4)
    assert "input ring" in str(e.value)
    ce.close()
    # pictures below 16x16
    ce = P.ClipEncoder(14, 16, 2, lib=LIB, gop=4, qp=30)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead(100, 1)
    assert "16x16" in str(e.value)
    ce.close()
    # not at frame 0
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30)
    ce.upload(c[:3])
    part1 = ce.encode(rewind=False)[0]
    for call in (lambda: ce.set_qp_schedule(good), lambda: ce.set_lookahead(100, 2)):
        with pytest.raises(P.H264EError) as e:
            call()
        assert "frame 0" in str(e.value)
    ce.upload(c[3:], first=3)
    assert part1 + ce.encode(rewind=False)[0] == plain
    ce.close()


def test_without_the_new_calls_nothing_changes():
    """bytes from the reference's recorded stream (tests/golden/golden.json); launches and rounds as recorded on the commit before this
    feature (one launch, one round, no relaunch for 8 CIF frames in the emulation)"""
    P = pkg.load_pkg()
    g = next(x for x in GOLDEN if (x["clip"], x["w"], x["frames"], x["flags"]) == ("synth", 352, 8, "--qp 26 --gop 30"))
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=LIB, gop=30, qp=26)
    ce.upload(c)
    out, sizes, st = ce.encode(profile=True)
    ce.close()
    assert sizes == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"]
    assert (st.kernel_launches, st.rounds, st.reencoded_gops, st.frames, st.next_idr_pic_id_state) == (1, 1, 0, 8, 1)


# ---- the CLI

def _app(tmp_path, c, w, h, args, name="o.264", env=None):
    yuv = tmp_path / ("la_%dx%d.yuv" % (w, h))
    c.tofile(yuv)
    out = tmp_path / name
    r = subprocess.run([APP, "--input", str(yuv), "--output", str(out), "--stats", "x"] + args, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    return r, (out.read_bytes() if out.exists() else b"")


def test_cli_qpfile(tmp_path):
    case = CASES["qcif_gop5_forced"]
    w, h, gop = case["create"][:3]
    raw, _ = R.pictures(case)
    qpfile = tmp_path / "qp.txt"
    qpfile.write_text("\n".join(" ".join(str(q) for q in case["qp"][i:i + 4]) for i in range(0, len(case["qp"]), 4)) + "\n")
    base = ["--gop", str(gop), "--qp", "26", "--keyframes", ",".join(str(f) for f in case["forced"])]
    r, out = _app(tmp_path, raw, w, h, base + ["--qpfile", str(qpfile)])
    assert r.returncode == 0, r.stdout + r.stderr
    sizes = [int(l.split("bytes=")[1]) for l in r.stdout.splitlines() if l.startswith("frame=")]
    check_case(case, out, sizes, "--qpfile")
    assert "lookahead" not in r.stdout
    for text in ("30 30 30", " ".join(["30"] * 11), " ".join(["30"] * 9 + ["52"]), " ".join(["30"] * 9 + ["x"])):
        qpfile.write_text(text)
        r, _ = _app(tmp_path, raw, w, h, base + ["--qpfile", str(qpfile)], name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout, (text, r.stdout)
    for extra in (["--gpus", "2"], ["--clip", "0"], ["--kbps", "100"], ["--qpfile", str(tmp_path / "missing.txt")]):
        r, _ = _app(tmp_path, raw, w, h, base + ["--qpfile", str(qpfile)] + extra, name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout, (extra, r.stdout)


def test_cli_lookahead(tmp_path, controlled):
    d = controlled
    w, h, n, gop, W, kbps = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps"))
    base = ["--gop", str(gop), "--kbps", str(kbps)]
    want_line = "lookahead: window %d, QP %d..%d, %.1f kbps for a target of %d" % (W, d["qp"].min(), d["qp"].max(), sum(d["sizes"]) * 8.0 * 30.0 / n / 1000.0, kbps)
    # (a staging buffer of two frames and a ring of eight: the window's frames arrive in several uploads)
    for env in (None, dict(H264E_APP_STAGE_KB=str(2 * w * h * 3 // 2 // 1024 + 1), H264E_APP_RING_KB=str(8 * w * h * 3 // 2 // 1024 + 1))):
        r, out = _app(tmp_path, d["clip"], w, h, base + ["--lookahead", str(W)], env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        assert out == d["out"]
        assert [l for l in r.stdout.splitlines() if l.startswith("lookahead")] == [want_line]
    # --kbps alone stays the reference's controller
    P = d["P"]
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, kbps=kbps)
    ce.upload(d["clip"])
    ref_rc = ce.encode()[0]
    ce.close()
    r, out = _app(tmp_path, d["clip"], w, h, base)
    assert r.returncode == 0 and out == ref_rc and out != d["out"] and "lookahead" not in r.stdout
    for args in (base + ["--lookahead", str(W), "--gpus", "2"], base + ["--lookahead", str(W), "--clip", "0"], ["--gop", str(gop), "--qp", "30", "--lookahead", str(W)],
                 base + ["--lookahead", str(n + 1)]):
        r, _ = _app(tmp_path, d["clip"], w, h, args, name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout, (args, r.stdout)
