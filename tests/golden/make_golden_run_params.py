#!/usr/bin/env python3
"""Regenerate tests/golden/run_params.json: what the REFERENCE encoder answers, frame by frame, when the H264E_run_param_t of
H264E_encode changes from call to call (h264-lab.h:6701-6775, :6497, :6611) -- frame_type DEFAULT / P / KEY, encode_speed,
desired_frame_bytes, the QP window, run_param == NULL, H264E_set_vbv_state in front of a frame.  oracle/api_harness.c is a translation
unit that includes the reference header and calls its public API (`make -C oracle api`).  Build container only; the output is data:
the scripts themselves and, per line, size, md5, key-frame flag and (const_input_flag = 0) the md5 of the planes written back.

Lines with a frame type the product refuses (I, DROPPABLE, GOLDEN, RECOVERY, CUSTOM) are NOT given to the reference: the recorded stream
is the reference's stream without those calls, which is what the product must produce with them (the refusal moves nothing).  What those
frame types CODE in the reference is outside the product by decision, so no script here depends on it; a divergence that only such a
feature could close does not belong in this fixture.

Not scripted, because the reference itself cannot answer: run_param == NULL with temporal_denoise_flag (h264-lab.h:6686 reads opt before
:6701 replaces a NULL one), NULL on the first call, const_input_flag = 0 on a cropped picture (the reconstruction of the coded size is
written over the caller's smaller planes)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "api_harness")
HARNESS_THR = os.path.join(ROOT, "oracle", "_ref", "api_harness_thr")

D, P, K = 0, 2, 6
I_, DROPPABLE, GOLDEN, RECOVERY, CUSTOM = 5, 1, 4, 3, 99
VBV = 100000 // 8


def F(ft=D, speed=0, dfb=0, q=None, qmin=10, qmax=50, vbv=None, null=0):
    """one line; q: constant QP (qp_min = qp_max = q)"""
    if q is not None:
        qmin = qmax = q
    return [ft, speed, dfb, qmin, qmax] + (list(vbv) if vbv else [-1, -1]) + [null]


def kbps(k):
    return k * 1000 // 8 // 30


def case(w, h, gop, frames, vbv=VBV, cinp=1, den=0, slices=1):
    return dict(create=[w, h, gop, vbv, cinp, den, slices], frames=frames)


OVER = (12500, 40000)         # fullness far above the size: h264-lab.h:6497-6498 holds for any desired_frame_bytes used here


def overflow_on_key_frames(cinp, slices=1):
    # gop 12 at 200 kbps: overflow events on frame 0, on the GOP-boundary key frame 12, on a forced KEY (17, which restarts the GOP: next
    # DEFAULT key frame is 29), on the P frame 20 (transparent) and again on the key frame 29
    fr = []
    for t in range(32):
        fr.append(F(K if t == 17 else D, dfb=kbps(200), vbv=OVER if t in (0, 12, 17, 20, 29) else None))
    return case(176, 144, 12, fr, cinp=cinp, slices=slices)


def forced_key(then_p):
    fr = []
    for t in range(24):
        ft = K if t == 5 else (P if then_p and 6 <= t <= 15 else D)
        fr.append(F(ft, q=28))
    return case(176, 144, 8, fr, cinp=0)


def explicit_p():
    # P on every frame across the GOP boundary (10) and the 5-bit frame_num wrap (32); back to DEFAULT at 36: frame_num is past the GOP,
    # so 36 is still a P frame, the counter restarts behind it (h264-lab.h:6611) and 37 is a key frame
    return case(64, 48, 10, [F(D, q=26)] + [F(P, q=26) for _ in range(35)] + [F(D, q=26) for _ in range(4)], cinp=0)


def cqp_changes(w, h, cinp):
    # key frames (gop 4: 0, 4, 8, ...) at q below and above 30: pic_init_qp clamp (h264-lab.h:6768-6770) and the sign of slice_qp_delta;
    # 0 (window 10..51), 5 (qp_min repaired to 10, above qp_max 5) and 60 (qp_max repaired to 51, below qp_min 60): h264-lab.h:6707-6715
    qs = [24, 26, 33, 40, 36, 30, 18, 51, 0, 12, 5, 60, 60, 29, 31, 10, 5, 44, 45, 46]
    fr = [F(q=q) for q in qs] + [F(qmin=40, qmax=20), F(qmin=40, qmax=20), F(qmin=35, qmax=12), F(qmin=35, qmax=12), F(qmin=20, qmax=40), F(qmin=9, qmax=52)]
    return case(w, h, 4, fr, cinp=cinp)


def speed_changes(slices=1):
    sp = [0, 1, 2, 8, 9, 10, 10, 9, 8, 2, 1, 0, 8, 0, 10, 1, 9, 2, 0, 0, 8, 8, 1, 10]
    return case(176, 144, 7, [F(speed=s, q=30) for s in sp], cinp=0 if slices == 1 else 1, slices=slices)


def rc_steps():
    return case(352, 288, 15, [F(dfb=kbps(300 if t < 10 else 600 if t < 20 else 150)) for t in range(30)])


def cqp_rc_cqp():
    return case(176, 144, 10, [F(q=30) for _ in range(8)] + [F(dfb=kbps(200)) for _ in range(12)] + [F(q=26) for _ in range(8)], cinp=0)


def rc_window():
    win = [(10, 50)] * 6 + [(20, 40)] * 6 + [(28, 32)] * 6 + [(30, 30)] * 3 + [(34, 38)] * 3 + [(10, 51)] * 4
    return case(176, 144, 9, [F(dfb=kbps(150), qmin=a, qmax=b) for a, b in win])


def null_run_param():
    fr = [F(dfb=kbps(200), speed=1)] + [F(null=1) for _ in range(5)]
    fr += [F(K, dfb=kbps(300)), F(null=1), F(null=1)]          # the stored copy says KEY: every NULL call is a key frame
    fr += [F(P, q=32, speed=8), F(null=1), F(null=1), F(D, q=27), F(null=1), F(null=1), F(null=1), F(null=1, vbv=OVER), F(null=1)]
    return case(176, 144, 6, fr, cinp=0)


def denoiser(cinp):
    # speeds below 2 (denoised) and above (raw, state kept), a forced KEY, and a transparent frame: the denoiser runs in front of it
    sp = [0, 1, 0, 2, 0, 9, 1, 0, 0, 8, 0, 1, 0, 0, 2, 1, 0, 0]
    fr = [F(K if t == 7 else D, speed=s, dfb=kbps(200), vbv=OVER if t in (12, 15) else None) for t, s in enumerate(sp)]
    return case(176, 144, 10, fr, cinp=cinp, den=1)


def refusals():
    # refused calls: in front of the first key frame, in a GOP, in front of a GOP-boundary key frame, twice in a row, in front of a NULL call
    q = dict(q=29)
    fr = [F(GOLDEN, **q), F(D, **q), F(D, **q), F(I_, **q), F(D, **q), F(DROPPABLE, speed=9, q=40), F(null=1), F(D, **q), F(RECOVERY, **q), F(CUSTOM, **q),
          F(D, **q), F(D, **q), F(I_, dfb=kbps(100)), F(D, **q), F(K, **q), F(CUSTOM, q=20), F(null=1), F(P, **q), F(DROPPABLE, **q), F(D, **q), F(D, **q), F(D, **q)]
    return case(176, 144, 5, fr, cinp=0)


def big(which):
    fr = []
    for t in range(12):
        if which == 0:
            fr.append(F(K if t == 5 else D, speed=0 if t < 7 else 8, dfb=kbps(4000 if t < 4 else 1500)))
        else:
            fr.append(F(K if t == 8 else P if 2 <= t <= 4 else D, speed=[9, 2, 0, 1][t // 3], dfb=kbps(2500 if t < 6 else 8000), qmin=16, qmax=44))
    return case(1920, 1080, 6 if which else 30, fr, vbv=500000, slices=1 if which == 0 else 4)


NAMED = {
    "overflow_on_key_frames_recon": overflow_on_key_frames(0),
    "overflow_on_key_frames_const_input": overflow_on_key_frames(1),
    "overflow_on_key_frames_2_slices": overflow_on_key_frames(1, slices=2),
    "forced_key_then_default": forced_key(False),
    "forced_key_then_explicit_p": forced_key(True),
    "explicit_p_across_gop_and_frame_num_wrap": explicit_p(),
    "gop_0_40_frames": case(64, 48, 0, [F(q=31, speed=t % 3) for t in range(40)], cinp=0),
    "cqp_changes_every_frame": cqp_changes(176, 144, 0),
    "cqp_changes_every_frame_cropped": cqp_changes(200, 120, 1),
    "speed_changes_every_frame": speed_changes(),
    "speed_changes_every_frame_3_slices": speed_changes(3),
    "rc_bitrate_steps_cif": rc_steps(),
    "cqp_rc_cqp": cqp_rc_cqp(),
    "rc_qp_window_narrows": rc_window(),
    "null_run_param": null_run_param(),
    "denoiser_mixed_speeds_const_input": denoiser(1),
    "denoiser_mixed_speeds_recon": denoiser(0),
    "refused_frame_types": refusals(),
    "hd1080_key_speed_bitrate": big(0),
    "hd1080_4_slices_key_speed_bitrate": big(1),
}


def _lcg(seed):
    s = seed & 0xffffffff
    while True:
        s = (s * 1664525 + 1013904223) & 0xffffffff
        yield s >> 8


def random_cases(n, seed):
    r = _lcg(seed)
    out = {}
    sizes = [(64, 48), (96, 80), (128, 96), (176, 144), (200, 120), (130, 70), (320, 240), (352, 288)]
    speeds = [0, 0, 1, 2, 8, 9, 10]
    for k in range(n):
        w, h = sizes[next(r) % len(sizes)]
        frames = 12 + next(r) % (9 if w * h > 320 * 200 else 29)
        gop = [0, 1, 2, 3, 5, 8, 12, 30][next(r) % 8]
        cropped = bool((w | h) & 15)
        cinp = 1 if cropped else next(r) % 2
        den = next(r) % 5 == 0
        slices = 2 + next(r) % 3 if next(r) % 5 == 0 else 1
        slices = min(slices, (h + 15) // 16)            # more row bands than macroblock rows: the product's split differs by design
        vbv = [VBV, VBV, 6000, 40000][next(r) % 4]
        cur = None
        fr = []
        for t in range(frames):
            if cur is None or next(r) % 3 == 0:         # new run parameters
                if next(r) % 2:
                    a, b = 10 + next(r) % 42, 10 + next(r) % 42
                    if next(r) % 4:
                        a, b = min(a, b), max(a, b)
                    cur = dict(speed=speeds[next(r) % 7], dfb=kbps(30 + next(r) % 600), qmin=a, qmax=b)
                else:
                    cur = dict(speed=speeds[next(r) % 7], q=[0, 5, 60][next(r) % 3] if next(r) % 8 == 0 else 10 + next(r) % 42)
            x = next(r) % 100
            ft = D if t == 0 or x < 72 else K if x < 80 else P if x < 96 else [I_, DROPPABLE, GOLDEN, RECOVERY, CUSTOM][next(r) % 5]
            refused = ft not in (D, P, K)
            null = 1 if (t > 0 and not den and not refused and next(r) % 8 == 0) else 0
            ev = None
            if not refused and vbv and next(r) % 12 == 0:
                size = [vbv, 6000, 25000][next(r) % 3]
                ev = (size, [-1, 0, size // 2, size * 3][next(r) % 4])
            fr.append(F(ft, vbv=ev, null=null, **cur))
        if fr[-1][0] not in (D, P, K):
            fr[-1][0] = D
        out["random_%02d" % k] = case(w, h, gop, fr, vbv=vbv, cinp=cinp, den=int(den), slices=slices)
    return out


def run(name, c, tmp):
    import run_param_cases as R
    w, h, gop, vbv, cinp, den, slices = c["create"]
    assert c["frames"][0][0] != P and not c["frames"][0][7] and c["frames"][-1][0] in R.ACCEPTED
    assert cinp or not ((w | h) & 15)
    assert slices <= (h + 15) // 16
    for l in c["frames"]:
        assert not (den and l[7]) and (l[0] in R.ACCEPTED or l[5] < 0)
    path = os.path.join(tmp, "script.txt")
    open(path, "w").write(R.script_text(c))
    out = os.path.join(tmp, "o.264")
    r = subprocess.run([HARNESS_THR if slices > 1 else HARNESS, path, out], capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    assert len(lines) == len(c["frames"]), (name, r.stdout, r.stderr)
    c["sizes"], c["md5"], c["key"] = [], [], []
    if not cinp:
        c["recon_md5"] = []
    for l in lines:
        d = dict(x.split("=") for x in l.split() if "=" in x)
        if l.endswith("refused"):
            c["sizes"].append(-1); c["md5"].append(""); c["key"].append(0)
            if not cinp:
                c["recon_md5"].append("")
            continue
        assert d["status"] == "0", (name, l)
        c["sizes"].append(int(d["bytes"])); c["md5"].append(d["md5"]); c["key"].append(int(d["key"]))
        if not cinp:
            c["recon_md5"].append(d["recon"])
    data = open(out, "rb").read()
    c["bytes"], c["stream_md5"] = len(data), hashlib.md5(data).hexdigest()
    assert c["bytes"] == sum(s for s in c["sizes"] if s > 0)
    return c


def main():
    import run_param_cases as R
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "api"], stdout=subprocess.DEVNULL)
    cases = dict(NAMED)
    cases.update(random_cases(40, 20260))
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        for name, c in cases.items():
            run(name, c, tmp)
            print(name, c["create"], len(c["frames"]), c["bytes"])
    cov = R.check_coverage(cases)
    print(cov)
    with open(os.path.join(HERE, "run_params.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(cases[k], sort_keys=True, separators=(",", ":")) for k in sorted(cases)) + "\n}\n")


if __name__ == "__main__":
    main()
