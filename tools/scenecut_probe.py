#!/usr/bin/env python3
"""What scene-cut detection costs on the bench clip (1080p synth_v1 x 600, QP 26, GOP 30; the clip has no cuts, so the stream is the
same with the detector on): the detector's own time per frame from HIP events around its kernel launches (H264E_clip_scenecut_time;
the first pass of a fresh encoder analyses every frame, warm-up encoder first), and the clip encoder's throughput with the detector off
and on, alternating, `--reps` times: first pass (which runs the detector's kernels and reads the records back) and rewound pass (which
reuses the records).  Prints one JSON line.

    python tools/scenecut_probe.py [--frames 600] [--reps 3]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30


def clip_passes(P, frames, scenecut):
    enc = P.ClipEncoder(W, H, frames, gop=GOP, qp=QP, speed=0, scenecut=scenecut)
    enc.generate_synth(0, frames, t0=0, seed=1)
    t0 = time.perf_counter()
    out1, _, st1 = enc.encode()
    t1 = time.perf_counter()
    out2, _, st2 = enc.encode()
    t2 = time.perf_counter()
    ms, analysed = enc.scenecut_time()
    cuts = int(enc.read_scenecut()[1].sum()) if scenecut else 0
    enc.close()
    assert out1 == out2
    return dict(first_fps=frames / (t1 - t0), rewound_fps=frames / (t2 - t1), md5=hashlib.md5(out1).hexdigest(), cuts=cuts,
                spin_relaunches=st1.spin_relaunches + st2.spin_relaunches, kernel_us_per_frame=1e3 * ms / analysed if analysed else None, analysed=analysed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    P = pkg.load_pkg()
    clip_passes(P, min(a.frames, 60), P.H264E_SCENECUT_DEFAULT)         # warm-up: code objects, page tables
    res = {"off": [], "on": []}
    for _ in range(a.reps):
        for mode in ("off", "on"):
            res[mode].append(clip_passes(P, a.frames, P.H264E_SCENECUT_DEFAULT if mode == "on" else 0))
    line = {"clip": "1080p synth_v1 x %d, QP %d, GOP %d" % (a.frames, QP, GOP), "reps": a.reps}
    for mode in ("off", "on"):
        line[mode] = {
            "first_pass_fps": round(statistics.median(r["first_fps"] for r in res[mode]), 1),
            "rewound_pass_fps": round(statistics.median(r["rewound_fps"] for r in res[mode]), 1),
            "md5": res[mode][0]["md5"], "spin_relaunches": sum(r["spin_relaunches"] for r in res[mode]),
            "samples_first": [round(r["first_fps"], 1) for r in res[mode]], "samples_rewound": [round(r["rewound_fps"], 1) for r in res[mode]],
        }
    on = res["on"]
    line["detector_kernel_us_per_frame"] = round(statistics.median(r["kernel_us_per_frame"] for r in on), 3)
    line["detector_samples_us"] = [round(r["kernel_us_per_frame"], 3) for r in on]
    line["frames_analysed"] = on[0]["analysed"]
    line["cuts"] = on[0]["cuts"]
    line["same_stream"] = line["on"]["md5"] == line["off"]["md5"]
    for k in ("first_pass_fps", "rewound_pass_fps"):
        line["cost_%s_pct" % k.replace("_fps", "")] = round(100.0 * (line["off"][k] / line["on"][k] - 1.0), 2)
    off = sorted(r["first_fps"] for r in res["off"])
    line["off_spread_first_pass_pct"] = round(100.0 * (off[-1] / off[0] - 1.0), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
