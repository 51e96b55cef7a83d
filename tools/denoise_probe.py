#!/usr/bin/env python3
"""What the temporal denoiser costs on the bench clip (1080p synth_v1, QP 26, GOP 30): clip encoder first pass (which runs the
denoise kernels) and rewound pass (which reuses the denoised pictures), and the per-frame API (H264E_encode), each with the denoiser
off and on, alternating, `--reps` times.  Prints one JSON line.  The kernel's own time per frame comes from a profiler run of this
tool, e.g.  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/denoise_probe.py --frames 120 --reps 1

    python tools/denoise_probe.py [--frames 600] [--perframe 60] [--reps 3]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30


def clip_passes(P, frames, denoise):
    enc = P.ClipEncoder(W, H, frames, gop=GOP, qp=QP, speed=0, denoise=denoise)
    enc.generate_synth(0, frames, t0=0, seed=1)
    t0 = time.time()
    out1, _, st1 = enc.encode()
    t1 = time.time()
    out2, _, st2 = enc.encode()
    t2 = time.time()
    enc.close()
    assert out1 == out2
    return dict(first_fps=frames / (t1 - t0), rewound_fps=frames / (t2 - t1), md5=hashlib.md5(out1).hexdigest(),
                spin_relaunches=st1.spin_relaunches + st2.spin_relaunches)


def host_frames(P, n):
    ce = P.ClipEncoder(W, H, n)
    ce.generate_synth()
    buf = np.empty((n, W * H * 3 // 2), np.uint8)
    ce.L.H264E_clip_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert ce.L.H264E_clip_download(ce.c, 0, n, buf.ctypes.data) == 0
    ce.close()
    return buf


def per_frame_fps(P, c, denoise):
    e = P.Encoder(W, H, gop=GOP, qp=QP, denoise=denoise)
    e.encode(c[0])
    t0 = time.time()
    for t in range(1, len(c)):
        e.encode(c[t])
    dt = time.time() - t0
    e.close()
    return (len(c) - 1) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--perframe", type=int, default=60)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    P = pkg.load_pkg()
    res = {"off": [], "on": []}
    for _ in range(a.reps):
        for mode in ("off", "on"):
            res[mode].append(clip_passes(P, a.frames, mode == "on"))
    c = host_frames(P, a.perframe) if a.perframe > 1 else None
    pf = {"off": [], "on": []}
    for _ in range(a.reps if c is not None else 0):
        for mode in ("off", "on"):
            pf[mode].append(per_frame_fps(P, c, mode == "on"))
    line = {"clip": "1080p synth_v1 x %d, QP %d, GOP %d" % (a.frames, QP, GOP), "reps": a.reps}
    for mode in ("off", "on"):
        line[mode] = {
            "first_pass_fps": statistics.median(r["first_fps"] for r in res[mode]),
            "rewound_pass_fps": statistics.median(r["rewound_fps"] for r in res[mode]),
            "per_frame_api_fps": statistics.median(pf[mode]) if pf[mode] else None,
            "md5": res[mode][0]["md5"], "spin_relaunches": sum(r["spin_relaunches"] for r in res[mode]),
            "samples_first": [round(r["first_fps"], 1) for r in res[mode]], "samples_rewound": [round(r["rewound_fps"], 1) for r in res[mode]],
            "samples_per_frame": [round(x, 2) for x in pf[mode]],
        }
    for k in ("first_pass_fps", "rewound_pass_fps", "per_frame_api_fps"):
        if line["off"][k] and line["on"][k]:
            line["cost_%s_pct" % k.replace("_fps", "")] = round(100.0 * (line["off"][k] / line["on"][k] - 1.0), 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
