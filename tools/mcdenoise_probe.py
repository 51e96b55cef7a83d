#!/usr/bin/env python3
"""What the motion-compensated temporal denoiser costs and saves on the bench clip (1080p synth_v1, QP 26, GOP 30): the clip encoder with
the filter off, with the plain denoiser, and with H264E_clip_set_denoise_motion 1 and 2 (lookahead search range 8, controller off),
the modes alternating in one process, `--reps` times, medians.  Per mode: first-pass fps (which runs the pre-pass kernels), rewound fps
(which reuses the pictures), coded bytes on that clip and on its first `--noisy-frames` frames with hash noise of amplitude 6 added,
and the HIP-event time per frame of the filter's and the cost pass' launches.  A second part runs the three pre-pass kernels alone
through the device layer, `--loop` frames back to back between two stream syncs, so that the plain denoiser's kernel (which the library
does not time) stands next to the others from the same run.  Writes profiles/mcdenoise_probe.json and prints the same line.

    python tools/mcdenoise_probe.py [--frames 600] [--noisy-frames 120] [--reps 3] [--loop 320]
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
import mcdenoise_model  # noqa: E402
import pkg  # noqa: E402

W, H, QP, GOP, R = 1920, 1080, 26, 30, 8
MODES = {"off": dict(), "plain": dict(denoise=True), "motion1": dict(lookahead_search=R, denoise_motion=1), "motion2": dict(lookahead_search=R, denoise_motion=2)}


def clip_passes(P, frames, kw, host=None):
    enc = P.ClipEncoder(W, H, frames, gop=GOP, qp=QP, speed=0, **kw)
    if host is None:
        enc.generate_synth(0, frames, t0=0, seed=1)
    else:
        enc.upload(host)
    t0 = time.time()
    out1, _, st1 = enc.encode()
    t1 = time.time()
    out2, _, st2 = enc.encode()
    t2 = time.time()
    mc_ms, mc_n = enc.denoise_time()
    la_ms, la_n = enc.lookahead_time()
    enc.close()
    assert out1 == out2
    return dict(first_fps=frames / (t1 - t0), rewound_fps=frames / (t2 - t1), bytes=len(out1), md5=hashlib.md5(out1).hexdigest(),
                spin_relaunches=st1.spin_relaunches + st2.spin_relaunches, mc_us=1000.0 * mc_ms / mc_n if mc_n else None,
                la_us=1000.0 * la_ms / la_n if la_n else None)


def host_frames(P, n):
    ce = P.ClipEncoder(W, H, n)
    ce.generate_synth()
    buf = np.empty((n, W * H * 3 // 2), np.uint8)
    ce.L.H264E_clip_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    assert ce.L.H264E_clip_download(ce.c, 0, n, buf.ctypes.data) == 0
    ce.close()
    return buf


def kernels_alone(P, c, loop):
    """us per frame of each pre-pass kernel, `loop` frames back to back through the device layer (16 per call, the ring's length)"""
    L = P.load()
    L.h264e_hip_pool_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_pool_destroy.argtypes = [C.c_void_p]
    L.h264e_hip_pool_destroy.restype = None
    L.h264e_hip_upload_i420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.h264e_hip_denoise_reset.argtypes = [C.c_void_p]
    L.h264e_hip_denoise_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_lookahead_search_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.h264e_hip_mcdenoise_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_sync.argtypes = [C.c_void_p]
    n = 16
    pool = C.c_void_p()
    assert L.h264e_hip_pool_create(C.byref(pool), 0, W, H, 1, n) == 0
    out = {}
    try:
        part = np.ascontiguousarray(c[:n])
        assert L.h264e_hip_upload_i420(pool, 0, n, part.ctypes.data) == 0 and L.h264e_hip_denoise_reset(pool) == 0
        rec = np.zeros((n, 3), np.uint64)
        calls = max(loop // n, 1)
        # the frames keep their ring slots, so call k filters "frames" 16k.. of a clip that repeats every 16 frames
        runs = {"cost_pass_search8": lambda k: L.h264e_hip_lookahead_search_frames(pool, n * k, n, R, rec.ctypes.data, None),
                "plain_denoiser": lambda k: L.h264e_hip_denoise_frames(pool, 0, n, int(k == 0)),
                "motion1": lambda k: L.h264e_hip_mcdenoise_frames(pool, n * k, n, 1, int(k == 0)),
                "motion2": lambda k: L.h264e_hip_mcdenoise_frames(pool, n * k, n, 2, int(k == 0))}
        for name, run in runs.items():
            assert run(0) == 0 and L.h264e_hip_sync(pool) == 0
            t0 = time.time()
            for k in range(1, calls + 1):
                assert run(k) == 0
            assert L.h264e_hip_sync(pool) == 0
            out[name] = round(1e6 * (time.time() - t0) / (calls * n), 2)
    finally:
        L.h264e_hip_pool_destroy(pool)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--noisy-frames", type=int, default=120)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop", type=int, default=320)
    a = ap.parse_args()
    P = pkg.load_pkg()
    res = {m: [] for m in MODES}
    for _ in range(a.reps):
        for m, kw in MODES.items():
            res[m].append(clip_passes(P, a.frames, kw))
    clean = host_frames(P, max(a.noisy_frames, 16))
    noisy = np.stack([mcdenoise_model.hash_noise(f, salt=77 + i) for i, f in enumerate(clean[: a.noisy_frames])]) if a.noisy_frames else None
    line = {"clip": "1080p synth_v1 x %d, QP %d, GOP %d, lookahead search %d" % (a.frames, QP, GOP, R), "reps": a.reps, "noisy_frames": a.noisy_frames}
    for m, kw in MODES.items():
        r = res[m]
        line[m] = {
            "first_pass_fps": round(statistics.median(x["first_fps"] for x in r), 1), "rewound_pass_fps": round(statistics.median(x["rewound_fps"] for x in r), 1),
            "samples_first": [round(x["first_fps"], 1) for x in r], "samples_rewound": [round(x["rewound_fps"], 1) for x in r],
            "bytes": r[0]["bytes"], "md5": r[0]["md5"], "same_stream_every_rep": len({x["md5"] for x in r}) == 1, "spin_relaunches": sum(x["spin_relaunches"] for x in r),
            "filter_kernel_us_per_frame": round(statistics.median(x["mc_us"] for x in r), 3) if r[0]["mc_us"] is not None else None,
            "cost_pass_kernel_us_per_frame": round(statistics.median(x["la_us"] for x in r), 3) if r[0]["la_us"] is not None else None,
        }
        if noisy is not None:
            x = clip_passes(P, a.noisy_frames, kw, host=noisy)
            line[m]["noisy_bytes"] = x["bytes"]
            line[m]["clean_bytes_same_frames"] = clip_passes(P, a.noisy_frames, kw, host=clean[: a.noisy_frames])["bytes"]
    line["kernels_alone_us_per_frame"] = kernels_alone(P, clean, a.loop)
    text = json.dumps(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    open(os.path.join(ROOT, "profiles", "mcdenoise_probe.json"), "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
