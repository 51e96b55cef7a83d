#!/usr/bin/env python3
"""What the device-side quality metrics cost at 1080p (synth_v1, QP 26, GOP 30, the clip resident in HBM), by the method of DESIGN.md 4.5d:
`--warmup` calls are thrown away, the median of `--reps` calls is reported with their minimum and maximum, the cases alternate within
every repetition.  One clip encoder, `--frames` frames, encoded again and again with

  - off:       no metric (no launch, no allocation),
  - ssd:       the sums of squared differences (h264e_ssd_kernel, the parent commit's kernel), and
  - ssd_ssim:  the sums and the SSIM (h264e_ssim_kernel + h264e_ssim_mean_kernel, enc_ssim.h) --

reporting per case the clip throughput by wall clock around H264E_clip_encode (frames per second), and for the two metrics the HIP-event
time per frame around their launches alone (H264E_clip_quality_time), on the same frames, with their ratio.  The last frame's values are
compared with tests/ssim_model.py.  Prints one JSON line.

    python tools/quality_probe.py [--frames 60] [--reps 25] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402
import ssim_model as SM  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30
CASES = [("off", dict(ssd=False, ssim=False)), ("ssd", dict(ssd=True, ssim=False)), ("ssd_ssim", dict(ssd=True, ssim=True))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    P = pkg.load_pkg()
    ce = P.ClipEncoder(W, H, a.frames, gop=GOP, qp=QP)
    ce.generate_synth()
    fps = {name: [] for name, _ in CASES}
    ssd_us = {name: [] for name, _ in CASES[1:]}
    ssim_us = []
    streams = set()
    for rep in range(a.warmup + a.reps):
        for name, q in CASES:
            ce.set_quality(**q)
            a0, b0, n0 = ce.quality_time(True)
            t0 = time.perf_counter()
            out, sizes, _ = ce.encode()
            t1 = time.perf_counter()
            a1, b1, n1 = ce.quality_time(False)
            assert len(sizes) == a.frames and n1 - n0 == (0 if name == "off" else a.frames)
            streams.add(hash(out))
            if rep < a.warmup:
                continue
            fps[name].append(a.frames / (t1 - t0))
            if name != "off":
                ssd_us[name].append(1e3 * (a1 - a0) / a.frames)
            if name == "ssd_ssim":
                ssim_us.append(1e3 * (b1 - b0) / a.frames)
    assert len(streams) == 1, "the metrics changed the stream"
    ssd, ssim = ce.read_quality()
    f = a.frames - 1
    inp, rec = ce.download(f, 1)[0], ce.read_recon(f)
    want = SM.frame(inp, rec, W, H)
    assert [int(v) for v in ssd[f]] == SM.frame_ssd(inp, rec, W, H)
    assert all(abs(ssim[f][k] - want[k]) <= SM.tolerance(W >> (k > 0), H >> (k > 0)) for k in range(3))
    ce.close()

    def stat(v, digits):
        return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}

    line = {"clip": "1080p synth_v1, QP %d, GOP %d, resident" % (QP, GOP), "frames": a.frames, "reps": a.reps, "warmup": a.warmup,
            "fps": {name: stat(v, 1) for name, v in fps.items()},
            "ssd_kernel_us_per_frame": {name: stat(v, 2) for name, v in ssd_us.items()},
            "ssim_kernels_us_per_frame": stat(ssim_us, 2),
            "ssim_over_ssd": round(statistics.median(ssim_us) / statistics.median(ssd_us["ssd_ssim"]), 3) if statistics.median(ssd_us["ssd_ssim"]) else None,
            "last_frame_ssim": [float(v) for v in ssim[f]], "last_frame_ssim_hex": [float(v).hex() for v in ssim[f]]}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
