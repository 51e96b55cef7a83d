#!/usr/bin/env python3
"""What the scaled device input costs (enc_scale.h, h264e_scale_kernel): HIP-event time per frame of H264E_clip_upload_device_scaled
for 3840x2160 -> 1920x1080, 1920x1080 -> 1280x720, 1920x1080 -> 640x360 and a 1920x1080 crop of 3840x2160, next to its yardstick, the
plain ingest (enc_ingest.h) of a 3840x2160 I420 frame, which reads the same 12.4 MB of source.  Every call hands over `--batch` frames
(distinct source tensors, one kernel launch each, back to back on the encoder's copy stream); the events are recorded on that stream
around the launches alone (H264E_clip_input_time).  `--warmup` calls are thrown away, the median of `--reps` calls is reported, the
cases alternate within every repetition.  The slot of the first frame of every case is compared with tests/scale_model.py before
anything is timed.  Prints one JSON line.

    python tools/scale_probe.py [--batch 8] [--reps 25] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402
import scale_model as M  # noqa: E402

CASES = [
    ("ingest_3840x2160", (3840, 2160), (3840, 2160), None),
    ("scale_3840x2160_to_1920x1080", (3840, 2160), (1920, 1080), None),
    ("scale_1920x1080_to_1280x720", (1920, 1080), (1280, 720), None),
    ("scale_1920x1080_to_640x360", (1920, 1080), (640, 360), None),
    ("crop_1920x1080_of_3840x2160", (3840, 2160), (1920, 1080), (960, 540, 1920, 1080)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    P = pkg.load_pkg()
    assert P.load().h264e_hip_device_count() > 0, "no HIP device visible"
    rng = np.random.default_rng(3)
    sources, runs = {}, []
    for size in sorted({c[1] for c in CASES}):
        w, h = size
        host = [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for _ in range(a.batch)]
        sources[size] = (host, [torch.from_numpy(x).cuda() for x in host])
    torch.cuda.synchronize()
    for name, size, (dw, dh), crop in CASES:
        host, dev = sources[size]
        ce = P.ClipEncoder(dw, dh, a.batch, gop=30, qp=26)
        kw = {} if name.startswith("ingest") else dict(src_size=size, crop=crop)
        ce.upload_device(dev, "i420", **kw)
        want = host[0].ravel() if name.startswith("ingest") else M.scale_frame(host[0], size[0], size[1], dw, dh, crop)
        assert np.array_equal(ce.download(0, 1)[0], want), name + ": the slot differs from the model"
        ce.input_time(True)
        runs.append((name, ce, dev, kw, []))
    for rep in range(a.warmup + a.reps):
        for name, ce, dev, kw, ms in runs:
            before = ce.input_time(True)
            ce.upload_device(dev, "i420", **kw)
            after = ce.input_time(True)
            assert after[1] - before[1] == a.batch
            if rep >= a.warmup:
                ms.append((after[0] - before[0]) / a.batch)
    line = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "us_per_frame": {}, "min_max_us": {}}
    for name, ce, _, _, ms in runs:
        ce.close()
        line["us_per_frame"][name] = round(1e3 * statistics.median(ms), 2)
        line["min_max_us"][name] = [round(1e3 * min(ms), 2), round(1e3 * max(ms), 2)]
    line["scale_4k_to_1080p_over_ingest_4k"] = round(line["us_per_frame"]["scale_3840x2160_to_1920x1080"] / line["us_per_frame"]["ingest_3840x2160"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
