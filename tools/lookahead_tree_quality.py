#!/usr/bin/env python3
"""What the cost tree's QP offsets (H264E_clip_set_lookahead_tree) do to quality at equal target, on the GPU: CIF x 128 of synth, pan,
scene and the still-then-sliding clip of tools/lookahead_calibrate.py --step, GOP 30, W = 16, 300 kbit/s, search 8, strength 0 / 2 / 4 / 8
with the default frames ahead, all in one process.  Per clip and strength: total bits against the target, mean and minimum luma PSNR and
mean luma SSIM from the device metrics (quality=True), the first window's offsets, the base QPs, and the per-frame luma PSNR around the
key frame at 30 and the window boundary at 32.  Prints one JSON line per row (profiles/lookahead_tree_probe.json).

    python tools/lookahead_tree_quality.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clips  # noqa: E402
import pkg  # noqa: E402

W, H, N, GOP, WINDOW, KBPS, SEARCH = 352, 288, 128, 30, 16, 300, 8
SHOWN = (28, 29, 30, 31, 32, 33)


def main():
    P = pkg.load_pkg()
    target = 8 * (KBPS * 1000 // 8 // 30) * N
    for name in ("synth", "pan", "scene", "vpan"):
        c = clips.vpan(W, H, N, 8, lambda t: t >= N // 2) if name == "vpan" else clips.make(name, W, H, N)
        for s in (0, 2, 4, 8):
            ce = P.ClipEncoder(W, H, N, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=WINDOW, lookahead_search=SEARCH, lookahead_tree=s, quality=True)
            ce.upload(c)
            out, sizes, _ = ce.encode()
            ssd, ssim = ce.read_quality()
            _, qp = ce.read_lookahead(costs=False)
            delta, base = (ce.read_lookahead_tree_sums()[1:] if s else (np.zeros(N, np.int8), qp))
            ce.close()
            psnr = 10 * np.log10(255.0 * 255.0 * W * H / np.maximum(ssd[:, 0].astype(np.float64), 1e-9))
            print(json.dumps({"clip": name, "strength": s, "bits": 8 * len(out), "bits_over_target": round(8 * len(out) / target, 3),
                              "mean_psnr_y": round(float(psnr.mean()), 2), "min_psnr_y": round(float(psnr.min()), 2), "mean_ssim_y": round(float(ssim[:, 0].mean()), 4),
                              "offsets_window_1": delta[WINDOW:2 * WINDOW].tolist(), "base_qp": base[::WINDOW].tolist(),
                              "psnr_y_frames_%d_%d" % (SHOWN[0], SHOWN[-1]): [round(float(psnr[f]), 2) for f in SHOWN]}))


if __name__ == "__main__":
    main()
