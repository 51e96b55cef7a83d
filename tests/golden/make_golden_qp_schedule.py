#!/usr/bin/env python3
"""Regenerate tests/golden/qp_schedule.json: what the REFERENCE encoder answers, frame by frame, when H264E_encode is handed
qp_min = qp_max = qp[f] and desired_frame_bytes = 0 on frame f -- the streams the clip encoder must write with
H264E_clip_set_qp_schedule.  It writes scripts for oracle/_ref/api_harness and api_harness_thr (row-band slices), built by
`make -C oracle api`, in the format of tests/run_param_cases.py, and runs them on the CPU.  Build container only; the output is data: the
scripts themselves, the QP and forced lists and, per frame, size, md5 and key-frame flag.  Pictures are synth_v1 frames 0, 1, ...
Without both harness binaries nothing is written.

    python tests/golden/make_golden_qp_schedule.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import make_golden_run_params as G  # noqa: E402  (the script runner and the line format)
import scenecut_model as M  # noqa: E402


def qs(w, h, gop, qp, forced=(), speed=0, slices=1, den=0):
    """one case: len(qp) frames, frame f at constant QP qp[f], KEY on `forced`"""
    fr = [G.F(G.K if t in forced else G.D, speed=speed, q=q) for t, q in enumerate(qp)]
    c = G.case(w, h, gop, fr, cinp=1, den=den, slices=slices)
    c["forced"] = sorted(forced)
    c["qp"] = list(qp)
    c["clip"] = dict(speed=speed)
    return c


CASES = {
    # the QP moves every frame (no two neighbours are equal) and reaches both ends; key frames (0, 4, 8) at 24 < 30, 51 > 30 and 10: pic_init_qp follows the key frame,
    # slice_qp_delta of the P frames behind it has both signs
    "tiny_gop4_every_frame": qs(64, 48, 4, [24, 30, 10, 44, 51, 36, 27, 45, 10, 11, 40, 29]),
    # a forced key frame (3) at a QP above 30 between periodic ones (0, 8) at QPs below
    "qcif_gop5_forced": qs(176, 144, 5, [22, 25, 31, 38, 35, 33, 30, 28, 26, 41], forced=[3]),
    "qcif_2_slices": qs(176, 144, 4, [28, 34, 20, 45, 33, 32, 18, 30], slices=2),
    "qcif_denoise": qs(176, 144, 6, [26, 30, 35, 24, 40, 28, 33, 21], den=1),
    "tiny_cropped_34x18": qs(34, 18, 3, [30, 12, 48, 25, 37, 31, 29, 50]),
}


def main():
    for path in (G.HARNESS, G.HARNESS_THR):
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "api"], stdout=subprocess.DEVNULL)
            break
    for path in (G.HARNESS, G.HARNESS_THR):
        if not os.access(path, os.X_OK):
            sys.exit("make_golden_qp_schedule: %s is missing (the reference harness, build container only): nothing written" % path)
    with tempfile.TemporaryDirectory() as tmp:
        for name, c in CASES.items():
            G.run(name, c, tmp)
            gop = c["create"][2]
            assert c["key"] == [int(k) for k in M.kinds(len(c["frames"]), gop, c["forced"])], (name, c["key"])
            assert all(s > 0 for s in c["sizes"]), name
            print(name, c["create"], len(c["frames"]), c["bytes"])
    with open(os.path.join(HERE, "qp_schedule.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(CASES[k], sort_keys=True, separators=(",", ":")) for k in sorted(CASES)) + "\n}\n")


if __name__ == "__main__":
    main()
