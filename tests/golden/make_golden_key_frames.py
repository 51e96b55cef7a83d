#!/usr/bin/env python3
"""Regenerate tests/golden/key_frames.json: what the REFERENCE encoder answers, frame by frame, when H264E_encode is handed
H264E_FRAME_TYPE_KEY (6) on a list of forced frames and H264E_FRAME_TYPE_DEFAULT (0) on all others -- the streams the clip encoder must
write with H264E_clip_set_key_frames.  It writes scripts for oracle/_ref/api_harness and api_harness_thr (row-band slices), built by
`make -C oracle api`, in the format of tests/run_param_cases.py, and runs them on the CPU.  Build container only; the output is data: the
scripts themselves, the forced list and, per frame, size, md5 and key-frame flag.  Pictures are synth_v1 frames 0, 1, ...

    python tests/golden/make_golden_key_frames.py
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


def kf(w, h, gop, n, forced, q=30, kbps=0, speed=0, slices=1, den=0):
    """one case: n frames, KEY on `forced`; constant QP q or rate control at kbps (QP 10..50 as encode_app --kbps)"""
    fr = [G.F(G.K if t in forced else G.D, speed=speed, dfb=G.kbps(kbps)) if kbps else G.F(G.K if t in forced else G.D, speed=speed, q=q) for t in range(n)]
    c = G.case(w, h, gop, fr, cinp=1, den=den, slices=slices)
    c["forced"] = sorted(forced)
    c["clip"] = dict(qp=q, kbps=kbps, speed=speed)
    return c


CASES = {
    # CIF: forced key frames in the middle of a GOP; the periodic counter restarts there (frame 30 is a P frame, the next periodic key frame is 35 = 5 + 30)
    "cif_gop30_mid_gop": kf(352, 288, 30, 36, [2, 5], q=30),
    # a forced key frame one frame before a periodic one, and on one
    "qcif_gop8_before_and_on_periodic": kf(176, 144, 8, 30, [7, 23, 24], q=28),
    # two forced key frames in a row, then one right behind a periodic key
    "qcif_gop10_two_in_a_row": kf(176, 144, 10, 26, [4, 5, 15], q=33),
    # gop 1: the frame behind a forced key frame is a P frame (the counter wraps only on a DEFAULT call)
    "qcif_gop1_quirk": kf(176, 144, 1, 12, [3, 4, 8], q=30),
    # gop 0: frame 0 and the forced frames only; frame_num passes the 5-bit wrap between key frames
    "tiny_gop0": kf(64, 48, 0, 44, [5, 40], q=31),
    # rate control: the scheduled kind reaches rc_frame_start / rc_frame_end
    "cif_kbps300": kf(352, 288, 15, 24, [4, 16, 17], kbps=300),
    "qcif_kbps150_gop0": kf(176, 144, 0, 20, [9], kbps=150),
    # --qp 0: the controller over QP 10..51 without a byte target
    "qcif_qp0": kf(176, 144, 12, 18, [5, 6], q=0),
    # row-band slices
    "qcif_2_slices": kf(176, 144, 9, 20, [3, 8, 14], q=28, slices=2),
    "cif_8_slices_kbps400": kf(352, 288, 30, 16, [6, 7], kbps=400, slices=8),
    # the denoiser in front of forced key frames
    "qcif_denoise": kf(176, 144, 10, 18, [4, 9, 13], q=26, den=1),
    # a strip (one macroblock row), a tiny cropped picture, a cropped picture (const_input_flag = 1)
    "strip_640x16": kf(640, 16, 6, 16, [2, 5, 11], q=26),
    "tiny_cropped_34x18": kf(34, 18, 5, 16, [1, 2, 9], q=26),
    "cropped_200x120": kf(200, 120, 7, 18, [6, 10], q=30, speed=8),
}


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "api"], stdout=subprocess.DEVNULL)
    with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
        for name, c in CASES.items():
            G.run(name, c, tmp)
            w, h, gop = c["create"][:3]
            assert c["key"] == [int(k) for k in M.kinds(len(c["frames"]), gop, c["forced"])], (name, c["key"])
            print(name, c["create"], len(c["frames"]), c["bytes"])
    with open(os.path.join(HERE, "key_frames.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(CASES[k], sort_keys=True, separators=(",", ":")) for k in sorted(CASES)) + "\n}\n")


if __name__ == "__main__":
    main()
