#!/usr/bin/env python3
"""Regenerate tests/golden/lookahead.json: how many bytes the REFERENCE's own rate control (oracle/_ref/encode_app_ref --kbps) writes for
the clips and targets of the lookahead controller's bitrate test -- the yardstick for its deviation from the target
(tests/test_gpu_lookahead.py).  Build container only; the output is data: clip, size, frames, flags, target and stream size.

    python tests/golden/make_golden_lookahead.py
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
REF = os.path.join(HERE, "..", "..", "oracle", "_ref", "encode_app_ref")

import clips  # noqa: E402

W, H, FRAMES, GOP = 352, 288, 128, 30
CASES = [(clip, kbps) for clip in ("synth", "pan") for kbps in (300, 1000)]


def main():
    if not os.access(REF, os.X_OK):
        sys.exit("make_golden_lookahead: %s is missing (the reference CLI, build container only): nothing written" % REF)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for clip, kbps in CASES:
            c = clips.make(clip, W, H, FRAMES)
            yuv = os.path.join(tmp, "c_%dx%d.yuv" % (W, H))
            c.tofile(yuv)
            o = os.path.join(tmp, "o.264")
            subprocess.run([REF, "--input", yuv, "--output", o, "--gop", str(GOP), "--kbps", str(kbps)], capture_output=True, text=True, check=True)
            data = open(o, "rb").read()
            out.append(dict(clip=clip, w=W, h=H, frames=FRAMES, gop=GOP, kbps=kbps, input_md5=hashlib.md5(c.tobytes()).hexdigest(), bytes=len(data)))
            print(clip, kbps, len(data), "%.1f kbps" % (len(data) * 8 * 30 / FRAMES / 1000))
    with open(os.path.join(HERE, "lookahead.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, sort_keys=True) for e in out) + "\n]\n")


if __name__ == "__main__":
    main()
