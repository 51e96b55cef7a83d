#!/usr/bin/env python3
"""Regenerate tests/golden/side_by_side.json: what the REFERENCE encoder writes for the fresh clips of the side-by-side tests
(tests/test_oracle.py: test_oracle_vs_compiled_reference, test_oracle_row_bands_vs_compiled_reference; tests/test_emu_cli.py:
test_psnr_line_equals_reference), so that those tests check against the reference also where oracle/_ref is not built.

Runs only in the build container: it executes oracle/_ref/encode_app_ref and encode_app_ref_thr (`make -C oracle ref`).  The
fixture is data: md5 and length of every stream, and the reference's PSNR line."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clips  # noqa: E402
import oracle_lib  # noqa: E402
import synth  # noqa: E402

# the parameters of the tests named above
QPS = [10, 18, 26, 34, 42, 51]
MODES = ["--gop 30", "--gop 2 --speed 1", "--gop 30 --speed 9"]
ROW_BANDS = [(2, "--qp 26 --gop 30"), (3, "--qp 40 --gop 2"), (5, "--qp 18 --gop 30 --speed 2"), (8, "--kbps 200 --gop 30")]
PSNR_FLAGS = ["--qp", "26", "--gop", "5", "--psnr", "x"]


def _run(app, c, w, h, args, tmp):
    yuv = os.path.join(tmp, "c_%dx%d.yuv" % (w, h))
    c.tofile(yuv)
    out = os.path.join(tmp, "o.264")
    r = subprocess.run([app, "--input", yuv, "--output", out] + args, check=True, capture_output=True, text=True)
    data = open(out, "rb").read()
    return {"md5": hashlib.md5(data).hexdigest(), "bytes": len(data)}, r.stdout


def main():
    res = {"oracle_vs_ref": {}, "row_bands": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for qp in QPS:
            for mode in MODES:
                flags = ("--qp %d " % qp) + mode
                res["oracle_vs_ref"][flags], _ = _run(oracle_lib.REF_APP, synth.clip(128, 96, 5, seed=qp), 128, 96, flags.split(), tmp)
        for slices, flags in ROW_BANDS:
            c = clips.make("pan", 176, 144, 5) if slices == 3 else synth.clip(176, 144, 5, seed=slices)
            res["row_bands"]["%s --threads %d" % (flags, slices)], _ = _run(oracle_lib.REF_APP_THR, c, 176, 144, flags.split() + ["--threads", str(slices)], tmp)
        s, stdout = _run(oracle_lib.REF_APP, clips.make("synth", 176, 144, 12), 176, 144, PSNR_FLAGS, tmp)
        s["psnr_line"] = [l for l in stdout.splitlines() if "YPSNR" in l]
        res["psnr"] = s
    with open(os.path.join(HERE, "side_by_side.json"), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote tests/golden/side_by_side.json")


if __name__ == "__main__":
    main()
