#!/usr/bin/env python3
"""Regenerate tests/golden/launch_plan.json: for the configurations of tests/launch_plan_cases.py, what the host side of the device
boundary (h264-lab_amd/csrc/h264e_pool.h) decides for every launch -- window geometry, kernel variant, jobs, workgroups, a hash of the
dispatch order, active jobs -- as the emulation's launch function logs it (H264E_EMU_LAUNCH_LOG).  This project's own data, no GPU
needed.  A change of this file is a change of BEHAVIOUR (pick_variant's thresholds, the band policy, the frames per launch): a
refactor of the pool leaves it byte for byte as it is.

    python tests/golden/make_golden_launch_plan.py
"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import launch_plan_cases as L  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu")], stdout=subprocess.DEVNULL)
    out = {}
    for name in L.CASES:
        t0 = time.time()
        out[name] = L.run(name)
        print("%-28s %3d launches, variants %s, %.1f s" % (name, len(out[name]), sorted({ln.split()[1] for ln in out[name]}), time.time() - t0))
    with open(os.path.join(HERE, "launch_plan.json"), "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(out[k], indent=1) for k in sorted(out)) + "\n}\n")


if __name__ == "__main__":
    main()
