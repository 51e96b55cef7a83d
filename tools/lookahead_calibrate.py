#!/usr/bin/env python3
"""The initial calibration factors of the lookahead controller (LOOKAHEAD_K0_P / LOOKAHEAD_K0_KEY in h264e_host.c, K0 in
tests/lookahead_model.py), measured on the CPU: over synth, pan, scene and noise at CIF and QP 20 / 26 / 32 / 38 the median of

    ((coded bits - H) << 24) / (C * Lq[t][qp - 10])

per frame type, with the coded sizes from the oracle (the reference's bytes) and C from the numpy model of the cost pass.  Prints the
table that DESIGN.md 4.5k quotes.

    python tools/lookahead_calibrate.py [frames] [gop]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clips  # noqa: E402
import lookahead_model as M  # noqa: E402
import oracle_lib  # noqa: E402
import scenecut_model  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    gop = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    w, h = 352, 288
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    ratios = {0: [], 1: []}
    print("| clip | QP | median k, P frames | median k, key frames |")
    print("|---|---|---|---|")
    for name in ("synth", "pan", "scene", "noise"):
        c = clips.make(name, w, h, n)
        cost = M.costs(c, w, h)
        for qp in (20, 26, 32, 38):
            stream, sizes = oracle_lib.encode_clip(c, w, h, gop=gop, qp=qp)
            hdr = (40, 40 + 8 * M.parameter_set_bytes(stream))
            row = {0: [], 1: []}
            for f in range(n):
                t = kinds[f]
                den = int(cost[0][f] if t else cost[1][f]) * M.LQ[t][qp - 10]
                if den:
                    row[t].append((max(8 * sizes[f] - hdr[t], 0) << 24) // den)
            for t in (0, 1):
                ratios[t] += row[t]
            print("| %s | %d | %d | %d |" % (name, qp, np.median(row[0]), np.median(row[1])))
    print("| all | | **%d** | **%d** |" % (np.median(ratios[0]), np.median(ratios[1])))


if __name__ == "__main__":
    main()
