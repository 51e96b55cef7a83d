#!/usr/bin/env python3
"""The initial calibration factors of the lookahead controller (LOOKAHEAD_K0_P / LOOKAHEAD_K0_KEY in h264e_host.c, K0 in
tests/lookahead_model.py), measured on the CPU: over synth, pan, scene and noise at CIF and QP 20 / 26 / 32 / 38 the median of

    ((coded bits - H) << 24) / (C * Lq[t][qp - 10])

per frame type, with the coded sizes from the oracle (the reference's bytes) and C from the numpy model of the cost pass.  Prints the
table that DESIGN.md 4.5k quotes.  --search R measures the same with the cost pass' motion search of range R
(tests/lookahead_motion_model.py): the P-frame median is LOOKAHEAD_K0_SEARCH / K0_SEARCH; the key-frame column does not move, I(f) is not
searched.

    python tools/lookahead_calibrate.py [frames] [gop] [--search R]

--step replays the controller instead (the model's plan, sizes from the oracle at the planned QPs) on the clip the search exists for: CIF,
still for its first half and sliding down 8 samples a frame afterwards, 128 frames, GOP 30, W = 16, 300 kbit/s, with the range given by
--search and without; prints per window the QP and the coded bits against the budget 8*dfb*W.

    python tools/lookahead_calibrate.py --step [--search R]

--step --tree S[+S..][,A] replays the controller with the cost tree's QP offsets instead (tests/lookahead_tree_model.py; A frames ahead,
default W) on CIF x 128 of synth, pan, scene and that still-then-sliding clip, GOP 30, W = 16, 300 kbit/s, once per strength and once
with strength 0 in the same run: total bits, mean and minimum luma PSNR of the oracle's reconstruction, and the per-frame PSNR around
the key frame at 30 and the window boundary at 32 (does quality pump?).  Prints the table that DESIGN.md 4.5n quotes.

    python tools/lookahead_calibrate.py --step --search 8 --tree 2+4+8,16
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clips  # noqa: E402
import lookahead_model as M  # noqa: E402
import lookahead_motion_model as ML  # noqa: E402
import lookahead_tree_model as MT  # noqa: E402
import oracle_lib  # noqa: E402
import scenecut_model  # noqa: E402


def oracle_bits(c, w, h, gop, qp):
    """coded bits per frame with a QP per frame: the oracle frame by frame with qp_min = qp_max = qp[f]"""
    e = oracle_lib.Encoder(w, h, gop=gop, qp=26)
    bits = []
    for f in range(len(qp)):
        assert oracle_lib.lib().h264o_set_run_param(e.e, 0, 0, 0, int(qp[f]), int(qp[f]), 0) == 0
        bits.append(8 * len(e.encode(c[f])))
    e.close()
    return bits


def step_report(search):
    w, h, n, gop, W, kbps = 352, 288, 128, 30, 16, 300
    c = clips.vpan(w, h, n, 8, lambda t: t >= n // 2)
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    hdr = (40, 40 + 8 * M.parameter_set_bytes(oracle_lib.encode_clip(c[:1], w, h, gop=gop, qp=26)[0]))
    budget = 8 * (kbps * 1000 // 8 // 30) * W
    rows = {}
    for R in (0, search):
        cost = ML.costs(c, w, h, R)
        bits, qp = [], []
        for a in range(0, n, W):
            # the plan reads the sizes of finished windows only: what lies behind window a does not matter yet
            plan = ML.plan(cost, kinds, hdr, bits + [0] * (n - len(bits)), kbps, W, search=R)
            qp += plan[a:a + W].tolist()
            bits = oracle_bits(c, w, h, gop, qp)
        rows[R] = [(qp[a], sum(bits[a:a + W])) for a in range(0, n, W)]
        print("range %d: %d bits for a target of %d" % (R, sum(bits), 8 * (kbps * 1000 // 8 // 30) * n))
    print("| window | frames | QP, no search | bits / budget | QP, search %d | bits / budget |" % search)
    print("|---|---|---|---|---|---|")
    for j in range(n // W):
        (q0, b0), (q1, b1) = rows[0][j], rows[search][j]
        print("| %d | %d..%d | %d | %d / %d = %.2f | %d | %d / %d = %.2f |" % (j, j * W, j * W + W - 1, q0, b0, budget, b0 / budget, q1, b1, budget, b1 / budget))


def tree_report(search, strengths, ahead):
    w, h, n, gop, W, kbps = 352, 288, 128, 30, 16, 300
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    target = 8 * (kbps * 1000 // 8 // 30) * n
    shown = (28, 29, 30, 31, 32, 33)
    print("| clip | strength | bits | bits / target | mean PSNR-Y | min PSNR-Y | offsets of window 1 | base QPs | PSNR-Y of frames %s |" % ", ".join(str(f) for f in shown))
    print("|---|---|---|---|---|---|---|---|---|")
    for name in ("synth", "pan", "scene", "vpan"):
        c = clips.vpan(w, h, n, 8, lambda t: t >= n // 2) if name == "vpan" else clips.make(name, w, h, n)
        hdr = (40, 40 + 8 * M.parameter_set_bytes(oracle_lib.encode_clip(c[:1], w, h, gop=gop, qp=26)[0]))
        rec, fields, intra = MT.analyse(c, w, h, search)
        for s in [0] + strengths:
            deltas = MT.windows(rec, fields, intra, kinds, W, s, ahead)[2] if s else np.zeros(n, np.int8)
            e = oracle_lib.Encoder(w, h, gop=gop, qp=26)
            bits, psnr, base = [], [], []
            for a in range(0, n, W):
                qp, bq = MT.plan(rec, kinds, hdr, bits + [0] * (n - len(bits)), kbps, W, deltas, search=search)
                base.append(int(bq[a]))
                for f in range(a, min(a + W, n)):
                    assert oracle_lib.lib().h264o_set_run_param(e.e, 0, 0, 0, int(qp[f]), int(qp[f]), 0) == 0
                    bits.append(8 * len(e.encode(c[f])))
                    buf, cw, ch = e.recon()
                    d = buf[: cw * ch].reshape(ch, cw)[:h, :w].astype(np.int64) - c[f][: w * h].reshape(h, w)
                    mse = float((d * d).mean())
                    psnr.append(10 * np.log10(255.0 * 255.0 / mse) if mse else 99.0)
            e.close()
            print("| %s | %d | %d | %.3f | %.2f | %.2f | %s | %s | %s |" % (name, s, sum(bits), sum(bits) / target, np.mean(psnr), np.min(psnr), deltas[W:2 * W].tolist(), base,
                                                                       " ".join("%.2f" % psnr[f] for f in shown)))


def main():
    argv = sys.argv[1:]
    search = 0
    tree = None
    if "--tree" in argv:
        i = argv.index("--tree")
        tree = argv[i + 1].split(",")
        del argv[i:i + 2]
    if "--search" in argv:
        i = argv.index("--search")
        search = int(argv[i + 1])
        del argv[i:i + 2]
    if "--step" in argv and tree:
        return tree_report(search or ML.MAX_RANGE, [int(v) for v in tree[0].split("+")], int(tree[1]) if len(tree) > 1 else 16)
    if "--step" in argv:
        return step_report(search or ML.MAX_RANGE)
    n = int(argv[0]) if len(argv) > 0 else 24
    gop = int(argv[1]) if len(argv) > 1 else 8
    w, h = 352, 288
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    ratios = {0: [], 1: []}
    print("| clip | QP | median k, P frames | median k, key frames |")
    print("|---|---|---|---|")
    for name in ("synth", "pan", "scene", "noise"):
        c = clips.make(name, w, h, n)
        cost = ML.costs(c, w, h, search) if search else M.costs(c, w, h)
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
