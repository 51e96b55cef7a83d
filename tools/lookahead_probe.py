#!/usr/bin/env python3
"""What bitrate targeting costs on the bench clip (1080p synth_v1 x 600, GOP 30, target 4000 kbit/s), three ways in ONE process: the
lookahead window controller (H264E_clip_set_lookahead: this project's own QP choice), the reference's controller (kbps = 4000: every
frame's QP follows the frame before it) and constant QP 26.  Per mode: fps of a first pass (which runs the cost pass) and of a rewound
pass, launches, frames encoded again, achieved bitrate and QP range; for the window controller the cost pass' kernel time per frame
from HIP events (H264E_clip_lookahead_time) and a sweep of the window over 8 / 16 / 32 / 64.  Prints one JSON line.

--search R adds a fourth mode behind the first, the window controller with the cost pass' motion search of range R
(H264E_clip_set_lookahead_search), in the same process and order, and leaves the window sweep out: what the search costs per frame and
in first-pass fps against the same run without it (profiles/lookahead_motion_probe.json).

--tree S[,A] (with --search) adds a fifth mode behind that one, the searched controller with the cost tree of strength S and A frames
ahead (H264E_clip_set_lookahead_tree; A left out = the default), alternating with the others in the same process: the tree's kernel time
per frame step from HIP events (H264E_clip_lookahead_tree_time) and first-pass fps with the tree on and off
(profiles/lookahead_tree_probe.json).

    python tools/lookahead_probe.py [--frames 600] [--reps 3] [--kbps 4000] [--search R] [--tree S[,A]]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30


def clip_passes(P, frames, **kw):
    enc = P.ClipEncoder(W, H, frames, gop=GOP, speed=0, **kw)
    enc.generate_synth(0, frames, t0=0, seed=1)
    t0 = time.perf_counter()
    out1, _, st1 = enc.encode()
    t1 = time.perf_counter()
    out2, _, st2 = enc.encode()
    t2 = time.perf_counter()
    r = dict(first_fps=frames / (t1 - t0), rewound_fps=frames / (t2 - t1), md5=hashlib.md5(out1).hexdigest(), launches=st2.rounds, encoded_again=st2.reencoded_gops,
             spin_relaunches=st1.spin_relaunches + st2.spin_relaunches, kbps=len(out1) * 8 * 30 / frames / 1000.0)
    if kw.get("abr_kbps"):
        ms, analysed = enc.lookahead_time()
        qp = enc.read_lookahead(costs=False)[1]
        r.update(kernel_us_per_frame=1e3 * ms / analysed if analysed else None, analysed=analysed, qp_range=[int(qp.min()), int(qp.max())])
    if kw.get("lookahead_tree"):
        ms, steps = enc.lookahead_tree_time()
        _, delta, base = enc.read_lookahead_tree_sums()
        r.update(tree_kernel_us_per_step=1e3 * ms / steps if steps else None, tree_steps=steps, offset_range=[int(delta.min()), int(delta.max())],
                 base_qp_range=[int(base.min()), int(base.max())])
    enc.close()
    assert out1 == out2
    return r


def summary(rs):
    s = {"first_pass_fps": round(statistics.median(r["first_fps"] for r in rs), 1), "rewound_pass_fps": round(statistics.median(r["rewound_fps"] for r in rs), 1),
         "samples_first": [round(r["first_fps"], 1) for r in rs], "samples_rewound": [round(r["rewound_fps"], 1) for r in rs],
         "launches": rs[0]["launches"], "launches_after_a_stop": rs[0]["encoded_again"], "kbps": round(rs[0]["kbps"], 1), "md5": rs[0]["md5"],
         "same_stream_every_rep": len({r["md5"] for r in rs}) == 1, "spin_relaunches": sum(r["spin_relaunches"] for r in rs)}
    if "qp_range" in rs[0]:
        s.update(qp_range=rs[0]["qp_range"], cost_pass_kernel_us_per_frame=round(statistics.median(r["kernel_us_per_frame"] for r in rs), 3), frames_analysed=rs[0]["analysed"])
    if "tree_steps" in rs[0]:
        s.update(tree_kernel_us_per_frame_step=round(statistics.median(r["tree_kernel_us_per_step"] for r in rs), 3), tree_frame_steps=rs[0]["tree_steps"],
                 offset_range=rs[0]["offset_range"], base_qp_range=rs[0]["base_qp_range"])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kbps", type=int, default=4000)
    ap.add_argument("--search", type=int, default=0)
    ap.add_argument("--tree", default="")
    a = ap.parse_args()
    if a.tree and not a.search:
        ap.error("--tree needs --search")
    P = pkg.load_pkg()
    modes = {"lookahead_w32": dict(qp=QP, abr_kbps=a.kbps, lookahead=32)}
    if a.search:
        modes["lookahead_w32_search"] = dict(qp=QP, abr_kbps=a.kbps, lookahead=32, lookahead_search=a.search)
    if a.tree:
        modes["lookahead_w32_search_tree"] = dict(modes["lookahead_w32_search"], lookahead_tree=tuple(int(v) for v in a.tree.split(",")))
    modes.update({"reference_kbps": dict(kbps=a.kbps), "constant_qp": dict(qp=QP)})
    for m in ("lookahead_w32", "lookahead_w32_search", "lookahead_w32_search_tree")[:3 if a.tree else 2 if a.search else 1]:
        clip_passes(P, min(a.frames, 64), **modes[m])                     # warm-up: code objects, page tables
    res = {m: [] for m in modes}
    for _ in range(a.reps):
        for m, kw in modes.items():
            res[m].append(clip_passes(P, a.frames, **kw))
    line = {"clip": "1080p synth_v1 x %d, GOP %d, target %d kbit/s, constant QP %d" % (a.frames, GOP, a.kbps, QP), "reps": a.reps}
    for m in modes:
        line[m] = summary(res[m])
    if a.search:
        off, on = line["lookahead_w32"], line["lookahead_w32_search"]
        line["search"] = {"range": a.search, "cost_pass_us_per_frame_over_without": round(on["cost_pass_kernel_us_per_frame"] / off["cost_pass_kernel_us_per_frame"], 2),
                          "first_pass_fps_over_without": round(on["first_pass_fps"] / off["first_pass_fps"], 3),
                          "first_pass_spread_without": round((max(off["samples_first"]) - min(off["samples_first"])) / off["first_pass_fps"], 3)}
        if a.tree:
            tr = line["lookahead_w32_search_tree"]
            line["tree"] = {"strength_ahead": a.tree, "first_pass_fps_over_search_alone": round(tr["first_pass_fps"] / on["first_pass_fps"], 3),
                            "rewound_pass_fps_over_search_alone": round(tr["rewound_pass_fps"] / on["rewound_pass_fps"], 3),
                            "first_pass_spread_search_alone": round((max(on["samples_first"]) - min(on["samples_first"])) / on["first_pass_fps"], 3)}
    else:
        line["window_sweep"] = {str(w): summary([clip_passes(P, a.frames, qp=QP, abr_kbps=a.kbps, lookahead=w)]) for w in (8, 16, 32, 64)}
    line["lookahead_over_reference_kbps_rewound"] = round(line["lookahead_w32"]["rewound_pass_fps"] / line["reference_kbps"]["rewound_pass_fps"], 2)
    line["lookahead_over_reference_kbps_first"] = round(line["lookahead_w32"]["first_pass_fps"] / line["reference_kbps"]["first_pass_fps"], 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
