#!/usr/bin/env python3
"""What float planar RGB costs and saves at 1080p, in both directions, next to the 8-bit path and to what a caller wrote before.  One
process measures these cases, ALTERNATING them inside every repetition (so that drift hits all alike):

  plain_in_<t>    H264E_clip_upload_device of 1920x1080 frames: t = u8 ("rgbp") and, with --float, f16 / bf16 / f32 ("rgbpf")
  scaled_in_<t>   the same from 3840x2160 frames through a window (H264E_clip_upload_device_scaled)
  out_<t>         H264E_clip_read_recon_device of every encoded frame into a (3, 1080, 1920) tensor
  *_<t>_two_step  with --float, the two steps the float formats replace, inside the same timed region: torch's
                  (x * 255).round().clamp(0, 255).to(uint8) and "rgbp" on the way in; the "rgbp" read and (u8.float() / 255).to(dtype)
                  on the way out

Per case, microseconds per frame over --frames frames per call and --reps repetitions after one that warms up: "kernel" = HIP events
around the ingest / scale / egress launches alone (H264E_clip_input_time, H264E_clip_output_time; the two-step cases show their 8-bit
launch there, torch's kernels only in the wall column), "wall" = the host clock around the call through the binding, between two device
synchronisations; median, minimum and maximum.  --lib PATH measures another build of the library (the parent commit's, for the 8-bit
cases) through this binding.  With --float it also checks each float destination against the IEEE definition and counts for how many
of the 256 values torch's own device-side division differs from it.  Prints a table and writes everything as JSON to --out.

    python tools/float_io_probe.py --float --out new.json
    python tools/float_io_probe.py --lib /path/to/parent/libh264e_mi355x.so --out parent.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import float_model as FM  # noqa: E402
import pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--float", action="store_true")
ap.add_argument("--out", required=True)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--frames", type=int, default=8)
a = ap.parse_args()
import torch
P = pkg.load_pkg()
kw = dict(lib=a.lib) if a.lib else {}
W, H, SW, SH, N = 1920, 1080, 3840, 2160, a.frames
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
g = torch.Generator(device="cuda"); g.manual_seed(1)
src8 = {"plain": [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2)],
        "scaled": [torch.randint(0, 256, (3, SH, SW), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2)]}
srcf = {}
if a.float:
    for k, dt in DT.items():
        for geo in src8:
            srcf[(geo, k)] = [(t.cpu().float() / 255).to(dt).cuda() for t in src8[geo]]
torch.cuda.synchronize()
quant = lambda t: (t * 255).round().clamp(0, 255).to(torch.uint8)
enc = {"plain": P.ClipEncoder(W, H, N, gop=30, qp=26, **kw), "scaled": P.ClipEncoder(W, H, N, gop=30, qp=26, **kw)}
out_ce = P.ClipEncoder(W, H, N, gop=30, qp=26, **kw)
out_ce.generate_synth(); out_ce.encode()
outs = {"u8": torch.empty((3, H, W), dtype=torch.uint8, device="cuda")}
for k, dt in DT.items():
    outs[k] = torch.empty((3, H, W), dtype=dt, device="cuda")

cases = []      # (name, function returning (wall seconds, kernel ms or None))
def in_case(geo, name, frames_fn, fmt):
    ce = enc[geo]; win = dict(src_size=(SW, SH)) if geo == "scaled" else {}
    def run():
        ms0, n0 = ce.input_time(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ce.upload_device(frames_fn(), fmt, **win)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        ms1, n1 = ce.input_time(False)
        return t1 - t0, (ms1 - ms0)
    cases.append(("%s_in_%s" % (geo, name), run))
def out_case(name, fmt, out, post):
    def run():
        ms0, n0 = out_ce.output_time(True)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for f in range(N):
            out_ce.read_recon_device(f, fmt, out=out)
            if post: r = post(out)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        ms1, n1 = out_ce.output_time(False)
        return t1 - t0, (ms1 - ms0)
    cases.append(("out_%s" % name, run))
for geo in ("plain", "scaled"):
    in_case(geo, "u8", lambda geo=geo: [src8[geo][i % 2] for i in range(N)], "rgbp")
    if a.float:
        for k in DT:
            in_case(geo, k, lambda geo=geo, k=k: [srcf[(geo, k)][i % 2] for i in range(N)], "rgbpf")
            in_case(geo, k + "_two_step", lambda geo=geo, k=k: [quant(srcf[(geo, k)][i % 2]) for i in range(N)], "rgbp")
out_case("u8", "rgbp", outs["u8"], None)
if a.float:
    for k, dt in DT.items():
        out_case(k, "rgbpf", outs[k], None)
        out_case(k + "_two_step", "rgbp", outs["u8"], lambda o, dt=dt: (o.float() / 255).to(dt))

res = {name: {"wall_us": [], "kernel_us": []} for name, _ in cases}
for rep in range(a.reps + 1):
    for name, run in cases:
        wall, ms = run()
        if rep:     # the first repetition warms up
            res[name]["wall_us"].append(round(1e6 * wall / N, 2)); res[name]["kernel_us"].append(round(1e3 * ms / N, 2))
for name in res:
    for k in ("wall_us", "kernel_us"):
        v = res[name][k]; res[name][k + "_median"] = statistics.median(v); res[name][k + "_min"] = min(v); res[name][k + "_max"] = max(v)
extra = {}
if a.float:     # correctness spot checks and one figure: how torch divides on the device
    u8 = outs["u8"]; out_ce.read_recon_device(0, "rgbp", out=u8)
    for k, dt in DT.items():
        out_ce.read_recon_device(0, "rgbpf", out=outs[k])
        assert torch.equal(outs[k], (u8.cpu().float() / 255).to(dt).cuda()), k
    v = torch.arange(256, device="cuda", dtype=torch.uint8)
    dev = (v.float() / 255).cpu().numpy().view(np.uint32)
    extra["torch_device_division_differs_from_ieee_for"] = int((dev != FM.table("f32")).sum())
json.dump({"lib": a.lib or "product", "frames": N, "reps": a.reps, "cases": res, "extra": extra}, open(a.out, "w"), indent=1)
print("wrote", a.out, extra)
for name in res:
    print("%-32s wall %8.1f us/frame  kernel %8.1f us/frame" % (name, res[name]["wall_us_median"], res[name]["kernel_us_median"]))
