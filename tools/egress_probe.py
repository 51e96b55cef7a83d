#!/usr/bin/env python3
"""What device-resident output costs and saves at 1080p (synth_v1, QP 26, GOP 30).  Per format (I420, NV12, RGB of 3 and 4 bytes per
pixel, planar RGB into a CHW tensor with the default matrix and with BT.709 full range; with --fmt also float planar RGB, "rgbp_f16" /
"rgbp_bf16" / "rgbp_f32", and "rgbp_f16_via_divide" / ...: the 8-bit planar read followed by torch's (u8.float() / 255).to(dtype), the
two steps the float formats replace, whose call_us holds both and whose kernel_us the egress alone): the time per frame of
H264E_clip_read_recon_device into a torch tensor, over `--frames` encoded frames and `--reps` repetitions --

  - kernel_us: the HIP-event time around the egress launch alone (H264E_clip_output_time), and
  - c_call_us: the host wall clock around the C call alone with a prepared H264E_dev_frame_t, which ends in a device synchronise (the
    memory check, events, launch, kernel, wait), and
  - call_us: the same around the binding's read_recon_device, which describes the tensor anew for every call --

next to the only way there was before, timed by the same loop: H264E_clip_read_recon to host memory (a blocking device-to-host copy of
the coded-size I420 picture) plus the upload of that picture to a torch tensor (host_roundtrip_us, the two parts given separately; the
crop and the colour conversion a caller would still have to do on the way are NOT in it).  The first repetition warms up and is dropped.
Every format's first frame is compared with the model (tests/egress_model.py).  Prints one JSON line.

    python tools/egress_probe.py [--frames 8] [--reps 5] [--fmt i420,rgbp,rgbp_f32,rgbp_f32_via_divide,...]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import egress_model as EM  # noqa: E402
import float_model as FM  # noqa: E402
import pkg  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30
CW, CH = (W + 15) // 16 * 16, (H + 15) // 16 * 16
FORMATS = [("i420", "i420", 3, None), ("nv12", "nv12", 3, None), ("rgb3", "rgb", 3, None), ("rgb4", "rgb", 4, None), ("rgbp", "rgbp", 3, None),
           ("rgbp_bt709_full", "rgbp", 3, "bt709-full")]
FLOAT_FORMATS = [("rgbp_" + k + v, "rgbp" if v else "rgbp_" + k, 3, None) for k in FM.KINDS for v in ("", "_via_divide")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fmt", default=",".join(f[0] for f in FORMATS), help="comma-separated, of: %s" % ", ".join(f[0] for f in FORMATS + FLOAT_FORMATS))
    a = ap.parse_args()
    known = {f[0]: f for f in FORMATS + FLOAT_FORMATS}
    for f in a.fmt.split(","):
        if f not in known:
            ap.error("--fmt %s: one of %s" % (f, ", ".join(known)))
    import torch
    P = pkg.load_pkg()
    line = {"clip": "1080p synth_v1, QP %d, GOP %d" % (QP, GOP), "frames": a.frames, "reps": a.reps, "formats": {}}
    for name, fmt, pb, color in [known[f] for f in a.fmt.split(",")]:
        kind = name.split("_")[1] if (name, fmt, pb, color) in FLOAT_FORMATS else None
        dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, None: None}[kind]
        ce = P.ClipEncoder(W, H, a.frames, gop=GOP, qp=QP, color=color)
        ce.generate_synth()
        ce.encode()
        out = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda") if name == "rgb4" else P.recon_out(fmt, W, H)
        torch.cuda.synchronize()
        kernel_us, call_us, c_call_us, d2h_us, h2d_us = [], [], [], [], []
        desc, _keep = P.dev_frame(out, fmt, W, H)
        for _ in range(a.reps + 1):                     # the first repetition warms up (code object, page tables, pinned staging)
            ms0, n0 = ce.output_time(True)
            t0 = time.perf_counter()
            for f in range(a.frames):
                ce.read_recon_device(f, fmt, out=out)
                if name.endswith("_via_divide"):
                    res = (out.float() / 255).to(dtype)
            if name.endswith("_via_divide"):
                torch.cuda.synchronize()
            t1 = time.perf_counter()
            ms1, n1 = ce.output_time(False)
            assert n1 - n0 == a.frames
            kernel_us.append(1e3 * (ms1 - ms0) / a.frames)
            call_us.append(1e6 * (t1 - t0) / a.frames)
            t0 = time.perf_counter()
            for f in range(a.frames):
                assert ce.L.H264E_clip_read_recon_device(ce.c, f, ctypes.byref(desc)) == 0
            c_call_us.append(1e6 * (time.perf_counter() - t0) / a.frames)
            d2h = h2d = 0.0
            for f in range(a.frames):
                t0 = time.perf_counter()
                host = ce.read_recon(f)
                t1 = time.perf_counter()
                dev = torch.from_numpy(host).cuda()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                d2h += t1 - t0
                h2d += t2 - t1
            d2h_us.append(1e6 * d2h / a.frames)
            h2d_us.append(1e6 * h2d / a.frames)
        ce.read_recon_device(0, fmt, out=out)
        want = EM.recon_to("rgbp" if kind else fmt, ce.read_recon(0), CW, CH, W, H, color, pb)
        if kind and not name.endswith("_via_divide"):      # the float formats: the model's table of the 8-bit planes, as bit patterns
            want = FM.dequantise(want, kind)
            out = out.view(torch.int16 if FM.BYTES[kind] == 2 else torch.int32)
            want = want.view(np.int16 if FM.BYTES[kind] == 2 else np.int32)
        got = tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy().reshape(want.shape)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) if isinstance(out, tuple) else np.array_equal(got, want), name
        assert dev.numel() == CW * CH * 3 // 2
        ce.close()
        med = lambda v: round(statistics.median(v[1:]), 1)
        line["formats"][name] = {"kernel_us": med(kernel_us), "c_call_us": med(c_call_us), "call_us": med(call_us), "host_roundtrip_us": round(med(d2h_us) + med(h2d_us), 1),
                                 "read_recon_to_host_us": med(d2h_us), "upload_to_tensor_us": med(h2d_us),
                                 "samples_kernel_us": [round(x, 1) for x in kernel_us[1:]], "samples_c_call_us": [round(x, 1) for x in c_call_us[1:]], "samples_call_us": [round(x, 1) for x in call_us[1:]],
                                 "samples_host_roundtrip_us": [round(x + y, 1) for x, y in zip(d2h_us[1:], h2d_us[1:])]}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
