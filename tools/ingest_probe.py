#!/usr/bin/env python3
"""What device-resident input costs and saves at 1080p (synth_v1, QP 26, GOP 30).  Per format (I420, NV12, RGB 3 and 4 bytes per pixel,
planar RGB from a CHW tensor with the default matrix and with BT.709 full range ("rgbp_bt709_full", H264E_clip_set_color), and "rgbp_via_permute": the same CHW tensor turned into HWC by torch's permute().contiguous() and handed
over as interleaved RGB, the two steps the planar format replaces; with --fmt also float planar RGB, "rgbp_f16" / "rgbp_bf16" / "rgbp_f32":
the same picture as a float CHW tensor in [0, 1] through the float ingest, and "rgbp_f16_via_quantise" / ...: that tensor quantised by
torch, (x * 255).round().clamp(0, 255).to(uint8), and handed over as "rgbp", the two steps the float formats replace):
with --fmt also the decoder surfaces, "i420_16" / "nv12_16" / "i444" / "i444_16": the same picture as 10-bit words in int16 tensors and /
or with chroma of the luma's size through the kernels of enc_hbd.h, and "i420_16_via_torch" / ...: those tensors quantised by torch,
((x.int() + r) >> s).clamp(max=255).to(uint8) per plane, plus the rounded 2x2 mean for 4:4:4, and handed over as "i420" / "nv12", the steps
the new formats replace);
with --fmt also 4:2:2, "i422" / "nv16" / "yuyv" / "uyvy" and their "_16" names: the same picture with every chroma row twice, as planes, U,V
pairs or one packed plane, of bytes or of 10-bit words in int16 tensors, through the kernels of enc_422.h, and "i422_via_torch" / ...: those
tensors de-interleaved, quantised and reduced by torch, (a + b + 1) >> 1 over the row pairs, and handed over as "i420", the steps the 4:2:2
formats replace):
the time per frame of H264E_clip_upload_device over `--frames` frames handed over in one call (one ingest kernel launch per frame, one
wait at the end: launch + kernel, host wall clock around a call that ends in a device synchronise), next to H264E_clip_upload of the
same frames from host memory -- the copy it replaces.  Then the per-frame API: H264E_encode (host planes) against H264E_encode_device
(torch tensor), alternating, `--reps` times.  Prints one JSON line.  The kernel's own time comes from a profiler run of this tool, e.g.
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/ingest_probe.py --frames 60 --reps 1

    python tools/ingest_probe.py [--frames 60] [--perframe 60] [--reps 5] [--fmt i420,rgbp,rgbp_f16,rgbp_f16_via_quantise,...]
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
import color_model as CM  # noqa: E402
import ingest_model as M  # noqa: E402
import pkg  # noqa: E402

W, H, QP, GOP = 1920, 1080, 26, 30
FORMATS = ("i420", "nv12", "rgb3", "rgb4", "rgbp", "rgbp_bt709_full", "rgbp_via_permute")
FLOAT_FORMATS = tuple("rgbp_" + k + v for k in ("f16", "bf16", "f32") for v in ("", "_via_quantise"))
HBD_FORMATS = tuple(k + v for k in ("i420_16", "nv12_16", "i444", "i444_16") for v in ("", "_via_torch"))
C422_FORMATS = tuple(k + s16 + v for k in ("i422", "nv16", "yuyv", "uyvy") for s16 in ("", "_16") for v in ("", "_via_torch"))
HBD_DEPTH = 10


def c422_sources(torch, c, base, w=W, h=H):
    """the frames of the packed I420 clip c (w x h) as the 4:2:2 format `base` takes them: every chroma row twice, 10-bit words
    (sample << 2) in int16 tensors for the "_16" names -- both quantise / average back to c"""
    import c422_model as C4
    out = []
    for f in c:
        y, u, v = f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)
        planes = C4.from_420(y, u, v)
        if base.endswith("_16"):
            planes = [(p.astype(np.int16) << (HBD_DEPTH - 8)) for p in planes]
        arrays = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in C4.layout(planes, base)]
        out.append(arrays[0] if len(arrays) == 1 else tuple(arrays))
    return out


def c422_two_step(torch, frame, base):
    """what a caller writes today in front of "i420": de-interleave, quantise, the rounded mean of the row pairs -- (frame, format name)"""
    parts = [frame] if not isinstance(frame, tuple) else list(frame)
    if base.endswith("_16"):
        r, s = 1 << (HBD_DEPTH - 9), HBD_DEPTH - 8
        parts = [((x.int() + r) >> s).clamp(max=255).to(torch.uint8) for x in parts]
    if base.startswith("i422"):
        y, u, v = parts
    elif base.startswith("nv16"):
        y, u, v = parts[0], parts[1][:, 0::2], parts[1][:, 1::2]
    else:
        iy, iu = (0, 1) if base.startswith("yuyv") else (1, 0)
        y, u, v = parts[0][:, iy::2].contiguous(), parts[0][:, iu::4], parts[0][:, iu + 2::4]
    return (y,) + tuple(((x[0::2].int() + x[1::2] + 1) >> 1).to(torch.uint8) for x in (u, v)), "i420"


def hbd_sources(torch, c, base):
    """the frames of the packed I420 clip c as `base` takes them: 10-bit words (sample << 2) in int16 tensors for the 16-bit layouts,
    chroma repeated 2 x 2 for 4:4:4 -- both quantise / average back to c"""
    out = []
    for f in c:
        y, u, v = f[:W * H].reshape(H, W), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2)
        if base.startswith("i444"):
            u, v = u.repeat(2, 0).repeat(2, 1), v.repeat(2, 0).repeat(2, 1)
        planes = [y, u, v]
        if base.endswith("_16"):
            planes = [(p.astype(np.int16) << (HBD_DEPTH - 8)) for p in planes]
        if base.startswith("nv12"):
            uv = np.empty((H // 2, W), planes[1].dtype)
            uv[:, 0::2], uv[:, 1::2] = planes[1], planes[2]
            planes = [planes[0], uv]
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes))
    return out


def hbd_two_step(torch, frame, base):
    """what a caller writes today in front of the 8-bit formats: (frame, format name)"""
    if base.endswith("_16"):
        r, s = 1 << (HBD_DEPTH - 9), HBD_DEPTH - 8
        frame = tuple(((x.int() + r) >> s).clamp(max=255).to(torch.uint8) for x in frame)
    if base.startswith("i444"):
        frame = (frame[0],) + tuple(((x[0::2, 0::2].int() + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2).to(torch.uint8) for x in frame[1:])
    return frame, "nv12" if base.startswith("nv12") else "i420"


def host_frames(P, n):
    ce = P.ClipEncoder(W, H, n)
    ce.generate_synth()
    buf = ce.download()
    ce.close()
    return buf


def sources(torch, c, fmt):
    """(frames for upload_device, binding format name, the packed I420 frames they stand for)"""
    if fmt == "i420":
        t = torch.from_numpy(c).cuda().view(len(c), H * 3 // 2, W)
        return [t[i] for i in range(len(c))], "i420", c
    if fmt == "nv12":
        pairs = [M.i420_to_nv12(f, W, H) for f in c]
        return [(torch.from_numpy(y).cuda(), torch.from_numpy(uv).cuda()) for y, uv in pairs], "nv12", c
    pb = 4 if fmt == "rgb4" else 3
    rgb = M.rgb_clip(W, H, 2, pb)
    model = np.stack([CM.rgb_to_i420(rgb[i % 2], *((1, 1) if fmt == "rgbp_bt709_full" else (0, 0))) for i in range(len(c))])
    if fmt in ("rgbp", "rgbp_bt709_full", "rgbp_via_permute") or fmt in FLOAT_FORMATS:
        ts = [torch.from_numpy(np.ascontiguousarray(rgb[i].transpose(2, 0, 1))).cuda() for i in range(2)]
        if fmt in FLOAT_FORMATS:            # v / 255 in the sample type: quantises back to v
            dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[fmt.split("_")[1]]
            ts = [(t.cpu().float() / 255).to(dtype).cuda() for t in ts]
            return [ts[i % 2] for i in range(len(c))], "rgbpf", model
        return [ts[i % 2] for i in range(len(c))], "rgbp", model
    ts = [torch.from_numpy(rgb[i]).cuda() for i in range(2)]
    return [ts[i % 2] for i in range(len(c))], "rgb", model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--perframe", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fmt", default=",".join(FORMATS), help="comma-separated, of: %s" % ", ".join(FORMATS + FLOAT_FORMATS + HBD_FORMATS + C422_FORMATS))
    a = ap.parse_args()
    fmts = [f for f in a.fmt.split(",") if f]
    for f in fmts:
        if f not in FORMATS + FLOAT_FORMATS + HBD_FORMATS + C422_FORMATS:
            ap.error("--fmt %s: one of %s" % (f, ", ".join(FORMATS + FLOAT_FORMATS + HBD_FORMATS + C422_FORMATS)))
    import torch
    P = pkg.load_pkg()
    c = host_frames(P, max(a.frames, a.perframe))
    line = {"clip": "1080p synth_v1, QP %d, GOP %d" % (QP, GOP), "frames": a.frames, "reps": a.reps, "formats": {}}
    for fmt in fmts:
        base = fmt[: -len("_via_torch")] if fmt.endswith("_via_torch") else fmt
        if fmt in C422_FORMATS:
            src, name, model = c422_sources(torch, c[: a.frames], base), base, c[: a.frames]
        elif fmt in HBD_FORMATS:
            src, name, model = hbd_sources(torch, c[: a.frames], base), base, c[: a.frames]
        else:
            src, name, model = sources(torch, c[: a.frames], fmt)
        torch.cuda.synchronize()
        ce = P.ClipEncoder(W, H, a.frames, gop=GOP, qp=QP, color="bt709-full" if fmt == "rgbp_bt709_full" else None)
        dev_ms, host_ms = [], []
        for _ in range(a.reps + 1):                     # the first repetition warms up (code object, page tables)
            t0 = time.perf_counter()
            if fmt == "rgbp_via_permute":
                ce.upload_device([t.permute(1, 2, 0).contiguous() for t in src], "rgb")
            elif fmt.endswith("_via_torch"):
                made = [(c422_two_step if fmt in C422_FORMATS else hbd_two_step)(torch, f, base) for f in src]
                ce.upload_device([m[0] for m in made], made[0][1])
            elif fmt in HBD_FORMATS + C422_FORMATS:
                ce.upload_device(src, name, **(dict(depth=HBD_DEPTH) if name.endswith("_16") else {}))
            elif fmt.endswith("_via_quantise"):
                ce.upload_device([(t * 255).round().clamp(0, 255).to(torch.uint8) for t in src], "rgbp")
            else:
                ce.upload_device(src, name)
            t1 = time.perf_counter()
            assert np.array_equal(ce.download(0, 1)[0], model[0])
            t2 = time.perf_counter()
            ce.upload(model)
            t3 = time.perf_counter()
            dev_ms.append(1e3 * (t1 - t0) / a.frames)
            host_ms.append(1e3 * (t3 - t2) / a.frames)
        ce.close()
        line["formats"][fmt] = {"device_ms_per_frame": round(statistics.median(dev_ms[1:]), 4), "host_upload_ms_per_frame": round(statistics.median(host_ms[1:]), 4),
                                "samples_device": [round(x, 4) for x in dev_ms[1:]], "samples_host": [round(x, 4) for x in host_ms[1:]]}
    t = torch.from_numpy(c[: a.perframe]).cuda().view(a.perframe, H * 3 // 2, W)
    fps = {"host": [], "device": []}
    outs = {}
    for _ in range(a.reps):
        for mode in ("host", "device"):
            e = P.Encoder(W, H, gop=GOP, qp=QP)
            parts = [e.encode(c[0]) if mode == "host" else e.encode_device(t[0], "i420")]
            t0 = time.perf_counter()
            for i in range(1, a.perframe):
                parts.append(e.encode(c[i]) if mode == "host" else e.encode_device(t[i], "i420"))
            dt = time.perf_counter() - t0
            e.close()
            fps[mode].append((a.perframe - 1) / dt)
            outs[mode] = b"".join(parts)
    assert outs["host"] == outs["device"]
    line["per_frame_api"] = {m: {"fps": round(statistics.median(v), 2), "samples": [round(x, 2) for x in v]} for m, v in fps.items()}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
