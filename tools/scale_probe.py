#!/usr/bin/env python3
"""What the scaled device input costs (enc_scale.h, h264e_scale_kernel): HIP-event time per frame of H264E_clip_upload_device_scaled
for 3840x2160 -> 1920x1080, 1920x1080 -> 1280x720, 1920x1080 -> 640x360 and a 1920x1080 crop of 3840x2160, next to its yardstick, the
plain ingest (enc_ingest.h) of a 3840x2160 I420 frame, which reads the same 12.4 MB of source.  Every call hands over `--batch` frames
(distinct source tensors, one kernel launch each, back to back on the encoder's copy stream); the events are recorded on that stream
around the launches alone (H264E_clip_input_time).  `--warmup` calls are thrown away, the median of `--reps` calls is reported, the
cases alternate within every repetition.  The slot of the first frame of every case is compared with tests/scale_model.py before
anything is timed.  Planar RGB (enc_scale_rgb.h, h264e_scale_rgb_kernel): 3840x2160 "rgbp" -> 1920x1080 from CHW tensors (24.9 MB of
source), and at 1920x1080 the plain "rgbp" ingest next to the interleaved "rgb" ingest of the same image and to the copy a caller
without the planar format pays first, torch's permute(1, 2, 0).contiguous() of the CHW frame (torch events around a batch of them).
--hbd times the decoder surfaces instead (enc_hbd.h): 3840x2160 -> 1920x1080 of "i420_16", "nv12_16", "i444" and "i444_16" frames (10-bit
words in int16 tensors) through h264e_scale_hbd_kernel, next to the two steps they replace -- torch's quantiser per plane,
((x.int() + r) >> s).clamp(max=255).to(uint8), plus the rounded 2x2 mean for 4:4:4 (torch events around a batch of them), followed by the
existing 8-bit "i420" / "nv12" window of the result.
--c422 times the 4:2:2 layouts (enc_422.h): 1920x1080 at the picture's size (h264e_ingest_422_kernel) and 3840x2160 -> 1920x1080
(h264e_scale_422_kernel) of "i422", "nv16", "yuyv", "uyvy" and their "_16" names, next to the two steps they replace -- torch de-interleaves, quantises and takes (a + b + 1) >> 1 over the row
pairs, then the existing "i420" ingest or window of the result -- and next to the existing "nv12" and "p010" kernels on the same picture.
Prints one JSON line.

    python tools/scale_probe.py [--batch 8] [--reps 25] [--warmup 3] [--hbd | --c422]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import color_model as CM  # noqa: E402
import pkg  # noqa: E402
import scale_model as M  # noqa: E402

# name, format, source size, picture size, crop
CASES = [
    ("ingest_3840x2160", "i420", (3840, 2160), (3840, 2160), None),
    ("scale_3840x2160_to_1920x1080", "i420", (3840, 2160), (1920, 1080), None),
    ("scale_1920x1080_to_1280x720", "i420", (1920, 1080), (1280, 720), None),
    ("scale_1920x1080_to_640x360", "i420", (1920, 1080), (640, 360), None),
    ("crop_1920x1080_of_3840x2160", "i420", (3840, 2160), (1920, 1080), (960, 540, 1920, 1080)),
    ("rgbp_scale_3840x2160_to_1920x1080", "rgbp", (3840, 2160), (1920, 1080), None),
    ("rgbp_crop_1920x1080_of_3840x2160", "rgbp", (3840, 2160), (1920, 1080), (960, 540, 1920, 1080)),
    ("rgbp_ingest_1920x1080", "rgbp", (1920, 1080), (1920, 1080), None),
    ("rgb3_ingest_1920x1080", "rgb", (1920, 1080), (1920, 1080), None),
    # the same launches with a matrix that is not the default (H264E_clip_set_color): the coefficients are launch arguments either way
    ("rgbp_scale_3840x2160_to_1920x1080_bt709_full", "rgbp", (3840, 2160), (1920, 1080), None),
    ("rgbp_ingest_1920x1080_bt709_full", "rgbp", (1920, 1080), (1920, 1080), None),
    ("rgb3_ingest_1920x1080_bt709_full", "rgb", (1920, 1080), (1920, 1080), None),
]


def make_sources(torch, rng, fmt, size, batch):
    """(host arrays, device tensors) of `batch` distinct random frames"""
    w, h = size
    if fmt == "i420":
        host = [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for _ in range(batch)]
    else:
        host = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for _ in range(batch)]
        if fmt == "rgb":
            host = [np.ascontiguousarray(x.transpose(1, 2, 0)) for x in host]
    return host, [torch.from_numpy(x).cuda() for x in host]


def model(fmt, host, size, dw, dh, crop, plain, color=(0, 0)):
    if fmt == "i420":
        return host.ravel() if plain else M.scale_frame(host, size[0], size[1], dw, dh, crop)
    if fmt == "rgb":
        return CM.to_i420(np.ascontiguousarray(host.transpose(2, 0, 1)), *color)
    return CM.to_i420(host, *color) if plain else CM.scale_to_i420(host, dw, dh, crop, *color)


HBD_DEPTH = 10


def hbd_main(a):
    """4K -> 1080p of the 16-bit and 4:4:4 layouts against torch's quantiser / 2x2 mean in front of the 8-bit window"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hbd_model as HM
    from ingest_probe import hbd_two_step
    P = pkg.load_pkg()
    assert P.load().h264e_hip_device_count() > 0, "no HIP device visible"
    (sw, sh), (dw, dh) = (3840, 2160), (1920, 1080)
    rng = np.random.default_rng(3)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    line = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "depth": HBD_DEPTH, "window": "3840x2160 -> 1920x1080", "us_per_frame": {}, "min_max_us": {}}
    for fmt in HM.FORMATS:
        cw, ch = (sw, sh) if HM.is_444(fmt) else (sw // 2, sh // 2)
        top = 1 << (HBD_DEPTH if HM.is_16(fmt) else 8)
        host = [[rng.integers(0, top, s).astype(np.int16 if HM.is_16(fmt) else np.uint8) for s in ((sh, sw), (ch, cw), (ch, cw))] for _ in range(a.batch)]
        parts = [[f[0], HM.interleave(f[1], f[2])] if fmt.startswith("nv12") else f for f in host]
        dev = [tuple(torch.from_numpy(p).cuda() for p in f) for f in parts]
        kw = dict(depth=HBD_DEPTH) if HM.is_16(fmt) else {}
        ce, ce8 = (P.ClipEncoder(dw, dh, a.batch, gop=30, qp=26) for _ in range(2))
        ce.upload_device(dev, fmt, src_size=(sw, sh), **kw)
        assert np.array_equal(ce.download(0, 1)[0], HM.slot(host[0], fmt, HBD_DEPTH, dw, dh)), fmt + ": the slot differs from the model"
        new_ms, torch_ms, old_ms = [], [], []
        for rep in range(a.warmup + a.reps):
            before = ce.input_time(True)
            ce.upload_device(dev, fmt, src_size=(sw, sh), **kw)
            after = ce.input_time(True)
            ev[0].record()
            made = [hbd_two_step(torch, f, fmt) for f in dev]
            ev[1].record()
            ev[1].synchronize()
            before8 = ce8.input_time(True)
            # 4:4:4: the mean has halved the chroma planes, the 8-bit source is a 4:2:0 frame of the luma's size
            ce8.upload_device([m[0] for m in made], made[0][1], src_size=(sw, sh))
            after8 = ce8.input_time(True)
            if rep >= a.warmup:
                new_ms.append((after[0] - before[0]) / a.batch)
                torch_ms.append(ev[0].elapsed_time(ev[1]) / a.batch)
                old_ms.append((after8[0] - before8[0]) / a.batch)
        if not HM.is_444(fmt):                      # 4:4:4's two steps average before they scale: another (twice rounded) picture
            assert np.array_equal(ce8.download(0, 1)[0], ce.download(0, 1)[0]), fmt + ": the two paths differ"
        ce.close()
        ce8.close()
        for name, ms in ((fmt, new_ms), (fmt + "_torch_part", torch_ms), (fmt + "_8bit_window_part", old_ms), (fmt + "_via_torch", [x + y for x, y in zip(torch_ms, old_ms)])):
            line["us_per_frame"][name] = round(1e3 * statistics.median(ms), 2)
            line["min_max_us"][name] = [round(1e3 * min(ms), 2), round(1e3 * max(ms), 2)]
        line[fmt + "_over_via_torch"] = round(line["us_per_frame"][fmt] / line["us_per_frame"][fmt + "_via_torch"], 3)
    print(json.dumps(line))


def c422_main(a):
    """1080p at the picture's size and 4K -> 1080p through the window: the 4:2:2 layouts against torch's de-interleave / quantiser / row mean
    in front of the existing "i420" path, and against the existing "nv12" and "p010" kernels on the same picture (the 4:2:0 frame whose chroma
    rows the 4:2:2 frame holds twice).  Kernel times are HIP events on the encoder's copy stream (H264E_clip_input_time), torch's part torch events"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import c422_model as C4
    import hbd_model as HM
    from ingest_probe import c422_two_step
    P = pkg.load_pkg()
    assert P.load().h264e_hip_device_count() > 0, "no HIP device visible"
    rng = np.random.default_rng(3)
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "depth": HBD_DEPTH, "cases": {}}
    for case, (sw, sh), (dw, dh) in (("ingest_1920x1080", (1920, 1080), (1920, 1080)), ("scale_3840x2160_to_1920x1080", (3840, 2160), (1920, 1080))):
        win = dict(src_size=(sw, sh)) if (sw, sh) != (dw, dh) else {}
        line = {"us_per_frame": {}, "min_max_us": {}, "source_mbytes": {}}
        base8 = [[rng.integers(0, 256, s).astype(np.uint8) for s in ((sh, sw), (sh // 2, sw // 2), (sh // 2, sw // 2))] for _ in range(a.batch)]
        want = M.scale_i420(*base8[0], dw, dh) if win else HM.pack(*base8[0])

        def timed(ce, dev, fmt, kw, ms, keep):
            before = ce.input_time(True)
            ce.upload_device(dev, fmt, **win, **kw)
            after = ce.input_time(True)
            if keep:
                ms.append((after[0] - before[0]) / a.batch)

        def report(name, ms):
            line["us_per_frame"][name] = round(1e3 * statistics.median(ms), 2)
            line["min_max_us"][name] = [round(1e3 * min(ms), 2), round(1e3 * max(ms), 2)]

        # the yardsticks: the existing kernels on the same picture
        for fmt in ("nv12", "p010"):
            planes = [[f[0], HM.interleave(f[1], f[2])] for f in base8]
            if fmt == "p010":
                planes = [[(p.astype(np.uint16) << 8).view(np.int16) for p in f] for f in planes]
            dev = [tuple(torch.from_numpy(p).cuda() for p in f) for f in planes]
            ce = P.ClipEncoder(dw, dh, a.batch, gop=30, qp=26)
            ms = []
            for rep in range(a.warmup + a.reps):
                timed(ce, dev, fmt, {}, ms, rep >= a.warmup)
            assert np.array_equal(ce.download(0, 1)[0], want), fmt + ": the slot differs from the model"
            ce.close()
            report(fmt, ms)
            line["source_mbytes"][fmt] = round(sum(p.nbytes for p in planes[0]) / 1e6, 2)
        for fmt in C4.FORMATS:
            host = [C4.from_420(*f) for f in base8]
            if C4.is_16(fmt):
                host = [[(p.astype(np.int16) << (HBD_DEPTH - 8)) for p in f] for f in host]
            arrays = [C4.layout(f, fmt) for f in host]
            dev = [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in f) for f in arrays]
            dev = [f[0] if len(f) == 1 else f for f in dev]
            kw = dict(depth=HBD_DEPTH) if C4.is_16(fmt) else {}
            ce, ce8 = (P.ClipEncoder(dw, dh, a.batch, gop=30, qp=26) for _ in range(2))
            ce.upload_device(dev, fmt, **win, **kw)
            assert np.array_equal(ce.download(0, 1)[0], C4.slot(host[0], fmt, HBD_DEPTH, dw, dh) if win else C4.slot(host[0], fmt, HBD_DEPTH)), fmt + ": the slot differs from the model"
            new_ms, torch_ms, old_ms = [], [], []
            for rep in range(a.warmup + a.reps):
                timed(ce, dev, fmt, kw, new_ms, rep >= a.warmup)
                ev[0].record()
                made = [c422_two_step(torch, f, fmt) for f in dev]
                ev[1].record()
                ev[1].synchronize()
                timed(ce8, [m[0] for m in made], "i420", {}, old_ms, rep >= a.warmup)
                if rep >= a.warmup:
                    torch_ms.append(ev[0].elapsed_time(ev[1]) / a.batch)
            # every chroma row comes twice here, so the two paths are the same arithmetic (tests/test_c422_model.py)
            assert np.array_equal(ce8.download(0, 1)[0], ce.download(0, 1)[0]), fmt + ": the two paths differ"
            ce.close()
            ce8.close()
            for name, ms in ((fmt, new_ms), (fmt + "_torch_part", torch_ms), (fmt + "_i420_part", old_ms), (fmt + "_via_torch", [x + y for x, y in zip(torch_ms, old_ms)])):
                report(name, ms)
            line["source_mbytes"][fmt] = round(sum(p.nbytes for p in arrays[0]) / 1e6, 2)
            line[fmt + "_over_via_torch"] = round(line["us_per_frame"][fmt] / line["us_per_frame"][fmt + "_via_torch"], 3)
        line["us_per_source_mbyte"] = {k: round(line["us_per_frame"][k] / v, 3) for k, v in line["source_mbytes"].items()}
        out["cases"][case] = line
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbd", action="store_true", help="time the 16-bit and 4:4:4 layouts (enc_hbd.h) against torch + the 8-bit window instead")
    ap.add_argument("--c422", action="store_true", help="time the 4:2:2 layouts (enc_422.h) against torch + the 8-bit window and the existing nv12 / p010 kernels instead")
    a = ap.parse_args()
    if a.hbd:
        return hbd_main(a)
    if a.c422:
        return c422_main(a)
    import torch
    P = pkg.load_pkg()
    assert P.load().h264e_hip_device_count() > 0, "no HIP device visible"
    rng = np.random.default_rng(3)
    sources, runs = {}, []
    for fmt, size in sorted({(c[1], c[2]) for c in CASES}):
        sources[fmt, size] = make_sources(torch, rng, fmt, size, a.batch)
    torch.cuda.synchronize()
    for name, fmt, size, (dw, dh), crop in CASES:
        host, dev = sources[fmt, size]
        color = (1, 1) if name.endswith("_bt709_full") else (0, 0)
        ce = P.ClipEncoder(dw, dh, a.batch, gop=30, qp=26, color=color)
        plain = "ingest" in name
        kw = {} if plain else dict(src_size=size, crop=crop)
        ce.upload_device(dev, fmt, **kw)
        assert np.array_equal(ce.download(0, 1)[0], model(fmt, host[0], size, dw, dh, crop, plain, color)), name + ": the slot differs from the model"
        ce.input_time(True)
        runs.append((name, fmt, ce, dev, kw, []))
    chw = sources["rgbp", (1920, 1080)][1]
    permute_ms, ev = [], (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    for rep in range(a.warmup + a.reps):
        for name, fmt, ce, dev, kw, ms in runs:
            before = ce.input_time(True)
            ce.upload_device(dev, fmt, **kw)
            after = ce.input_time(True)
            assert after[1] - before[1] == a.batch
            if rep >= a.warmup:
                ms.append((after[0] - before[0]) / a.batch)
        ev[0].record()
        hwc = [t.permute(1, 2, 0).contiguous() for t in chw]
        ev[1].record()
        ev[1].synchronize()
        del hwc
        if rep >= a.warmup:
            permute_ms.append(ev[0].elapsed_time(ev[1]) / a.batch)
    line = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "us_per_frame": {}, "min_max_us": {}}
    for name, _, ce, _, _, ms in runs + [("torch_permute_contiguous_1920x1080", None, None, None, None, permute_ms)]:
        if ce is not None:
            ce.close()
        line["us_per_frame"][name] = round(1e3 * statistics.median(ms), 2)
        line["min_max_us"][name] = [round(1e3 * min(ms), 2), round(1e3 * max(ms), 2)]
    us = line["us_per_frame"]
    line["scale_4k_to_1080p_over_ingest_4k"] = round(us["scale_3840x2160_to_1920x1080"] / us["ingest_3840x2160"], 3)
    line["rgbp_scale_4k_to_1080p_over_i420_scale"] = round(us["rgbp_scale_3840x2160_to_1920x1080"] / us["scale_3840x2160_to_1920x1080"], 3)
    line["rgbp_ingest_over_rgb3_ingest_1080p"] = round(us["rgbp_ingest_1920x1080"] / us["rgb3_ingest_1920x1080"], 3)
    line["permute_then_rgb3_ingest_over_rgbp_ingest_1080p"] = round((us["torch_permute_contiguous_1920x1080"] + us["rgb3_ingest_1920x1080"]) / us["rgbp_ingest_1920x1080"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
