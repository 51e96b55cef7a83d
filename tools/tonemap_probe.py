#!/usr/bin/env python3
"""What HDR10 device input costs (enc_tonemap.h, h264e_tonemap_kernel): HIP-event time per frame of H264E_clip_upload_device[_scaled] with
tone mapping on for a 3840x2160 P010 frame at size and through the window 3840x2160 -> 1920x1080 (the tone-map launch, then the existing
scale kernel from the encoder's surface), next to
  - the existing P010 paths of the same frames with tone mapping off (enc_hbd.h: what the new launches are added to or replace), and
  - the same definition written as torch expressions on the GPU in front of "rgbp" (torch events around a batch of them) plus the
    existing "rgbp" ingest or window of the result: what a caller without the setting writes today.
Every call hands over `--batch` frames (distinct source tensors, back to back on the encoder's copy stream); the events are recorded on
that stream around the launches alone (H264E_clip_input_time).  `--warmup` calls are thrown away, the median of `--reps` calls is
reported, the cases alternate within every repetition.  Before anything is timed the slot of the first frame is compared with
tests/tonemap_model.py (the top quarter of the picture, to keep numpy short) and with the torch chain's.  Prints one JSON line; --out also writes it.

    python tools/tonemap_probe.py [--batch 8] [--reps 25] [--warmup 3] [--out profiles/tonemap_probe.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pkg  # noqa: E402
import tonemap_model as TM  # noqa: E402

SRC, HALF = (3840, 2160), (1920, 1080)
COLOR = "bt709"


def make_sources(torch, rng, batch):
    """`batch` distinct P010 frames: (host (y, u, v) of the first, device (y, uv) int16 tensors of all)"""
    w, h = SRC
    first, dev = None, []
    for _ in range(batch):
        y, u, v = (rng.integers(0, 65536, s, dtype=np.uint16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
        if first is None:
            first = (y, u, v)
        dev.append(tuple(torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).cuda() for p in (y, TM.interleave(u, v))))
    return first, dev


class TorchChain:
    """steps 1 to 5 of the definition as torch expressions: every float32 operation a kernel of its own, so rounded on its own"""

    def __init__(self, torch, tables):
        ycc, eotf, scale, thresh = tables
        self.t = torch
        self.ycc = [int(c) for c in ycc]
        self.eotf, self.scale = torch.from_numpy(eotf).cuda(), torch.from_numpy(scale).cuda()
        self.thresh = torch.from_numpy(np.ascontiguousarray(thresh[1:])).cuda()
        self.g = TM.GAMUT.astype(np.float32).tolist()

    def __call__(self, frame):
        t = self.t
        ky, crv, cgu, cgv, cbu = self.ycc[:5]
        y, uv = frame
        Y = (((y.int() & 0xffff) + 32) >> 6).clamp(max=1023)
        c = (((uv.int() & 0xffff) + 32) >> 6).clamp(max=1023) - 512
        u, v = (p.repeat_interleave(2, 0).repeat_interleave(2, 1) for p in (c[:, 0::2], c[:, 1::2]))
        luma = ky * (Y - 64) + 8192
        R, G, B = (((luma + x) >> 14).clamp(0, 1023) for x in (crv * v, -cgu * u - cgv * v, cbu * u))
        sc = self.scale[t.maximum(t.maximum(R, G), B)]
        lin = [self.eotf[x] * sc for x in (R, G, B)]
        out = [t.bucketize((g[0] * lin[0] + g[1] * lin[1]) + g[2] * lin[2], self.thresh, right=True).to(t.uint8) for g in self.g]
        return t.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    P = pkg.load_pkg()
    rng = np.random.default_rng(3)
    first, dev = make_sources(torch, rng, a.batch)
    tables = P.tonemap_tables("pq")
    chain = TorchChain(torch, tables)
    torch.cuda.synchronize()
    enc = {name: P.ClipEncoder(size[0], size[1], a.batch, gop=30, qp=26, color=COLOR, tonemap=tm) for name, size, tm in
           (("tonemap_at_size", SRC, "pq"), ("tonemap_window", HALF, "pq"), ("p010_at_size", SRC, None), ("p010_window", HALF, None),
            ("rgbp_at_size", SRC, None), ("rgbp_window", HALF, None))}
    win = dict(src_size=SRC)

    def kernel_case(name):
        ce = enc[name]
        ce.input_time(True)
        before = ce.input_time(True)[0]
        ce.upload_device(dev, "p010", **(win if name.endswith("window") else {}))
        return (ce.input_time(True)[0] - before) / a.batch

    def torch_case(name):
        """(torch's chain, the rgbp launches behind it) per frame"""
        ce = enc[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rgb = [chain(f) for f in dev]
        e1.record()
        torch.cuda.synchronize()
        before = ce.input_time(True)[0]
        ce.upload_device(rgb, "rgbp", **(win if name.endswith("window") else {}))
        return e0.elapsed_time(e1) / a.batch, (ce.input_time(True)[0] - before) / a.batch

    # correctness first: the first frame's slot against the numpy model (the top quarter of the picture) and the torch chain's
    # (through the window the two paths are not the same function: the setting scales the tone-mapped 4:2:0 picture, "rgbp" scales R'G'B')
    checks = {}
    kernel_case("tonemap_at_size")
    torch_case("rgbp_at_size")
    checks["tonemap_at_size_equals_torch_chain"] = bool(np.array_equal(enc["tonemap_at_size"].download(0, 1)[0], enc["rgbp_at_size"].download(0, 1)[0]))
    q = SRC[1] // 4
    top = (first[0][:q], first[1][:q // 2], first[2][:q // 2])
    want = TM.slot(top, 16, tables, (1, 0))
    got = enc["tonemap_at_size"].download(0, 1)[0]
    w, h = SRC
    assert np.array_equal(got[:w * q], want[:w * q]), "the slot's luma differs from tests/tonemap_model.py"
    assert np.array_equal(got[w * h:w * h + w // 2 * (q // 2)], want[w * q:w * q + w // 2 * (q // 2)]), "the slot's U differs from tests/tonemap_model.py"
    checks["tonemap_at_size_equals_numpy_model_top_quarter"] = True

    names = ["tonemap_at_size", "tonemap_window", "p010_at_size", "p010_window"]
    samples = {n: [] for n in names}
    samples.update({"torch_chain": [], "rgbp_at_size_after_chain": [], "rgbp_window_after_chain": []})
    for rep in range(a.warmup + a.reps):
        row = {n: kernel_case(n) for n in names}
        c0, r0 = torch_case("rgbp_at_size")
        c1, r1 = torch_case("rgbp_window")
        row.update({"torch_chain": (c0 + c1) / 2, "rgbp_at_size_after_chain": r0, "rgbp_window_after_chain": r1})
        if rep >= a.warmup:
            for k, v in row.items():
                samples[k].append(v)
    for ce in enc.values():
        ce.close()
    med = {k: statistics.median(v) for k, v in samples.items()}
    nbytes = SRC[0] * SRC[1] * 3                    # P010: 3 bytes per pixel read
    line = {"source": "3840x2160 P010 (random words), hable, 1000 / 203 nits, color %s" % COLOR, "batch": a.batch, "reps": a.reps, "warmup": a.warmup,
            "what": "HIP-event ms per frame on the copy stream (torch_chain: torch events)", "checks": checks,
            "median_ms": {k: round(v, 4) for k, v in med.items()},
            "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in samples.items()},
            "torch_path_ms": {"at_size": round(med["torch_chain"] + med["rgbp_at_size_after_chain"], 4), "window": round(med["torch_chain"] + med["rgbp_window_after_chain"], 4)},
            "tonemap_at_size_GBps_read_and_written": round((nbytes + SRC[0] * SRC[1] * 1.5) / med["tonemap_at_size"] / 1e6, 1)}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
