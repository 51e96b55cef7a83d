"""The SSIM of include/h264e_mi355x.h (H264E_clip_set_ssim_output / H264E_read_quality / H264E_ssim_planes, h264-lab_amd/csrc/enc_ssim.h),
restated in numpy: the 8x8-window, step-4 SSIM of x264 and of ffmpeg's `ssim` filter, per plane.

A = the input plane, B = the reconstruction, both w x h samples of the PICTURE.
  block (i, j), i < bw = w >> 2, j < bh = h >> 2: the 4x4 samples at (4i, 4j); sums of a, of b, of a^2 + b^2, of ab.  Samples right of
      4 bw and below 4 bh take no part.
  window (i, j), i < bw - 1, j < bh - 1: blocks (i..i+1, j..j+1); s1, s2, ss, s12 = the sums of theirs, over 64 samples.
  c1 = 416, c2 = 235963 (x264's 8-bit constants); vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2;
  v = ((2 s1 s2 + c1)(2 covar + c2)) / ((s1^2 + s2^2 + c1)(vars + c2)): four exact integers, converted to float64, two float64 products, one
      float64 division.
  a plane's value: the mean of v over its N = (bw - 1)(bh - 1) windows -- here with math.fsum, i.e. the correctly rounded sum.

Tolerance of a device value against this model (derived, not measured): a window value carries at most 4 roundings of 2^-53 and |v| <= 1; a
sum of N such values in any order adds at most N 2^-53: |got - model| <= (N + 8) 2^-52."""
import math

import numpy as np

C1, C2 = 416, 235963


def windows(w, h):
    """(windows per row, rows of windows) of a w x h plane"""
    return (w >> 2) - 1, (h >> 2) - 1


def factors(a, b):
    """the four integer factors of every window, each an int64 array [bh - 1, bw - 1]: (n1, n2, d1, d2) with v = n1 n2 / (d1 d2)"""
    a = np.asarray(a).astype(np.int64)
    b = np.asarray(b).astype(np.int64)
    assert a.ndim == 2 and a.shape == b.shape
    h, w = a.shape
    bw, bh = w >> 2, h >> 2
    assert bw >= 2 and bh >= 2, "a %d x %d plane has no 8 x 8 window" % (w, h)
    a, b = a[: 4 * bh, : 4 * bw], b[: 4 * bh, : 4 * bw]

    def blocks(x):
        return x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def wins(x):
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]

    s1, s2, ss, s12 = wins(blocks(a)), wins(blocks(b)), wins(blocks(a * a + b * b)), wins(blocks(a * b))
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    return 2 * s1 * s2 + C1, 2 * covar + C2, s1 * s1 + s2 * s2 + C1, vars_ + C2


def window_values(a, b):
    n1, n2, d1, d2 = factors(a, b)
    return (n1.astype(np.float64) * n2.astype(np.float64)) / (d1.astype(np.float64) * d2.astype(np.float64))


def plane(a, b):
    v = window_values(a, b)
    return math.fsum(v.reshape(-1).tolist()) / v.size


def tolerance(w, h):
    nx, ny = windows(w, h)
    return (nx * ny + 8) * 2.0 ** -52


def split_i420(buf, w, h, pitch=None, rows=None):
    """the three planes of a packed I420 buffer whose luma rows are `pitch` samples apart (a reconstruction: the coded size), cropped to w x h"""
    pitch, rows = pitch or w, rows or h
    buf = np.asarray(buf, np.uint8).reshape(-1)
    y = buf[: pitch * rows].reshape(rows, pitch)[:h, :w]
    u = buf[pitch * rows: pitch * rows * 5 // 4].reshape(rows // 2, pitch // 2)[: h // 2, : w // 2]
    v = buf[pitch * rows * 5 // 4: pitch * rows * 3 // 2].reshape(rows // 2, pitch // 2)[: h // 2, : w // 2]
    return y, u, v


def frame(inp, rec, w, h):
    """[Y, U, V] of one frame: inp = packed I420 of w x h, rec = packed I420 of the coded size"""
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    return [plane(a, b) for a, b in zip(split_i420(inp, w, h), split_i420(rec, w, h, cw, ch))]


def frame_ssd(inp, rec, w, h):
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    return [int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum()) for a, b in zip(split_i420(inp, w, h), split_i420(rec, w, h, cw, ch))]


def all_of(y, u, v):
    """ffmpeg's "All" for 4:2:0"""
    return (4 * y + u + v) / 6


def line(values):
    """encode_app --ssim's line from per-frame [Y, U, V] values: the means over the frames"""
    n = len(values)
    y, u, v = (sum(f[k] for f in values) / n for k in range(3))
    a = all_of(y, u, v)
    return "SSIM Y=%.6f U=%.6f V=%.6f All=%.6f (%.2f db)" % (y, u, v, a, -10 * math.log10(1 - a) if a < 1 else float("inf"))
