"""Decoder surfaces as device input (include/h264e_mi355x.h H264E_DEV_DEPTH / H264E_DEV_CHROMA_444, h264-lab_amd/csrc/enc_hbd.h), restated
in numpy.

16-bit samples: unsigned words with d significant bits (9 .. 16), LSB aligned; every word v is quantised as it is loaded,

    q = min(255, (v + (1 << (d - 9))) >> (d - 8))           round half up, one clamp; words above 2^d - 1 saturate to 255,

and from q on the plane is the 8-bit plane.  4:4:4 (U and V of the luma's size) at the picture's size: luma as it is,

    U(i,j) = (a + b + c + d + 2) >> 2                       over the 2x2 block of the 8-bit (quantised first) samples, V likewise.

Through a window the area filter of tests/scale_model.py runs on the quantised samples, per plane; a 4:4:4 chroma plane's window is the
luma's, Sw x Sh at (cx, cy), reduced directly to Dw/2 x Dh/2.  Everything here returns the packed I420 picture the input slot holds."""
import numpy as np

import scale_model as SM

DEPTHS = range(9, 17)
FORMATS_16 = ("i420_16", "nv12_16", "i444_16")
FORMATS = FORMATS_16 + ("i444",)


def quantise(v, d):
    """the 8-bit samples of 16-bit words (any integer array; int16 tensors hold the same bits) at depth d"""
    v = np.asarray(v).astype(np.int64) & 0xffff
    return np.minimum(255, (v + (1 << (d - 9))) >> (d - 8)).astype(np.uint8)


def mean2x2(p):
    """the rounded mean of the 2x2 blocks of an 8-bit plane of even size"""
    p = np.asarray(p, np.uint8).astype(np.int32)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pack(y, u, v):
    return np.concatenate([np.asarray(y, np.uint8).ravel(), np.asarray(u, np.uint8).ravel(), np.asarray(v, np.uint8).ravel()])


def is_444(fmt):
    return fmt.startswith("i444")


def is_16(fmt):
    return fmt in FORMATS_16 or fmt in ("p010", "p016")


def eight_bit(planes, fmt, depth):
    """the planes (y, u, v) of a frame of format `fmt` as 8-bit planes of the same geometry"""
    return tuple(quantise(p, depth) for p in planes) if is_16(fmt) else tuple(np.asarray(p, np.uint8) for p in planes)


def slot(planes, fmt, depth=16, dw=None, dh=None, crop=None):
    """the packed I420 picture of dw x dh that the input slot holds for the frame (y, u, v): at the picture's size (dw = None) or through
    the window crop = (x, y, w, h) of it (None: the whole frame)"""
    y, u, v = eight_bit(planes, fmt, depth)
    if dw is None:
        return pack(y, mean2x2(u), mean2x2(v)) if is_444(fmt) else pack(y, u, v)
    if not is_444(fmt):
        return SM.scale_i420(y, u, v, dw, dh, crop)
    cx, cy, sw, sh = SM.window(y.shape[1], y.shape[0], crop)
    return pack(SM.scale_plane(y, cx, cy, sw, sh, dw, dh), SM.scale_plane(u, cx, cy, sw, sh, dw // 2, dh // 2), SM.scale_plane(v, cx, cy, sw, sh, dw // 2, dh // 2))


def picture(w, h, fmt, depth, t=0):
    """(y, u, v) of one w x h test frame of format `fmt`: uint16 words with `depth` significant bits (uint8 for "i444") -- a moving gradient
    with noise in the low bits, the extremes of the range, and for depths below 16 a sprinkle of words with garbage in the unused bits"""
    d = depth if is_16(fmt) else 8
    rng = np.random.default_rng(1000 * d + 7 * w + h + 31 * t + len(fmt))
    top = (1 << d) - 1
    cw, ch = (w, h) if is_444(fmt) else (w // 2, h // 2)

    def plane(pw, ph, k):
        yy, xx = np.mgrid[0:ph, 0:pw]
        p = ((xx * (5 + k) + yy * (3 + 2 * k) + 11 * t + 17 * k) * (top + 1) // 97 + rng.integers(0, 1 << (d - 7), (ph, pw))) & top
        flat = p.reshape(-1)
        flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = top
        flat[rng.integers(0, flat.size, max(1, flat.size // 16))] = 0
        if d < 16 and is_16(fmt):
            idx = rng.integers(0, flat.size, max(1, flat.size // 8))
            flat[idx] |= rng.integers(1, 1 << (16 - d), idx.size) << d
        return p.astype(np.uint16 if is_16(fmt) else np.uint8)

    return plane(w, h, 0), plane(cw, ch, 1), plane(cw, ch, 2)


def all_patterns_picture():
    """a 512 x 256 4:2:0 frame of 16-bit words: luma holds every word twice, U the words 0 .. 32767, V the rest"""
    rng = np.random.default_rng(5)
    y = rng.permutation(np.repeat(np.arange(65536, dtype=np.uint32), 2)).astype(np.uint16).reshape(256, 512)
    u = rng.permutation(np.arange(32768, dtype=np.uint32)).astype(np.uint16).reshape(128, 256)
    v = rng.permutation(np.arange(32768, 65536, dtype=np.uint32)).astype(np.uint16).reshape(128, 256)
    return y, u, v


def interleave(u, v):
    """NV12's chroma plane of U,V pairs"""
    uv = np.empty((u.shape[0], 2 * u.shape[1]), u.dtype)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return uv


# (source size, picture size, crop) of the window cases; the 16:1 case is for the 4:2:0 layouts, the 8:1 case for 4:4:4 (its chroma goes 16:1)
WINDOWS = {"2to1": ((128, 96), (64, 48), None), "fraction": ((100, 76), (64, 48), None), "16to1": ((1024, 768), (64, 48), None),
           "8to1": ((512, 384), (64, 48), None), "crop_6_2": ((140, 100), (64, 48), (6, 2, 128, 96)), "pure_crop": ((128, 96), (64, 48), (64, 48, 64, 48))}


def windows_of(fmt):
    return [k for k in WINDOWS if k != ("16to1" if is_444(fmt) else "8to1")]
