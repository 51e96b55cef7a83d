"""4:2:2 device input (include/h264e_mi355x.h H264E_DEV_CHROMA_422 / H264E_DEV_PACK_*, h264-lab_amd/csrc/enc_422.h), restated in numpy on
hbd_model.quantise and scale_model's filter.

A 4:2:2 frame has chroma of the luma's height and half its width: three planes ("i422"), a plane of U,V pairs ("nv16") or ONE plane of
groups Y0 U Y1 V ("yuyv") / U Y0 V Y1 ("uyvy"); the "_16" names hold 16-bit words with d significant bits, quantised first
(hbd_model.quantise).  At the picture's size luma is copied and

    U(i,j) = (a + b + 1) >> 1           a = U422(i, 2j), b = U422(i, 2j + 1), the 8-bit samples of one column in a pair of rows; V likewise.

Through a window the area filter of tests/scale_model.py runs on the 8-bit samples, per plane; a chroma plane's window is Sw/2 x Sh at
(cx/2, cy), reduced directly to Dw/2 x Dh/2.  Everything here returns the packed I420 picture the input slot holds."""
import numpy as np

import hbd_model as HM
import scale_model as SM

FORMATS_8 = ("i422", "nv16", "yuyv", "uyvy")
FORMATS_16 = tuple(f + "_16" for f in FORMATS_8)
FORMATS = FORMATS_8 + FORMATS_16
# the names with a fixed depth of 16 and the layout they are
ALIASES = {"p210": "nv16_16", "p216": "nv16_16", "y210": "yuyv_16", "y216": "yuyv_16", "yuy2": "yuyv"}


def is_16(fmt):
    return ALIASES.get(fmt, fmt) in FORMATS_16


def family(fmt):
    """"i422", "nv16", "yuyv" or "uyvy" """
    return ALIASES.get(fmt, fmt)[:4]


def mean_rows(p):
    """the rounded mean of the row pairs of an 8-bit plane of even height"""
    p = np.asarray(p, np.uint8).astype(np.int32)
    return ((p[0::2] + p[1::2] + 1) >> 1).astype(np.uint8)


def eight_bit(planes, fmt, depth):
    """the planes (y, u, v) of a frame as 8-bit planes of the same geometry"""
    return tuple(HM.quantise(p, depth) for p in planes) if is_16(fmt) else tuple(np.asarray(p, np.uint8) for p in planes)


def slot(planes, fmt, depth=16, dw=None, dh=None, crop=None):
    """the packed I420 picture of dw x dh that the input slot holds for the 4:2:2 frame (y, u, v) -- u and v of (h, w/2): at the picture's
    size (dw = None) or through the window crop = (x, y, w, h) of it (None: the whole frame)"""
    y, u, v = eight_bit(planes, fmt, depth)
    assert u.shape == v.shape == (y.shape[0], y.shape[1] // 2)
    if dw is None:
        return HM.pack(y, mean_rows(u), mean_rows(v))
    cx, cy, sw, sh = SM.window(y.shape[1], y.shape[0], crop)
    return HM.pack(SM.scale_plane(y, cx, cy, sw, sh, dw, dh), SM.scale_plane(u, cx // 2, cy, sw // 2, sh, dw // 2, dh // 2),
                   SM.scale_plane(v, cx // 2, cy, sw // 2, sh, dw // 2, dh // 2))


def picture(w, h, fmt, depth, t=0):
    """(y, u, v) of one w x h 4:2:2 test frame of format `fmt`: uint16 words with `depth` significant bits (uint8 for the 8-bit names) -- a
    moving gradient with noise in the low bits, the extremes of the range, and for depths below 16 a sprinkle of words with garbage in the
    unused bits"""
    d = depth if is_16(fmt) else 8
    rng = np.random.default_rng(2000 * d + 7 * w + h + 31 * t + len(family(fmt)))
    top = (1 << d) - 1

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

    return plane(w, h, 0), plane(w // 2, h, 1), plane(w // 2, h, 2)


# ---- the interleavers: the arrays a format stores, and back


def interleave_uv(u, v):
    """NV16's chroma plane of U,V pairs: (h, w) from two (h, w/2)"""
    return HM.interleave(u, v)


def interleave_packed(y, u, v, order):
    """one (h, 2w) plane of groups Y0 U Y1 V ("yuyv") or U Y0 V Y1 ("uyvy")"""
    out = np.empty((y.shape[0], 2 * y.shape[1]), y.dtype)
    iy, iu = (0, 1) if order == "yuyv" else (1, 0)
    out[:, iy::2], out[:, iu::4], out[:, iu + 2::4] = y, u, v
    return out


def layout(planes, fmt):
    """the arrays of the frame (y, u, v) as format `fmt` stores them: [y, u, v], [y, uv] or [packed]"""
    y, u, v = planes
    fam = family(fmt)
    return [y, u, v] if fam == "i422" else [y, interleave_uv(u, v)] if fam == "nv16" else [interleave_packed(y, u, v, fam)]


def planes_of(arrays, fmt):
    """(y, u, v) from the arrays of format `fmt`"""
    fam = family(fmt)
    if fam == "i422":
        return tuple(arrays)
    if fam == "nv16":
        return arrays[0], arrays[1][:, 0::2], arrays[1][:, 1::2]
    iy, iu = (0, 1) if fam == "yuyv" else (1, 0)
    return arrays[0][:, iy::2], arrays[0][:, iu::4], arrays[0][:, iu + 2::4]


def from_420(y, u, v):
    """the 4:2:2 frame that repeats every chroma row of a 4:2:0 frame"""
    return y, u.repeat(2, 0), v.repeat(2, 0)


# (source size, picture size, crop) of the window cases: 2:1; a fraction with a crop; the vertical limit (luma 8:1, chroma 16:1); 16:1 in width; a pure crop
WINDOWS = {"2to1": ((128, 96), (64, 48), None), "fraction_crop": ((100, 76), (64, 48), (2, 4, 96, 72)), "v8to1": ((64, 384), (64, 48), None),
           "h16to1": ((1024, 96), (64, 48), None), "pure_crop": ((128, 96), (64, 48), (64, 48, 64, 48))}
