"""Device-resident output (include/h264e_mi355x.h H264E_read_recon_device / H264E_clip_read_recon_device, h264-lab_amd/csrc/enc_egress.h,
DESIGN.md 4.5g), restated in numpy.  The reference has no conversion back to RGB, so this IS the definition:

  - the source is one reconstructed picture as read_recon returns it: packed I420 at the coded size W x H (multiples of 16); the
    destination is the picture's w x h samples (both even), the top-left corner of it;
  - "i420" and "nv12" copy the coded samples (NV12: U and V interleaved);
  - "rgb" and "rgbp": every chroma sample serves its 2x2 luma block (replication, no interpolation), and per pixel, with C = Y - yo,
    D = U - 128, E = V - 128,

        R = clamp8((ky C + rv E + 128) >> 8),  G = clamp8((ky C + gu D + gv E + 128) >> 8),  B = clamp8((ky C + bu D + 128) >> 8)

    with arithmetic shifts and a real clamp to 0..255; a fourth byte of an interleaved pixel is 255.  (ky, yo, rv, gu, gv, bu) is one of
    four rows: rv = 2(1 - Kr), bu = 2(1 - Kb), gu = -2 Kb (1 - Kb)/Kg, gv = -2 Kr (1 - Kr)/Kg, each times 255/224 for limited range;
    ky = 255/219 for limited range, 1 for full; times 256, rounded to nearest.

color is what set_color takes: None / (0, 0), a name of color_model.NAMES, or a (matrix, full_range) pair."""
import numpy as np

import color_model

# (matrix, full_range): (ky, yo, rv, gu, gv, bu)
ROWS = {
    (6, 0): (298, 16, 409, -100, -208, 516),
    (1, 0): (298, 16, 459, -55, -136, 541),
    (6, 1): (256, 0, 359, -88, -183, 454),
    (1, 1): (256, 0, 403, -48, -120, 475),
}
FORMATS = ("i420", "nv12", "rgb", "rgbp")


def row(color=None):
    if color is None:
        return ROWS[(6, 0)]
    matrix, full = color_model.NAMES[color] if isinstance(color, str) else color
    return ROWS[(matrix or 6, full)]


def derived_row(matrix, full):
    """the row from its recipe"""
    kr, kb = {6: (0.299, 0.114), 1: (0.2126, 0.0722)}[matrix]
    kg = 1 - kr - kb
    sy, sc = (1.0, 1.0) if full else (255 / 219, 255 / 224)
    vals = (sy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc)
    ky, rv, gu, gv, bu = (int(round(256 * x)) for x in vals)
    return (ky, 0 if full else 16, rv, gu, gv, bu)


def terms(y, u, v, coef):
    """int64 arrays: the three sums BEFORE the shift, and every product that goes through the 24-bit multiply"""
    ky, yo, rv, gu, gv, bu = coef
    c, d, e = y - yo, u - 128, v - 128
    products = (ky * c, rv * e, gu * d, gv * e, bu * d)
    return (ky * c + rv * e + 128, ky * c + gu * d + gv * e + 128, ky * c + bu * d + 128), products, (c, d, e)


def yuv_to_rgb(y, u, v, color=None):
    """int64 arrays of equal shape -> (R, G, B) int64 arrays in 0..255"""
    sums, _, _ = terms(np.asarray(y, np.int64), np.asarray(u, np.int64), np.asarray(v, np.int64), row(color))
    return tuple(np.clip(s >> 8, 0, 255) for s in sums)         # numpy's >> on signed integers is arithmetic


def planes(packed, W, H, w, h):
    """the (h, w) luma and the two (h/2, w/2) chroma planes of the picture inside a packed coded W x H I420 picture"""
    p = np.asarray(packed, np.uint8).reshape(-1)
    assert p.size == W * H * 3 // 2 and W % 16 == 0 and H % 16 == 0 and w <= W and h <= H and w % 2 == 0 and h % 2 == 0
    y = p[: W * H].reshape(H, W)[:h, :w]
    u = p[W * H: W * H * 5 // 4].reshape(H // 2, W // 2)[: h // 2, : w // 2]
    v = p[W * H * 5 // 4:].reshape(H // 2, W // 2)[: h // 2, : w // 2]
    return y, u, v


def recon_to(fmt, packed, W, H, w, h, color=None, pixel_bytes=3):
    """what the destination holds: "i420" a packed (h*3/2 * w) array, "nv12" (y of (h, w), uv of (h/2, w)), "rgb" (h, w, pixel_bytes),
    "rgbp" (3, h, w); all uint8"""
    y, u, v = planes(packed, W, H, w, h)
    if fmt == "i420":
        return np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
    if fmt == "nv12":
        return np.ascontiguousarray(y), np.stack([u, v], axis=2).reshape(h // 2, w)
    assert fmt in ("rgb", "rgbp"), fmt
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    r, g, b = yuv_to_rgb(y, up(u), up(v), color)
    if fmt == "rgbp":
        return np.stack([r, g, b]).astype(np.uint8)
    assert pixel_bytes in (3, 4)
    out = np.full((h, w, pixel_bytes), 255, np.uint8)
    out[:, :, 0], out[:, :, 1], out[:, :, 2] = r, g, b
    return out


def check_row(key, chunk=1 << 20):
    """every one of the 2^24 (Y, U, V) through the row, in chunks: both operands of every product fit 24 signed bits and every sum 32, so
    the device's 24-bit multiply and 32-bit adds compute exactly this; grey, black and white"""
    coef = ROWS[key]
    assert all(abs(k) < 1 << 23 for k in coef)
    for lo in range(0, 1 << 24, chunk):
        n = np.arange(lo, lo + chunk, dtype=np.int64)
        sums, products, operands = terms(n >> 16, (n >> 8) & 255, n & 255, coef)
        for o in operands:
            assert o.min() >= -(1 << 23) and o.max() < 1 << 23
        for x in products + sums:
            assert x.min() >= -(1 << 31) and x.max() < 1 << 31, (key, lo, int(x.min()), int(x.max()))
    k = np.arange(256, dtype=np.int64)
    r, g, b = yuv_to_rgb(k, np.full(256, 128), np.full(256, 128), key)
    assert np.array_equal(r, g) and np.array_equal(g, b), "grey is not neutral"
    assert (np.diff(r) >= 0).all()
    black, white = (0, 255) if key[1] else (16, 235)
    assert (int(r[black]), int(r[white])) == (0, 255), "black / white"
