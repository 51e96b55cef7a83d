"""The scaled device input's definition (include/h264e_mi355x.h H264E_dev_window_t, h264-lab_amd/csrc/enc_scale.h), restated in numpy.

A window of Sw x Sh samples at (cx, cy) of a plane is reduced to Dw x Dh (Dw <= Sw, Dh <= Sh) by an exact area filter:

    wx(i,k)  = max(0, min((i+1) Sw, (k+1) Dw) - max(i Sw, k Dw))           (sum over k = Sw; wy(j,l) likewise with Sh, Dh)
    out(i,j) = floor((sum_l sum_k wy(j,l) wx(i,k) src(cx+k, cy+l) + ((Sw Sh) >> 1)) / (Sw Sh))

scale_plane_direct() is that text, sample by sample in Python integers.  scale_plane() computes the same sums another way -- as
differences of the running integral of the piecewise-constant source, F(x) = Dw * (sum of the samples before k) + (x - k Dw) * src[k]
with k = x // Dw, taken at the column borders x = i Sw -- which is exact in int64 and fast enough for 4096 x 4096 planes; the model's own
tests hold the two together.  Chroma planes: every value halved, the half-sample siting shift ignored."""
import numpy as np


def scale_plane_direct(src, cx, cy, sw, sh, dw, dh):
    out = np.zeros((dh, dw), np.uint8)
    for j in range(dh):
        for i in range(dw):
            acc = 0
            for l in range(sh):
                wy = max(0, min((j + 1) * sh, (l + 1) * dh) - max(j * sh, l * dh))
                if not wy:
                    continue
                for k in range(sw):
                    wx = max(0, min((i + 1) * sw, (k + 1) * dw) - max(i * sw, k * dw))
                    acc += wy * wx * int(src[cy + l, cx + k])
            out[j, i] = (acc + ((sw * sh) >> 1)) // (sw * sh)
    return out


def _integrate(a, s, d):
    """sums over axis 1 of `a` (n x s, int64) with the weights of s -> d: n x d"""
    n = a.shape[0]
    before = np.zeros((n, s + 1), np.int64)
    np.cumsum(a, axis=1, out=before[:, 1:])
    padded = np.concatenate([a, np.zeros((n, 1), np.int64)], axis=1)
    x = np.arange(d + 1, dtype=np.int64) * s
    k = x // d
    f = d * before[:, k] + (x - k * d) * padded[:, k]
    return f[:, 1:] - f[:, :-1]


def scale_plane(src, cx, cy, sw, sh, dw, dh):
    """the window (cx, cy, sw, sh) of the 2-D uint8 array `src`, reduced to dh x dw"""
    assert 0 < dw <= sw and 0 < dh <= sh and cx >= 0 and cy >= 0 and cy + sh <= src.shape[0] and cx + sw <= src.shape[1]
    win = np.asarray(src)[cy:cy + sh, cx:cx + sw].astype(np.int64)
    h = _integrate(win, sw, dw)                     # sh x dw
    v = _integrate(np.ascontiguousarray(h.T), sh, dh).T   # dh x dw
    out = (v + ((sw * sh) >> 1)) // (sw * sh)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def window(src_w, src_h, crop):
    return (0, 0, src_w, src_h) if crop is None else tuple(crop)


def scale_i420(y, u, v, dw, dh, crop=None):
    """source planes (2-D uint8: y of (H, W), u and v of (H/2, W/2)) -> the packed I420 picture of dw x dh the encoder's input slot holds"""
    cx, cy, sw, sh = window(y.shape[1], y.shape[0], crop)
    return np.concatenate([scale_plane(y, cx, cy, sw, sh, dw, dh).ravel(),
                           scale_plane(u, cx // 2, cy // 2, sw // 2, sh // 2, dw // 2, dh // 2).ravel(),
                           scale_plane(v, cx // 2, cy // 2, sw // 2, sh // 2, dw // 2, dh // 2).ravel()])


def scale_frame(frame, src_w, src_h, dw, dh, crop=None):
    """the same for a packed I420 source frame"""
    y, u, v = split(frame, src_w, src_h)
    return scale_i420(y, u, v, dw, dh, crop)


def split(frame, w, h):
    f = np.asarray(frame, np.uint8).ravel()
    return f[:w * h].reshape(h, w), f[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:w * h * 3 // 2].reshape(h // 2, w // 2)


def nv12_planes(frame, w, h):
    """(y, interleaved uv of (h/2, w)) of a packed I420 frame"""
    y, u, v = split(frame, w, h)
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = u, v
    return y, uv


def source_clip(w, h, n, seed=7):
    """n packed I420 frames of w x h: a moving gradient with texture and noise, so that neighbouring samples differ and frames move"""
    rng = np.random.default_rng(seed + w * 131 + h)
    out = np.empty((n, w * h * 3 // 2), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(n):
        luma = (xx * 3 + yy * 2 + 9 * t + 40 * np.sin((xx + 5 * t) / 7.0) * np.cos(yy / 5.0)) % 256
        luma = np.clip(luma + rng.integers(-12, 13, (h, w)), 0, 255)
        cu = np.clip(128 + 60 * np.sin((xx[::2, ::2] + 3 * t) / 11.0) + rng.integers(-6, 7, (h // 2, w // 2)), 0, 255)
        cv = np.clip(128 + 60 * np.cos((yy[::2, ::2] - 2 * t) / 9.0) + rng.integers(-6, 7, (h // 2, w // 2)), 0, 255)
        out[t] = np.concatenate([luma.astype(np.uint8).ravel(), cu.astype(np.uint8).ravel(), cv.astype(np.uint8).ravel()])
    return out
