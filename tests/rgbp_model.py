"""The planar RGB device input's definition (include/h264e_mi355x.h H264E_DEV_FORMAT_RGBP, h264-lab_amd/csrc/enc_ingest.h and
enc_scale_rgb.h), restated in numpy as the composition of the two definitions the project already has:

  - at the picture's size: ingest_model.rgb_to_i420 of the same pixels -- byte for byte what interleaved RGB gives for the same image;
  - with a window: each of R, G, B is reduced from the window Sw x Sh at (cx, cy) to Dw x Dh by scale_model.scale_plane (the exact area
    filter, rounded to 8 bits per channel, all three at luma geometry), and rgb_to_i420 is applied to that Dw x Dh RGB picture.  Chroma is
    therefore the matrix of the rounded 2x2 mean of already rounded samples: the double rounding is part of the definition.

Frames are planar: uint8 (3, H, W), channel planes R, G, B."""
import numpy as np

import ingest_model
import scale_model


def to_i420(chw):
    """(3, h, w) uint8 -> the packed I420 picture the encoder's input slot holds"""
    chw = np.asarray(chw)
    assert chw.ndim == 3 and chw.shape[0] == 3 and chw.dtype == np.uint8
    return ingest_model.rgb_to_i420(np.ascontiguousarray(chw.transpose(1, 2, 0)))


def scale_rgb(chw, dw, dh, crop=None):
    """(3, H, W) uint8 -> the (3, dh, dw) RGB picture: every channel through the area filter at luma geometry"""
    chw = np.asarray(chw)
    cx, cy, sw, sh = scale_model.window(chw.shape[2], chw.shape[1], crop)
    return np.stack([scale_model.scale_plane(chw[c], cx, cy, sw, sh, dw, dh) for c in range(3)])


def scale_to_i420(chw, dw, dh, crop=None):
    """a window of the (3, H, W) source -> the packed I420 picture of dw x dh"""
    return to_i420(scale_rgb(chw, dw, dh, crop))


def clip(w, h, n, salt=11):
    """n planar test frames (n, 3, h, w): ingest_model.rgb_clip's pixels, channel planes"""
    return np.ascontiguousarray(ingest_model.rgb_clip(w, h, n, 3, salt).transpose(0, 3, 1, 2))


def noisy_clip(w, h, n, seed=3):
    """... with per-pixel noise on top, so that neighbouring samples of every channel differ and area sums round both ways"""
    rng = np.random.default_rng(seed + w * 131 + h)
    c = clip(w, h, n).astype(np.int64) + rng.integers(-20, 21, (n, 3, h, w))
    return np.clip(c, 0, 255).astype(np.uint8)
