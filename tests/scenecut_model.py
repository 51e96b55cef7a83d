"""numpy model of the clip encoder's key-frame schedule and of scene-cut detection (h264-lab_amd/csrc/enc_scenecut.h, h264e_host.c).

The schedule is the reference's rule (h264-lab.h:6725-6775, :6611-6614): what H264E_encode makes of frame f when it is handed
H264E_FRAME_TYPE_KEY on the forced frames and H264E_FRAME_TYPE_DEFAULT on all others.  The detector has no counterpart in the
reference; the integer definition below IS the definition:

    H_f[b] = number of luma samples of the raw input frame f with Y >> 2 == b,  b = 0..63
    D(f)   = (sum_b |H_f[b] - H_(f-1)[b]|) * 1024 // (2 * w * h),  D(0) = 0
    frame f > 0 that is not a key frame already (periodic, or forced by the caller) becomes one when D(f) > threshold

Frames are packed I420 (w*h luma bytes first)."""
import numpy as np

KEY, DEFAULT = 6, 0
SCENECUT_DEFAULT = 128


def schedule(n, gop, forced=()):
    """per frame (is_key, frame_num) for n frames.  frame_num and the periodic counter restart at every key frame; the counter wraps
    (h264-lab.h:6611) only on a DEFAULT call, so with gop = 1 the frame behind a forced key frame is a P frame; gop = 0: only forced
    frames and frame 0 are key frames."""
    forced = set(forced)
    out, fn = [], 0
    for f in range(n):
        key = f in forced or fn == 0
        if key:
            fn = 0
        out.append((key, fn))
        fn += 1
        if gop and fn >= gop and f not in forced:
            fn = 0
    return out


def kinds(n, gop, forced=()):
    return [k for k, _ in schedule(n, gop, forced)]


def histograms(clip, w, h):
    y = np.asarray(clip, np.uint8).reshape(len(clip), -1)[:, : w * h]
    return np.stack([np.bincount(f >> 2, minlength=64) for f in y]).astype(np.int64)


def distances(clip, w, h):
    H = histograms(clip, w, h)
    d = np.zeros(len(H), np.int64)
    d[1:] = np.abs(H[1:] - H[:-1]).sum(axis=1) * 1024 // (2 * w * h)
    return d.astype(np.int32)


def cuts(dist, gop, threshold, forced=()):
    """the merge rule: (is_cut per frame, the forced list with the detected cuts merged in).  A frame is tested against the schedule
    as it stands with the explicit list and the cuts BEFORE it."""
    forced = set(forced)
    is_cut, fn = np.zeros(len(dist), bool), 0
    for f in range(len(dist)):
        if threshold and f not in forced and fn and dist[f] > threshold:
            is_cut[f] = True
            forced.add(f)
        if f in forced or fn == 0:
            fn = 0
        fn += 1
        if gop and fn >= gop and f not in forced:
            fn = 0
    return is_cut, sorted(forced)


def detect(clip, w, h, gop, threshold=SCENECUT_DEFAULT, forced=()):
    """(dist, is_cut, merged forced list) of a clip"""
    d = distances(clip, w, h)
    c, merged = cuts(d, gop, threshold, forced)
    return d, c, merged
