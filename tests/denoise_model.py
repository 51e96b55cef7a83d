"""numpy restatement of the reference's temporal denoiser (h264-lab.h:1547-1621 h264e_denoise_run) from its contract:

per plane (Y at w x h, U and V at w/2 x h/2), cur = raw input, prev = state (the previous denoised picture, zeros at the start):
  border rows / columns: out = cur; a plane with w <= 2 or h <= 2: out = prev (left unchanged);
  interior: d = |cur - prev|, n = |sum over the 4 neighbours of (cur - prev)| >> 2, gd = 255 - T[d], gn = 255 - min(255, T[n] << 2),
            g = gn * gd, out = (prev * g + (65535 - g) * cur + 32768) >> 16.
All prev values are the old state.  out becomes the new state and the picture that is encoded."""
import numpy as np

# g_diff_to_gainQ8 (h264-lab.h:1122-1140), one entry per |difference| 0..255
GAIN = np.array([
    0, 16, 25, 32, 37, 41, 44, 48, 50, 53, 55, 57, 59, 60, 62, 64, 65, 66, 67, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79, 80,
    80, 81, 82, 82, 83, 83, 84, 85, 85, 86, 86, 87, 87, 88, 88, 89, 89, 90, 90, 91, 91, 92, 92, 92, 93, 93, 94, 94, 94, 95, 95, 96,
    96, 96, 97, 97, 97, 98, 98, 98, 99, 99, 99, 99, 100, 100, 100, 101, 101, 101, 102, 102, 102, 102, 103, 103, 103, 103, 104, 104, 104, 104, 105, 105,
    105, 105, 106, 106, 106, 106, 106, 107, 107, 107, 107, 108, 108, 108, 108, 108, 109, 109, 109, 109, 109, 110, 110, 110, 110, 110, 111, 111, 111, 111, 111, 112,
    112, 112, 112, 112, 112, 113, 113, 113, 113, 113, 113, 114, 114, 114, 114, 114, 114, 115, 115, 115, 115, 115, 115, 115, 116, 116, 116, 116, 116, 116, 117, 117,
    117, 117, 117, 117, 117, 118, 118, 118, 118, 118, 118, 118, 118, 119, 119, 119, 119, 119, 119, 119, 119, 120, 120, 120, 120, 120, 120, 120, 120, 121, 121, 121,
    121, 121, 121, 121, 121, 122, 122, 122, 122, 122, 122, 122, 122, 122, 123, 123, 123, 123, 123, 123, 123, 123, 123, 124, 124, 124, 124, 124, 124, 124, 124, 124,
    125, 125, 125, 125, 125, 125, 125, 125, 125, 125, 126, 126, 126, 126, 126, 126, 126, 126, 126, 126, 126, 127, 127, 127, 127, 127, 127, 127, 127, 127, 127, 128,
], dtype=np.int64)
assert GAIN.size == 256


def plane(cur, prev):
    """one plane: cur, prev 2-D uint8 arrays of the same shape -> out (uint8)"""
    h, w = cur.shape
    if w <= 2 or h <= 2:
        return prev.copy()
    c = cur.astype(np.int64)
    p = prev.astype(np.int64)
    dd = c - p
    out = cur.copy()
    ci, pi = c[1:-1, 1:-1], p[1:-1, 1:-1]
    d = np.abs(dd[1:-1, 1:-1])
    n = np.abs(dd[1:-1, :-2] + dd[1:-1, 2:] + dd[:-2, 1:-1] + dd[2:, 1:-1]) >> 2
    gd = 255 - GAIN[d]
    gn = 255 - np.minimum(255, GAIN[n] << 2)
    g = gn * gd
    v = (pi * g + (65535 - g) * ci + 32768) >> 16
    assert v.max(initial=0) <= 255
    out[1:-1, 1:-1] = v.astype(np.uint8)
    return out


def frame(cur, prev, w, h):
    """one packed I420 frame (w*h*3/2 bytes): raw input and previous state -> new state"""
    cur = np.asarray(cur, np.uint8).ravel()
    prev = np.asarray(prev, np.uint8).ravel()
    out = np.empty_like(cur)
    o = 0
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        n = pw * ph
        out[o:o + n] = plane(cur[o:o + n].reshape(ph, pw), prev[o:o + n].reshape(ph, pw)).ravel()
        o += n
    return out


def clip(frames, w, h, apply=None):
    """denoised pictures of consecutive frames from the zero state; apply[i] = False: frame i is not denoised (encode_speed >= 2),
    its raw picture is encoded and the state stays"""
    state = np.zeros(w * h * 3 // 2, np.uint8)
    out = []
    for i, f in enumerate(frames):
        if apply is not None and not apply[i]:
            out.append(np.asarray(f, np.uint8).ravel().copy())
            continue
        state = frame(f, state, w, h)
        out.append(state)
    return out


def device_planes(lib, frames, w, h, resident, chunk=None):
    """the same frames through the device layer's denoiser (include/h264e_hip.h h264e_hip_denoise_*) of a pool with `resident` input
    slots: frames are uploaded and denoised `chunk` at a time (default: as many as the ring holds) and read back with the test hook
    h264e_hip_read_denoised.  lib: path of the product library or of the emulation."""
    import ctypes as C
    L = C.CDLL(lib)
    L.h264e_hip_pool_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_pool_destroy.argtypes = [C.c_void_p]
    L.h264e_hip_pool_destroy.restype = None
    L.h264e_hip_upload_i420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.h264e_hip_denoise_reset.argtypes = [C.c_void_p]
    L.h264e_hip_denoise_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_read_denoised.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.h264e_hip_sync.argtypes = [C.c_void_p]
    L.h264e_hip_last_error.restype = C.c_char_p
    pool = C.c_void_p()
    assert L.h264e_hip_pool_create(C.byref(pool), 0, w, h, 1, resident) == 0, L.h264e_hip_last_error()
    fsz = w * h * 3 // 2
    chunk = chunk or resident
    out = []
    try:
        assert L.h264e_hip_denoise_reset(pool) == 0, L.h264e_hip_last_error()
        for f0 in range(0, len(frames), chunk):
            part = np.ascontiguousarray(np.asarray(frames[f0:f0 + chunk], np.uint8).reshape(-1, fsz))
            for i in range(part.shape[0]):
                assert L.h264e_hip_upload_i420(pool, (f0 + i) % resident, 1, part[i].ctypes.data) == 0, L.h264e_hip_last_error()
            assert L.h264e_hip_denoise_frames(pool, f0 % resident, part.shape[0], int(f0 == 0)) == 0, L.h264e_hip_last_error()
            for i in range(part.shape[0]):
                buf = np.empty(fsz, np.uint8)
                assert L.h264e_hip_read_denoised(pool, (f0 + i) % resident, buf.ctypes.data) == 0, L.h264e_hip_last_error()
                out.append(buf)
        assert L.h264e_hip_sync(pool) == 0, L.h264e_hip_last_error()
    finally:
        L.h264e_hip_pool_destroy(pool)
    return out
