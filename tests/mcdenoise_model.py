"""numpy restatement of the motion-compensated temporal denoiser (include/h264e_mi355x.h H264E_clip_set_denoise_motion, enc_mcdenoise.h).
The reference has no such filter; this integer definition is the definition the product is tested against.  Per frame f:

    cur = the RAW input (Y w x h, U and V w/2 x h/2); D_{f-1} = the previous OUTPUT of this filter, zeros in front of frame 0;
    (dx, dy) = frame f's motion field cell of block (bx, by) from the searched cost pass (lookahead_motion_model), nbx = (w/2) >> 3,
    nby = (h/2) >> 3; frame 0 has a zero field.
    luma vector of the 16x16 block at (16bx, 16by): mode 1 (2dx, 2dy); mode 2 the first candidate with the smallest sad among (0, 0) and
    then (2dx + rx, 2dy + ry), (rx, ry) in {-1, 0, 1}^2 in the order (|rx| + |ry|, ry, rx), where a candidate counts when its displaced
    block lies wholly inside the plane and sad = sum over the block of |Y_f(x, y) - D_{f-1}(x + vx, y + vy)|;
    chroma vector of the 8x8 block (bx, by): (dx, dy); samples that no block covers: (0, 0).
    filter, per plane, sample s with the vector v of its own block: first / last row and column out = cur, otherwise
    out = denoise_px(T, cur(s), D_{f-1}(clamp(s + v)), sum over the four neighbours n of cur(n) - D_{f-1}(clamp(n + v)))
    (denoise_model's formula), both coordinates clamped to the plane."""
import numpy as np

import denoise_model as DM
import lookahead_motion_model as ML

REFINE = sorted(((rx, ry) for ry in (-1, 0, 1) for rx in (-1, 0, 1)), key=lambda r: (abs(r[0]) + abs(r[1]), r[1], r[0]))


def candidates(dx, dy):
    """the ten luma candidates of a block whose field cell is (dx, dy), in order"""
    return [(0, 0)] + [(2 * dx + rx, 2 * dy + ry) for rx, ry in REFINE]


def block_sad(cur, prev, x0, y0, size, v):
    """sad of the size x size block at (x0, y0) of cur against prev displaced by v, or None when the displaced block leaves the plane"""
    h, w = cur.shape
    x1, y1 = x0 + v[0], y0 + v[1]
    if x1 < 0 or y1 < 0 or x1 + size > w or y1 + size > h:
        return None
    return int(np.abs(cur[y0:y0 + size, x0:x0 + size].astype(np.int64) - prev[y1:y1 + size, x1:x1 + size].astype(np.int64)).sum())


def luma_vectors(cur, prev, mv, mode):
    """(v int [nby, nbx, 2], sad int [nby, nbx]) of the luma planes cur / prev [h, w] and the field mv [nby, nbx, 2]"""
    h, w = cur.shape
    nby, nbx = mv.shape[:2]
    d = np.asarray(mv, np.int64)
    c, p = cur[: 16 * nby, : 16 * nbx].astype(np.int64), prev.astype(np.int64)
    yy, xx = np.mgrid[0:16 * nby, 0:16 * nbx]
    y0, x0 = 16 * np.arange(nby)[:, None], 16 * np.arange(nbx)[None, :]
    zero = np.zeros((nby, nbx), np.int64)
    cands = [(zero, zero)] + [(2 * d[:, :, 0] + rx, 2 * d[:, :, 1] + ry) for rx, ry in REFINE] if mode == 2 else [(2 * d[:, :, 0], 2 * d[:, :, 1])]
    v = np.zeros((nby, nbx, 2), np.int64)
    best = np.full((nby, nbx), 1 << 40, np.int64)
    for cx, cy in cands:
        inside = (x0 + cx >= 0) & (x0 + cx + 16 <= w) & (y0 + cy >= 0) & (y0 + cy + 16 <= h)
        px = np.clip(xx + np.repeat(np.repeat(cx, 16, axis=0), 16, axis=1), 0, w - 1)       # (clipped only where the candidate does not count)
        py = np.clip(yy + np.repeat(np.repeat(cy, 16, axis=0), 16, axis=1), 0, h - 1)
        sad = np.abs(c - p[py, px]).reshape(nby, 16, nbx, 16).sum(axis=(1, 3))
        take = inside & (sad < best)            # strictly smaller: the first of equals stays
        best[take] = sad[take]
        v[take] = np.stack([cx, cy], axis=-1)[take]
    return v, best


def plane(cur, prev, vec, size):
    """one plane: cur, prev [h, w] uint8, vec [nby, nbx, 2] the vector of each size x size block -> out (uint8)"""
    h, w = cur.shape
    nby, nbx = vec.shape[:2]
    vx, vy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    vx[: size * nby, : size * nbx] = np.repeat(np.repeat(vec[:, :, 0], size, axis=0), size, axis=1)
    vy[: size * nby, : size * nbx] = np.repeat(np.repeat(vec[:, :, 1], size, axis=0), size, axis=1)
    yy, xx = np.mgrid[0:h, 0:w]
    c, p = cur.astype(np.int64), prev.astype(np.int64)

    def diff(ox, oy):
        """cur(s + o) - prev(clamp(s + o + v(s))) for every sample s that has the neighbour s + o"""
        ys, xs = np.clip(yy + oy, 0, h - 1), np.clip(xx + ox, 0, w - 1)
        return c[ys, xs] - p[np.clip(yy + oy + vy, 0, h - 1), np.clip(xx + ox + vx, 0, w - 1)]

    pc = p[np.clip(yy + vy, 0, h - 1), np.clip(xx + vx, 0, w - 1)]
    d = np.abs(c - pc)
    n = np.abs(diff(-1, 0) + diff(1, 0) + diff(0, -1) + diff(0, 1)) >> 2
    gd = 255 - DM.GAIN[d]
    gn = 255 - np.minimum(255, DM.GAIN[n] << 2)
    g = gn * gd
    val = (pc * g + (65535 - g) * c + 32768) >> 16
    out = cur.copy()
    out[1:-1, 1:-1] = val[1:-1, 1:-1].astype(np.uint8)
    return out


def frame(cur, prev, w, h, mv, mode):
    """one packed I420 frame: raw input, previous state and the frame's field -> (new state, (v int8 [nby, nbx, 2], sad uint16))"""
    cur, prev = np.asarray(cur, np.uint8).ravel(), np.asarray(prev, np.uint8).ravel()
    cw, ch = w // 2, h // 2
    out = np.empty_like(cur)
    y, py = cur[: w * h].reshape(h, w), prev[: w * h].reshape(h, w)
    v, sad = luma_vectors(y, py, mv, mode)
    out[: w * h] = plane(y, py, v, 16).ravel()
    o = w * h
    for _ in range(2):
        out[o:o + cw * ch] = plane(cur[o:o + cw * ch].reshape(ch, cw), prev[o:o + cw * ch].reshape(ch, cw), mv.astype(np.int64), 8).ravel()
        o += cw * ch
    return out, (v.astype(np.int8), sad.astype(np.uint16))


def clip(frames, w, h, mode, R=8, fields=None):
    """(filtered pictures, [(v, sad)] per frame) of consecutive frames from the zero state; fields: [mv int8 [nby, nbx, 2]] per frame
    instead of the searched cost pass' of range R"""
    if fields is None:
        fields = [f[0] for f in ML.analyse(frames, w, h, R)[1]]
    state = np.zeros(w * h * 3 // 2, np.uint8)
    out, cells = [], []
    for f, mv in zip(frames, fields):
        state, c = frame(f, state, w, h, np.asarray(mv), mode)
        out.append(state)
        cells.append(c)
    return out, cells


def hash_noise(frames, amp=6, salt=77):
    """the clip plus uniform noise in -amp..amp per sample from the test clips' integer hash, clipped to 0..255"""
    import clips
    f = np.asarray(frames)
    n = (clips._hash_bytes(f.size, salt).astype(np.int64) % (2 * amp + 1) - amp).reshape(f.shape)
    return np.clip(f.astype(np.int64) + n, 0, 255).astype(np.uint8)


def luma_mse(a, b, w, h):
    return float(np.mean([((np.asarray(x[: w * h], np.int64) - np.asarray(y[: w * h], np.int64)) ** 2).mean() for x, y in zip(a, b)]))


def device_planes(lib, frames, w, h, resident, chunk, mode, R=8):
    """the same frames through the device layer (include/h264e_hip.h): the searched cost pass, then h264e_hip_mcdenoise_frames, `chunk`
    frames at a time in a pool of `resident` input slots; (pictures, [(v, sad)]) read back with h264e_hip_read_denoised and
    h264e_hip_mcdenoise_read_vectors.  lib: path of the product library or of the emulation."""
    import ctypes as C
    L = C.CDLL(lib)
    L.h264e_hip_pool_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_pool_destroy.argtypes = [C.c_void_p]
    L.h264e_hip_pool_destroy.restype = None
    L.h264e_hip_upload_i420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.h264e_hip_denoise_reset.argtypes = [C.c_void_p]
    L.h264e_hip_lookahead_search_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.h264e_hip_mcdenoise_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h264e_hip_mcdenoise_read_vectors.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.h264e_hip_read_denoised.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.h264e_hip_sync.argtypes = [C.c_void_p]
    L.h264e_hip_last_error.restype = C.c_char_p
    pool = C.c_void_p()
    assert L.h264e_hip_pool_create(C.byref(pool), 0, w, h, 1, resident) == 0, L.h264e_hip_last_error()
    fsz = w * h * 3 // 2
    nby, nbx = (h // 2) >> 3, (w // 2) >> 3
    out, cells = [], []
    try:
        assert L.h264e_hip_denoise_reset(pool) == 0, L.h264e_hip_last_error()
        assert L.h264e_hip_mcdenoise_frames(pool, 0, 1, mode, 1) != 0, "refused while the search has never run for the pool"
        assert b"motion field" in L.h264e_hip_last_error()
        for f0 in range(0, len(frames), chunk):
            part = np.ascontiguousarray(np.asarray(frames[f0:f0 + chunk], np.uint8).reshape(-1, fsz))
            rec = np.zeros((part.shape[0], 3), np.uint64)
            for i in range(part.shape[0]):
                assert L.h264e_hip_upload_i420(pool, (f0 + i) % resident, 1, part[i].ctypes.data) == 0, L.h264e_hip_last_error()
            assert L.h264e_hip_lookahead_search_frames(pool, f0, part.shape[0], R, rec.ctypes.data, None) == 0, L.h264e_hip_last_error()
            assert L.h264e_hip_mcdenoise_frames(pool, f0, part.shape[0], mode, int(f0 == 0)) == 0, L.h264e_hip_last_error()
            for i in range(part.shape[0]):
                buf, c = np.empty(fsz, np.uint8), np.zeros((nby, nbx), np.uint32)
                if resident > 1 or i == part.shape[0] - 1:          # a single-slot pool keeps the last picture only
                    assert L.h264e_hip_read_denoised(pool, (f0 + i) % resident, buf.ctypes.data) == 0, L.h264e_hip_last_error()
                    out.append(buf)
                else:
                    out.append(None)
                assert L.h264e_hip_mcdenoise_read_vectors(pool, f0 + i, c.ctypes.data) == 0, L.h264e_hip_last_error()
                cells.append((np.stack([(c & 0xff).astype(np.uint8).view(np.int8), ((c >> 8) & 0xff).astype(np.uint8).view(np.int8)], axis=-1), (c >> 16).astype(np.uint16)))
        assert L.h264e_hip_sync(pool) == 0, L.h264e_hip_last_error()
    finally:
        L.h264e_hip_pool_destroy(pool)
    return out, cells
