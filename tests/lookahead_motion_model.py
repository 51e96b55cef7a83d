"""numpy restatement of the lookahead's cost pass with a motion search (include/h264e_mi355x.h H264E_clip_set_lookahead_search,
enc_lookahead_search.h).  L_f, the blocks, m(b) and intra(b) are lookahead_model's; this integer definition of inter(b) and mv(b) is the
definition the product is tested against:

    A = [0, 8*nbx) x [0, 8*nby); candidates d = (dx, dy), |dx|, |dy| <= R, whose 8x8 block at (8bx + dx, 8by + dy) lies wholly inside A
    sad(b, d) = sum over the block of |L_f(x, y) - L_{f-1}(x + dx, y + dy)|
    inter(b) = the smallest sad; mv(b) = the candidate that reaches it and is first by (|dx| + |dy|, dy, dx)
    frame 0: inter(b) = intra(b), mv(b) = (0, 0);  R = 0 is the pass without search
"""
import numpy as np

import lookahead_model as M

MAX_RANGE = 8
K0_SEARCH = 53818           # initial calibration factor of P frames with search (tools/lookahead_calibrate.py --search 8); key frames keep M.K0[1]


def ranked(R):
    """the displacements of range R in the order that breaks ties: [(dx, dy)]"""
    return sorted(((dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)), key=lambda d: (abs(d[0]) + abs(d[1]), d[1], d[0]))


def search(cur, prev, R):
    """(inter int64 [nby, nbx], mv int8 [nby, nbx, 2]) of two half-resolution pictures (M.lowres)"""
    nby, nbx = cur.shape[0] >> 3, cur.shape[1] >> 3
    hh, ww = 8 * nby, 8 * nbx
    cur, prev = cur[:hh, :ww].astype(np.int64), prev[:hh, :ww].astype(np.int64)
    best = np.full((nby, nbx), 1 << 40, np.int64)
    mv = np.zeros((nby, nbx, 2), np.int8)
    ys, xs = 8 * np.arange(nby)[:, None], 8 * np.arange(nbx)[None, :]
    for dx, dy in ranked(R):
        # the overlap of the picture and the picture displaced by d; blocks not wholly inside it have no such candidate
        y0, y1, x0, x1 = max(0, -dy), min(hh, hh - dy), max(0, -dx), min(ww, ww - dx)
        diff = np.full((hh, ww), 0, np.int64)
        diff[y0:y1, x0:x1] = np.abs(cur[y0:y1, x0:x1] - prev[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
        sad = diff.reshape(nby, 8, nbx, 8).sum(axis=(1, 3))
        inside = (ys + dy >= 0) & (ys + dy + 8 <= hh) & (xs + dx >= 0) & (xs + dx + 8 <= ww)
        take = inside & (sad < best)            # strictly smaller: an equal sad later in the order does not replace
        best[take] = sad[take]
        mv[take] = (dx, dy)
    return best, mv


def analyse(clip, w, h, R):
    """((I, P, N) per frame as M.costs gives them, [(mv int8 [nby, nbx, 2], cost uint16 [nby, nbx])] per frame)"""
    n = len(clip)
    out_i, out_p, out_n = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    fields = []
    prev = None
    for f in range(n):
        l = M.lowres(np.asarray(clip[f][: w * h]).reshape(h, w))
        b = M._blocks(l)
        m = (b.sum(axis=2) + 32) >> 6
        intra = np.abs(b - m[:, :, None]).sum(axis=2)
        if prev is None:
            inter, mv = intra, np.zeros(intra.shape + (2,), np.int8)
        else:
            inter, mv = search(l, prev, R)
        out_i[f], out_p[f], out_n[f] = intra.sum(), np.minimum(intra, inter).sum(), (intra < inter).sum()
        fields.append((mv, inter.astype(np.uint16)))
        prev = l
    return (out_i, out_p, out_n), fields


def costs(clip, w, h, R):
    return analyse(clip, w, h, R)[0]


def plan(cost, kinds, header_bits, actual_bits, kbps, W, search=MAX_RANGE, **kw):
    """M.plan with the searched costs; with search on, the controller starts from K0_SEARCH for P frames"""
    k0 = M.K0
    M.K0 = (K0_SEARCH, k0[1]) if search else k0
    try:
        return M.plan(cost, kinds, header_bits, actual_bits, kbps, W, **kw)
    finally:
        M.K0 = k0
