"""numpy restatement of the lookahead's cost tree (include/h264e_mi355x.h H264E_clip_set_lookahead_tree, enc_lookahead_tree.h): cost
propagated backwards through the motion field of the searched cost pass, summed per frame, turned into QP offsets inside a window, and
the window controller with those offsets.  L_f, the blocks, intra(b), inter(b) and mv(b) are lookahead_motion_model's; this integer
definition is the definition the product is tested against:

    window [a, b), horizon e = min(b + ahead, n); in_f(t) = 0 for all blocks of all frames in [a, e)
    for f = e - 1 down to a + 1, unless key(f), every block s = (sx, sy) of frame f:
        i = intra_f(s), c = min(i, inter_f(s)), g = min(in_f(s), 2^40); amt = g if i == 0 else ((i + g)*(i - c)) // i
        x = 8sx + dx, y = 8sy + dy; tx, ox = x >> 3, x & 7; ty, oy = y >> 3, y & 7
        in_{f-1}(tx + u, ty + v) += (amt*wx*wy) >> 6 for u, v in {0, 1}, wx = ox if u else 8 - ox, wy likewise, weight 0 left out
    S(f) = min(sum_t min(in_f(t), 2^40), 2^48)
    lg(f) = 0 if I(f) == 0 else, with r = ((I + S) << 8) // I and e2 = floor(log2 r) - 8: 256*e2 + ((r >> e2) - 256)
    delta(f) = -min(6, (strength*lg(f) + 512) >> 10)

All values here stay below 2^56 (asserted), so int64 arrays hold them; np.add.at adds in any order, as the kernel's atomics do.
"""
import numpy as np

import lookahead_model as M
import lookahead_motion_model as ML

IN_MAX, SUM_MAX = 1 << 40, 1 << 48
DELTA_MAX = 6


def analyse(clip, w, h, R):
    """((I, P, N), fields as ML.analyse gives them, intra int64 [nby, nbx] per frame)"""
    rec, fields = ML.analyse(clip, w, h, R)
    intra = []
    for f in range(len(clip)):
        b = M._blocks(M.lowres(np.asarray(clip[f][: w * h]).reshape(h, w)))
        intra.append(np.abs(b - ((b.sum(axis=2) + 32) >> 6)[:, :, None]).sum(axis=2))
    return rec, fields, intra


def amounts(intra, inter, g_in):
    """amt of every block of a frame from its costs and what it received"""
    i, g = intra.astype(np.int64), np.minimum(g_in, IN_MAX)
    c = np.minimum(i, inter.astype(np.int64))
    assert int((i + g).max()) * int((i - c).max()) < 1 << 62
    return np.where(i == 0, g, ((i + g) * (i - c)) // np.maximum(i, 1))


def targets(mv):
    """per block: (tx, ox, ty, oy) of its displaced position"""
    nby, nbx = mv.shape[:2]
    x = 8 * np.arange(nbx)[None, :] + mv[:, :, 0].astype(np.int64)
    y = 8 * np.arange(nby)[:, None] + mv[:, :, 1].astype(np.int64)
    return x >> 3, x & 7, y >> 3, y & 7


def scatter(amt, mv):
    """what the blocks of frame f add to in_{f-1}: int64 [nby, nbx]"""
    out = np.zeros(amt.shape, np.int64)
    tx, ox, ty, oy = targets(mv)
    for v in (0, 1):
        for u in (0, 1):
            w = (ox if u else 8 - ox) * (oy if v else 8 - oy)
            sel = w > 0
            np.add.at(out, (ty[sel] + v, tx[sel] + u), (amt[sel] * w[sel]) >> 6)
    assert int(out.max(initial=0)) < 1 << 56
    return out


def run(intra, fields, kinds, a, e):
    """one run over frames [a, e): ({f: in_f}, {f: S(f)}, {f: sum of amt_f} for the frames that scatter)"""
    maps = {f: np.zeros(intra[f].shape, np.int64) for f in range(a, e)}
    amts = {}
    for f in range(e - 1, a, -1):
        if kinds[f]:
            continue
        amt = amounts(intra[f], fields[f][1], maps[f])
        amts[f] = int(amt.sum())
        maps[f - 1] += scatter(amt, fields[f][0])
    sums = {f: min(int(np.minimum(maps[f], IN_MAX).sum()), SUM_MAX) for f in range(a, e)}
    return maps, sums, amts


def log2_256(I, S):
    I, S = int(I), int(S)
    if I == 0:
        return 0
    r = ((I + S) << 8) // I
    e2 = r.bit_length() - 1 - 8
    return 256 * e2 + ((r >> e2) - 256)


def delta(I, S, strength):
    return -min(DELTA_MAX, (strength * log2_256(I, S) + 512) >> 10)


def windows(rec, fields, intra, kinds, W, strength, ahead):
    """the runs of all windows: (maps [n] of the frame's own window, S int [n], delta int8 [n])"""
    n = len(kinds)
    maps, S, d = [None] * n, [0] * n, np.zeros(n, np.int8)
    for a in range(0, n, W):
        b = min(a + W, n)
        m, s, _ = run(intra, fields, kinds, a, min(b + ahead, n))
        for f in range(a, b):
            maps[f], S[f], d[f] = m[f].astype(np.uint64), s[f], delta(rec[0][f], s[f], strength)
    return maps, np.array(S, np.uint64), d


def plan(cost, kinds, header_bits, actual_bits, kbps, W, deltas, qmin=10, qmax=50, search=ML.MAX_RANGE, qp_step=M.QP_STEP):
    """The controller with offsets, replayed as M.plan replays the one without: window j has a base QP Q_j, the smallest in [lo_j, hi_j]
    -- around Q_{j-1} -- whose predicted window sum with frame f at q_f = clamp(Q_j + deltas[f], qmin, qmax) fits T_j; the calibration
    sums every frame at its own q_f.  Returns (qp uint8 [n], base uint8 [n]).  With deltas all zero it is ML.plan."""
    n = len(kinds)
    dfb = kbps * 1000 // 8 // 30
    T = 8 * dfb * W
    k = [ML.K0_SEARCH if search else M.K0[0], M.K0[1]]
    debt = 0
    qp, base = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for a in range(0, n, W):
        b = min(a + W, n)
        carry = max(-(T // 2), min(T // 2, debt))
        Tj = 8 * dfb * (b - a) + carry
        c = [int(cost[0][f]) if kinds[f] else int(cost[1][f]) for f in range(a, b)]
        lo, hi = (max(qmin, int(base[a - 1]) - qp_step), min(qmax, int(base[a - 1]) + qp_step)) if a else (qmin, qmax)

        def qf(Q, f):
            return max(qmin, min(qmax, Q + int(deltas[f])))

        Q = lo
        while Q < hi and sum(header_bits[kinds[f]] + M.texture_bits(k[kinds[f]], c[f - a], qf(Q, f), kinds[f]) for f in range(a, b)) > Tj:
            Q += 1
        base[a:b] = Q
        for f in range(a, b):
            qp[f] = qf(Q, f)
        debt += 8 * dfb * (b - a) - sum(int(actual_bits[f]) for f in range(a, b))
        for t in (0, 1):
            fr = [f for f in range(a, b) if kinds[f] == t]
            den = sum(c[f - a] * M.LQ[t][min(int(qp[f]), 50) - 10] for f in fr)
            if fr and den:
                num = max(sum(int(actual_bits[f]) - header_bits[t] for f in fr), 0)
                k[t] = max(1, max(k[t] // 4, min((num << 24) // den, min(4 * k[t], M.K_MAX))))
    return qp, base
