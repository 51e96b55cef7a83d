"""numpy restatement of the lookahead rate control (include/h264e_mi355x.h H264E_clip_set_lookahead, enc_lookahead.h): the cost pass
and the window controller.  The reference has neither; these integer definitions are the definitions the product is tested against."""
import numpy as np

# the reference's bits-per-macroblock table (h264-lab.h rate control), [P, key][qp - 10]
LQ = (
    (664, 597, 530, 484, 432, 384, 341, 297, 262, 235, 198, 173, 153, 131, 114, 102, 84, 74, 64, 54, 47, 42, 35, 31, 26, 22, 20, 17,
     15, 13, 12, 10, 9, 9, 7, 7, 6, 5, 4, 1, 1),
    (1057, 975, 925, 868, 803, 740, 694, 630, 586, 547, 496, 457, 420, 378, 345, 318, 284, 258, 234, 210, 190, 178, 155, 141, 129,
     115, 102, 95, 82, 75, 69, 60, 55, 51, 45, 41, 40, 35, 31, 28, 24))
K0 = (15086, 14322)         # initial calibration factors, P and key frames (tools/lookahead_calibrate.py)
K_MAX, BITS_MAX = 1 << 40, 1 << 50
WINDOW_DEFAULT = 32
QP_STEP = 6                 # a window's QP is within this of the window's before it


def lowres(y):
    """L_f of a luma plane [h, w]: rounded 2x2 means, [h // 2, w // 2]"""
    h, w = y.shape
    y = y[: h // 2 * 2, : w // 2 * 2].astype(np.int64)
    return (y[0::2, 0::2] + y[0::2, 1::2] + y[1::2, 0::2] + y[1::2, 1::2] + 2) >> 2


def _blocks(l):
    """the 8x8 blocks that lie wholly inside l: [nby, nbx, 64]"""
    nby, nbx = l.shape[0] >> 3, l.shape[1] >> 3
    return l[: nby * 8, : nbx * 8].reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).reshape(nby, nbx, 64)


def costs(clip, w, h):
    """(I, P, N) per frame of a packed I420 clip [n, w*h*3/2]: uint64, uint64, int32"""
    n = len(clip)
    out_i, out_p, out_n = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32)
    prev = None
    for f in range(n):
        b = _blocks(lowres(np.asarray(clip[f][: w * h]).reshape(h, w)))
        m = (b.sum(axis=2) + 32) >> 6
        intra = np.abs(b - m[:, :, None]).sum(axis=2)
        inter = intra if prev is None else np.abs(b - prev).sum(axis=2)
        out_i[f], out_p[f], out_n[f] = intra.sum(), np.minimum(intra, inter).sum(), (intra < inter).sum()
        prev = b
    return out_i, out_p, out_n


def texture_bits(k, cost, q, key):
    return min((int(k) * int(cost) * LQ[key][min(q, 50) - 10]) >> 24, BITS_MAX)


def plan(cost, kinds, header_bits, actual_bits, kbps, W, qmin=10, qmax=50, trace=None, qp_step=QP_STEP):
    """The controller, replayed: cost = (I, P, N) as costs() returns them, kinds[f] = 1 for key frames, header_bits = (H of a P frame,
    H of a key frame), actual_bits[f] = coded bits of frame f (read only for windows that are finished when a later one is planned).
    Returns the QP of every frame.  trace (a list) receives (T_j, carry_j, k) per window.  qp_step: the definition's 6; another value
    (51 = no bound) shows what the bound changes, for tests that want to see it bite."""
    n = len(kinds)
    dfb = kbps * 1000 // 8 // 30
    T = 8 * dfb * W
    k = list(K0)
    debt = 0
    qp = np.zeros(n, np.uint8)
    for a in range(0, n, W):
        b = min(a + W, n)
        carry = max(-(T // 2), min(T // 2, debt))
        Tj = 8 * dfb * (b - a) + carry
        if trace is not None:
            trace.append((Tj, carry, tuple(k)))
        c = [int(cost[0][f]) if kinds[f] else int(cost[1][f]) for f in range(a, b)]
        lo, hi = (max(qmin, int(qp[a - 1]) - qp_step), min(qmax, int(qp[a - 1]) + qp_step)) if a else (qmin, qmax)
        q = lo
        while q < hi and sum(header_bits[kinds[f]] + texture_bits(k[kinds[f]], c[f - a], q, kinds[f]) for f in range(a, b)) > Tj:
            q += 1
        qp[a:b] = q
        # the window has been accepted: carry and calibration
        debt += 8 * dfb * (b - a) - sum(int(actual_bits[f]) for f in range(a, b))
        for t in (0, 1):
            fr = [f for f in range(a, b) if kinds[f] == t]
            den = sum(c[f - a] * LQ[t][min(q, 50) - 10] for f in fr)
            if fr and den:
                num = max(sum(int(actual_bits[f]) - header_bits[t] for f in fr), 0)
                k[t] = max(1, max(k[t] // 4, min((num << 24) // den, min(4 * k[t], K_MAX))))
    return qp


def parameter_set_bytes(stream):
    """length of SPS + PPS in front of a stream's first slice (start codes included)"""
    pos, found = 0, []
    while len(found) < 3:
        pos = stream.index(b"\x00\x00\x00\x01", pos)
        found.append(pos)
        pos += 4
    return found[2]
