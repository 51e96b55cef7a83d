"""The small streams of the partition search's chain step (enc_mb.h diamond_g: the packed SAD cache, the scan-order pick, the code
lengths carried from centre to centre) for tests/test_emu_scan_step.py and tests/test_gpu_scan_step.py: the smallest pictures in which the
scan can go wrong -- 64x64 and 96x80 (a cropped bottom row), 6 frames, GOP 6, speed 0 -- over the noise, extremes and pan generators, at
QP 10 and QP 51, in one and in two slices.  The oracle's stream, frame sizes and per-macroblock decision trace are computed once."""
import functools

import numpy as np

import clips
import oracle_lib

GOP = 6
FRAMES = 6
CASES = [(name, w, h, dict(qp=qp, speed=0, slices=sl))
         for w, h in ((64, 64), (96, 80)) for name in ("noise", "extremes", "pan") for qp in (10, 51) for sl in (0, 2)]
# (searches that end on the TOP of their range are the rarest: 6 in the 24 clips above, so two clips at 128x96 for the eight asked for)
CASES += [("extremes", 128, 96, dict(qp=51, speed=0, slices=sl)) for sl in (0, 2)]
CASE_IDS = ["%s_%dx%d_qp%d_slices%d" % (name, w, h, kw["qp"], max(kw["slices"], 1)) for name, w, h, kw in CASES]


@functools.lru_cache(maxsize=None)
def clip(i):
    name, w, h, _ = CASES[i]
    c = clips.make(name, w, h, FRAMES)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(i):
    """(stream, frame sizes, per frame the trace [(type, mvx, mvy)]) of case i"""
    _, w, h, kw = CASES[i]
    want, sizes = oracle_lib.encode_clip(clip(i), w, h, gop=GOP, **kw)
    o = oracle_lib.Encoder(w, h, gop=GOP, **kw)
    parts, traces = [], []
    for t in range(FRAMES):
        parts.append(o.encode(clip(i)[t]))
        traces.append([(typ, mvx, mvy) for typ, _, mvx, mvy, _ in o.trace()])
    o.close()
    assert b"".join(parts) == want, "the oracle's two entry points disagree"
    return want, sizes, traces


def encode(P, lib, i):
    """case i through the clip encoder of `lib` (None = the product library on the GPU): (stream, frame sizes, macroblock records)"""
    _, w, h, kw = CASES[i]
    ce = P.ClipEncoder(w, h, FRAMES, gop=GOP, lib=lib, keep_records=1, **kw)
    try:
        ce.upload(clip(i))
        out, sizes, st = ce.encode()
        assert st.spin_relaunches == 0
        recs = [ce.read_records(t) for t in range(FRAMES)]
    finally:
        ce.close()
    return out, sizes, recs


def check(what, i, out, sizes, recs):
    """bytes and frame sizes are the oracle's; every macroblock's type and mv[0] are its trace's: a failure names the macroblock"""
    want, want_sizes, traces = oracle(i)
    for t, (trace, got) in enumerate(zip(traces, recs)):
        assert len(trace) == len(got)
        for k, ((typ, mvx, mvy), (gx, gy, gt, _)) in enumerate(zip(trace, got)):
            assert gt == typ, "%s, %s: frame %d macroblock %d: type %d, oracle %d" % (CASE_IDS[i], what, t, k, gt, typ)
            if typ < 5:
                assert (gx, gy) == (mvx, mvy), "%s, %s: frame %d macroblock %d: mv (%d,%d), oracle (%d,%d)" % (CASE_IDS[i], what, t, k, gx, gy, mvx, mvy)
    assert sizes == want_sizes, "%s, %s: frame sizes %s, oracle %s" % (CASE_IDS[i], what, sizes, want_sizes)
    assert out == want, "%s, %s: the stream differs from the oracle's" % (CASE_IDS[i], what)


# ------------------------------------------------------------------ the full-sample scan at the stage hook, where truncation shows
#
# A cached cost only loses its upper bits when SAD + vector cost reaches 0x10000.  A 16x16 SAD is at most 65280, so the vector cost must
# add 256 or more: at QP 10 (lambda 13/16 per bit) that would take 316 bits, at QP 51 (43.6 per bit) the reference picture must lie
# within 0.4 per sample of the inverted input -- and a reconstruction at QP 51 is never that close to 0 / 255 (the dead-zone quantiser
# rounds towards the prediction, so nothing overshoots into the clip).  No stream at these QPs caches such a cost; the stage hook does,
# on pictures built for it: a dark reference under a bright input at QP 51, searched WITHOUT the sub-sample stage (speed 9), against the
# restatement below of the reference's loop as SURVEY.md F5 and h264-lab.h:4999-5077 describe it (one direction per iteration, a
# uint16_t cache[8] with the 0xffff sentinel, the corner rule, the diagonal probe and its restart).

LAMBDA_MV_Q4_QP51 = 697            # tables.h k_lambda_mv_q4[51]
STEP = ((4, 0), (-4, 0), (0, 4), (0, -4))


def _se_len(v):
    k = 2 * v - 1 if v > 0 else -2 * v
    return 2 * (k + 1).bit_length() - 1


def _mv_cost(v, pred):
    return ((_se_len(v[0] - pred[0]) + _se_len(v[1] - pred[1])) * LAMBDA_MV_Q4_QP51) >> 4


def _sad(ref, cur, px, py, w, h, v):
    x, y = px + (v[0] >> 2), py + (v[1] >> 2)
    return int(np.abs(ref[y: y + h, x: x + w].astype(np.int32) - cur[py: py + h, px: px + w].astype(np.int32)).sum())


def model_search(ref, cur, px, py, w, h, mv, pred, min_sad, rng, mask=0xffff):
    """(cost, mv, what it met) of the reference's full-sample search; ref 96x96, cur 16x16 (numpy uint8), vectors in quarter samples
    absolute in the picture, rng = (x0, y0, x1, y1).  mask = -1: what a cache of full-width costs would give -- NOT the reference"""
    inside = lambda v: rng[0] <= v[0] <= rng[2] and rng[1] <= v[1] <= rng[3]
    met = dict(trunc=0, corner=0, restarts=0)
    mv = tuple(mv)
    while True:
        d, loops, prev, moves, turned = 0, 4, -1, 0, 0
        cache = [0xffff] * 8
        while loops:
            v = (mv[0] + STEP[d][0], mv[1] + STEP[d][1])
            if inside(v) and cache[d] == 0xffff:
                cost = _sad(ref, cur, px, py, w, h, v) + _mv_cost(v, pred)
                cache[d] = cost & mask
                met["trunc"] |= cost >= 0x10000
                if cost < min_sad:
                    corner = cache[4 + d] if prev >= 0 else 0xffff
                    cache[4:8] = cache[0:4]
                    cache[0:4] = [0xffff] * 4
                    if prev >= 0:
                        cache[prev ^ 1] = corner
                    cache[d ^ 1] = min_sad & mask
                    turned |= prev >= 0 and prev != d
                    moves += 1
                    met["corner"] |= moves >= 3 and turned
                    prev, mv, min_sad = d, v, cost
                    d -= 1
                    loops = 5
            d = (d + 1) & 3
            loops -= 1
        pri = 2 if cache[3] >= cache[2] else 3
        sec = 0 if cache[1] >= cache[0] else 1
        v = (mv[0] + STEP[pri][0] + STEP[sec][0], mv[1] + STEP[pri][1] + STEP[sec][1])
        if inside(v):
            cost = _sad(ref, cur, px, py, w, h, v) + _mv_cost(v, pred)
            if cost < min_sad:
                mv, min_sad = v, cost
                met["restarts"] += 1
                continue
        return min_sad, mv, met


GEOMETRIES = ((0, 0, 16, 16), (0, 0, 16, 16), (0, 8, 16, 8), (8, 0, 8, 16), (8, 8, 8, 8))
# seeds of spark pictures (below) on which a cache of full-width costs ends the search elsewhere: found by a search over 40000 seeds
DECISIVE_SEEDS = (2522, 4991, 5039, 7838, 8837, 11657, 13139, 16025)


def _case(ref, cur, px, py, w, h, start, pred, rng):
    sad0 = _sad(ref, cur, px, py, w, h, start) + _mv_cost(start, pred)
    cost, mv, met = model_search(ref, cur, px, py, w, h, start, pred, sad0, rng)
    met["decisive"] = (cost, mv) != model_search(ref, cur, px, py, w, h, start, pred, sad0, rng, mask=-1)[:2]
    x, y = px + (mv[0] >> 2), py + (mv[1] >> 2)
    args = [px, py, w, h, start[0], start[1], pred[0], pred[1], sad0, 51, 9] + list(rng) + [0, 0, 4 * 96, 4 * 96]
    return ref.tobytes(), cur.tobytes(), args, cost, list(mv), ref[y: y + h, x: x + w].tobytes(), met


@functools.lru_cache(maxsize=None)
def stage_cases():
    """[(ref bytes, cur bytes, hook arguments without window / lane group, cost, mv, prediction rows, met)].
    Valley pictures, 16 x the four partition geometries (16x16 twice): a smooth valley of small values under sparse sparks as the
    reference, an input near 255 -- every SAD lies a little below its maximum, so that at 16x16 the costs straddle 0x10000.
    Spark pictures, 16x16 only: a black reference with sparse sparks of any height; the eight seeds are those where the truncated
    values order the neighbours differently AND the diagonal probe they choose wins, so that the truncation decides the result."""
    out = []
    for s in range(16):
        r = np.random.RandomState(1000 + s)
        yy, xx = np.mgrid[0:96, 0:96]
        cx, cy = 32 + r.randint(-10, 11), 32 + r.randint(-10, 11)
        valley = (np.abs(xx - cx) + np.abs(yy - cy)) // (6 + 3 * (s % 3))
        ref = np.minimum(valley + (r.randint(0, 40, (96, 96)) == 0) * r.randint(0, 24, (96, 96)), 255).astype(np.uint8)
        cur = (255 - r.randint(0, 3, (16, 16))).astype(np.uint8)
        for px, py, w, h in GEOMETRIES:
            start = (128 + 4 * r.randint(-6, 7), 128 + 4 * r.randint(-6, 7))
            pred = (start[0] + r.randint(-64, 65), start[1] + r.randint(-64, 65))
            half = (16, 40, 128)[s % 3]
            rng = (max(start[0] - half, 0), max(start[1] - half, 0), min(start[0] + half, 4 * (80 - px)), min(start[1] + half, 4 * (80 - py)))
            out.append(_case(ref, cur, px, py, w, h, start, pred, rng))
    for s in DECISIVE_SEEDS:
        r = np.random.RandomState(s)
        dens = (12, 25, 50)[s % 3]
        ref = ((r.randint(0, dens, (96, 96)) == 0) * r.randint(0, 256, (96, 96))).astype(np.uint8)
        cur = (255 - (r.randint(0, 8, (16, 16)) == 0) * r.randint(0, 30, (16, 16))).astype(np.uint8)
        start = (128 + 4 * r.randint(-6, 7), 128 + 4 * r.randint(-6, 7))
        pred = (start[0] + r.randint(-64, 65), start[1] + r.randint(-64, 65))
        out.append(_case(ref, cur, 0, 0, 16, 16, start, pred, (start[0] - 64, start[1] - 64, start[0] + 64, start[1] + 64)))
    return out


def check_stage_cases(run, groups=(0, 1, 2, 3)):
    """the cases through stage hook 8 (`run` of test_stages._hook), from the LDS window and from memory, in the named lane groups"""
    for window in (0, 1):
        for ci, (ref, cur, args, cost, mv, pred, _) in enumerate(stage_cases()):
            for grp in groups if ci < 10 else (ci % 4,):
                r = run(8, ref + cur, args + [window, grp], 16 + 256)
                got = np.frombuffer(r[:12], np.int32)
                assert (int(got[0]), [int(got[1]), int(got[2])]) == (cost, mv), ("full-sample search", window, grp, ci, args)
                px, py, w, h = args[:4]
                rows = np.frombuffer(r[16:272], np.uint8).reshape(16, 16)[py: py + h, px: px + w].tobytes()
                assert rows == pred, ("full-sample search prediction", window, grp, ci, args)
