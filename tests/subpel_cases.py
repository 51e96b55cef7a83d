"""The sub-sample stage of the partition search (enc_mb.h diamond_g after the full-sample scan; enc_kernels.h halfpel3_rows on sample pairs,
wave.h pk16 and avg4_u8) for tests/test_emu_subpel_arith.py and tests/test_gpu_subpel_arith.py: a model of the stage, and the smallest pictures on
which packed 16-bit and packed byte arithmetic can go wrong.

The model restates h264-lab.h:4999-5174 -- the full-sample scan as tests/scan_step_cases.py model_search states it (here it also hands out
the cache of the last centre and takes any QP), then the choice of the two probe directions from the four cached neighbour costs and the
seven probes in the reference's order with a strict `<`.  A probe's prediction is the oracle library's interp_luma (bound in
tests/test_stages.py), its vector cost the one of scan_step_cases._mv_cost.  Before it is trusted the model must reproduce the recorded
searches of the stage fixtures (model_reproduces_fixtures below, a test of its own in test_emu_subpel_arith.py).

Every case is one call of stage hook 8: a 96x96 reference picture, a 16x16 input, speed 0 (sub-sample stage ON)."""
import ctypes as C
import functools

import numpy as np

import scan_step_cases as K
import test_stage_edges as E
import test_stages as S

PAD = 48                      # the model reads the picture with its border extended: every vector of a case or fixture stays inside
LAMBDA_MV_Q4 = (13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 13, 14, 15, 15, 16, 17, 18, 20, 21, 23, 24, 28, 32, 37, 41, 45, 53, 62, 70, 79,
                87, 105, 123, 140, 158, 176, 195, 214, 234, 253, 272, 406, 541, 675, 810, 944, 895, 845, 796, 746, 697, 697)    # tables.h k_lambda_mv_q4
PROBES = ("02", "01", "20", "10", "11", "22", "12")          # steps of (pq, sq) from the full-sample winner, the reference's order
PROBE_STEPS = ((2, 0), (1, 0), (0, 2), (0, 1), (1, 1), (2, 2), (2, 1))
GEOMETRIES = ((0, 0, 16, 16), (0, 8, 16, 8), (8, 0, 8, 16), (8, 8, 8, 8))


def _tap6(a, b, c, d, e, f):
    return a - 5 * b + 20 * c + 20 * d - 5 * e + f


class Model:
    """one reference picture (96x96 uint8) under the model"""

    def __init__(self, ref):
        self.pad = np.pad(ref, PAD, mode="edge").astype(np.uint8)
        self.buf = self.pad.tobytes()
        self.stride = self.pad.shape[1]
        self.L = S._olib()

    def predict(self, px, py, w, h, v):
        """h x w prediction of the partition at (px, py) for the quarter-sample vector v (absolute in the picture)"""
        dst = C.create_string_buffer(256)
        self.L.interp_luma(self.buf, self.stride, 4 * (px + PAD) + v[0], 4 * (py + PAD) + v[1], w, h, dst)
        return np.frombuffer(dst.raw, np.uint8).reshape(16, 16)[:h, :w].copy()

    def _sad_full(self, cur, px, py, w, h, v):
        x, y = PAD + px + (v[0] >> 2), PAD + py + (v[1] >> 2)
        return int(np.abs(self.pad[y: y + h, x: x + w].astype(np.int32) - cur[py: py + h, px: px + w].astype(np.int32)).sum())

    def full_search(self, cur, px, py, w, h, mv, pred, min_sad, rng, lam):
        """scan_step_cases.model_search at any lambda; returns (cost, mv, cache[0:4] of the last centre)"""
        cost_of = lambda v: self._sad_full(cur, px, py, w, h, v) + (((K._se_len(v[0] - pred[0]) + K._se_len(v[1] - pred[1])) * lam) >> 4)
        inside = lambda v: rng[0] <= v[0] <= rng[2] and rng[1] <= v[1] <= rng[3]
        mv = tuple(mv)
        while True:
            d, loops, prev = 0, 4, -1
            cache = [0xffff] * 8
            while loops:
                v = (mv[0] + K.STEP[d][0], mv[1] + K.STEP[d][1])
                if inside(v) and cache[d] == 0xffff:
                    cost = cost_of(v)
                    cache[d] = cost & 0xffff
                    if cost < min_sad:
                        corner = cache[4 + d] if prev >= 0 else 0xffff
                        cache[4:8] = cache[0:4]
                        cache[0:4] = [0xffff] * 4
                        if prev >= 0:
                            cache[prev ^ 1] = corner
                        cache[d ^ 1] = min_sad & 0xffff
                        prev, mv, min_sad = d, v, cost
                        d -= 1
                        loops = 5
                d = (d + 1) & 3
                loops -= 1
            pri = 2 if cache[3] >= cache[2] else 3
            sec = 0 if cache[1] >= cache[0] else 1
            v = (mv[0] + K.STEP[pri][0] + K.STEP[sec][0], mv[1] + K.STEP[pri][1] + K.STEP[sec][1])
            if inside(v):
                cost = cost_of(v)
                if cost < min_sad:
                    mv, min_sad = v, cost
                    continue
            return min_sad, mv, cache[0:4]

    def search(self, cur, px, py, w, h, mv, pred, min_sad, qp, speed, rng, lim):
        """what hook 8 returns: dict(cost, mv, pred = h x w rows, and what the sub-sample stage met: `sub` None when it did not run)"""
        lam = LAMBDA_MV_Q4[qp]
        cost, mv, (c0, c1, c2, c3) = self.full_search(cur, px, py, w, h, mv, pred, min_sad, rng, lam)
        out = dict(full_mv=mv, sub=None)
        if not (speed < 9 and lim[0] + 16 <= mv[0] <= lim[2] - 16 and lim[1] + 16 <= mv[1] <= lim[3] - 16):
            out.update(cost=cost, mv=mv, pred=self.predict(px, py, w, h, mv))
            return out
        pq, sq, ms1, ms2 = (0, -1), (-1, 0), c1, c3
        if c3 >= c2:
            pq, ms2 = (0, 1), c2
        if c1 >= c0:
            sq, ms1 = (1, 0), c0
        if ms2 > ms1:
            pq, sq = sq, pq
        best, vbest, pbest = None, mv, None
        blk = cur[py: py + h, px: px + w].astype(np.int32)
        for name, (a, b) in zip(PROBES, PROBE_STEPS):
            v = (mv[0] + a * pq[0] + b * sq[0], mv[1] + a * pq[1] + b * sq[1])
            p = self.predict(px, py, w, h, v)
            c = int(np.abs(p.astype(np.int32) - blk).sum()) + (((K._se_len(v[0] - pred[0]) + K._se_len(v[1] - pred[1])) * lam) >> 4)
            if c < cost:
                cost, best, vbest, pbest = c, name, v, p
        vdg = (pq[0] + sq[0], pq[1] + sq[1])
        out.update(cost=cost, mv=vbest, pred=pbest if pbest is not None else self.predict(px, py, w, h, mv),
                   sub=dict(winner=best, hp_ox=int(vdg[0] < 0), hp_oy=int(vdg[1] < 0), pq_vertical=int(pq[0] == 0)))
        out["sub"].update(self._filter_extremes(px, py, w, h, mv, out["sub"]))
        # diamond_g's footprint test (rv_inside) against the hook's window, 64 x 64 from (32 - 24, 32 - 24): inside it the three planes come
        # from halfpel3_rows when the hook is asked for the window, outside it from interp_luma4 whatever the hook is asked for
        fx0, fy0 = px + (mv[0] >> 2), py + (mv[1] >> 2)
        out["sub"]["in_window"] = fx0 - 5 >= 8 and fy0 - 3 >= 8 and fx0 + w + 4 < 72 and fy0 + h + 3 < 72
        return out

    def _filter_extremes(self, px, py, w, h, mv, sub):
        """what the three half-sample planes of this search put through the filters: min / max of the horizontal and of the vertical
        first stage, of the second stage's symmetric pair sums and of its result before the clamp"""
        p = self.pad.astype(np.int64)
        fx0, fy0 = PAD + px + (mv[0] >> 2), PAD + py + (mv[1] >> 2)
        ix, iy = fx0 - sub["hp_ox"], fy0 - sub["hp_oy"]                 # the 2x2 integer cell that holds the three half-sample positions
        cols = lambda k: p[iy - 2: iy + h + 3, ix + k: ix + k + w]
        th = _tap6(cols(-2), cols(-1), cols(0), cols(1), cols(2), cols(3))                   # rows iy - 2 .. iy + h + 2
        rows = lambda k: p[iy + k: iy + k + h, fx0: fx0 + w]
        tv = _tap6(rows(-2), rows(-1), rows(0), rows(1), rows(2), rows(3))
        t = lambda k: th[k: k + h]
        af, be, cd = t(0) + t(5), t(1) + t(4), t(2) + t(3)
        centre = (af - 5 * be + 20 * cd + 512) >> 10
        pair = np.stack([af, be, cd])
        return dict(h1=(int(th.min()), int(th.max())), v1=(int(tv.min()), int(tv.max())), pair=(int(pair.min()), int(pair.max())),
                    centre=(int(centre.min()), int(centre.max())))


# ------------------------------------------------------------------ the recorded searches of the reference

def model_reproduces_fixtures():
    """the model on every recorded `diamond` case of tests/golden/stages.json and stage_edges.json (the cases that
    test_emu_scan_step.diamond_fixture_cases walks): cost, vector, prediction.  Returns (cases, cases whose sub-sample stage ran)"""
    n = ran = 0
    models = {}
    for fix, ref_of, b in ((S.FIX, lambda c: S._b(S.FIX["diamond_refs"][c["ref"]]["pic"]), S._b), (E.FIX, lambda c: E._diamond_ref(), E._b)):
        for ci, c in enumerate(fix["diamond"]):
            ref = ref_of(c)
            if ref not in models:
                models[ref] = Model(np.frombuffer(ref, np.uint8).reshape(96, 96))
            cur = np.frombuffer(b(c["cur"]), np.uint8).reshape(16, 16)
            r = models[ref].search(cur, c["px"], c["py"], c["w"], c["h"], c["mv_in"], c["mv_pred"], c["min_sad_in"], c["qp"], c["speed"], c["range"], c["limit"])
            assert (r["cost"], list(r["mv"])) == (c["cost"], c["mv"]), ("the model against the recorded search", ci, c["w"], c["h"], r["cost"], r["mv"], c["cost"], c["mv"])
            stride = 16 if fix is S.FIX else c["w"]             # (stages.json records the 16x16 buffer, stage_edges.json the partition's rows)
            want = np.frombuffer(b(c["pred"]), np.uint8)[: stride * c["h"]].reshape(c["h"], stride)[:, : c["w"]]
            assert (r["pred"] == want).all(), ("the model's prediction against the recorded one", ci)
            n += 1
            ran += r["sub"] is not None
    return n, ran


# ------------------------------------------------------------------ pictures

P3A, P3B = (255, 0, 255), (0, 255, 0)                              # 255,0,255,255,0,255 -> tap6 10710; 0,255,0,0,255,0 -> -2550
P6A, P6B = (0, 0, 255, 255, 0, 0), (255, 255, 0, 0, 255, 255)      # the runs at which one clamp side after the other is reached
P2A, P2B = (255, 0), (0, 255)
ONES = (255,)


def _line(pat):
    return np.array([pat[i % len(pat)] for i in range(96)], np.uint8)


def _product(rowpat, colpat):
    """255 where the row's and the column's pattern are both 255"""
    return np.minimum.outer(_line(rowpat), _line(colpat)).astype(np.uint8)


def _smooth(seed):
    """low-pass noise stretched to the full range: a picture on which the cost has ONE valley, so that a chosen sub-sample position wins"""
    r = np.random.RandomState(seed)
    a = r.randint(0, 256, (112, 112)).astype(np.float64)
    k = np.ones(7) / 7
    for _ in range(2):
        a = np.apply_along_axis(lambda m: np.convolve(m, k, mode="same"), 0, a)
        a = np.apply_along_axis(lambda m: np.convolve(m, k, mode="same"), 1, a)
    a = a[8:104, 8:104]
    return np.clip((a - a.min()) * 255.0 / (a.max() - a.min()), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def pictures():
    """[(name, 96x96 uint8)]"""
    out = []
    for name, pat in (("p3a", P3A), ("p3b", P3B), ("p6a", P6A), ("p6b", P6B)):
        out.append(("columns_" + name, _product(ONES, pat)))
        out.append(("rows_" + name, _product(pat, ONES)))
    for rn, rp in (("p3a", P3A), ("p3b", P3B)):
        for cn, cp in (("p3a", P3A), ("p3b", P3B)):
            out.append(("product_%s_%s" % (rn, cn), _product(rp, cp)))
    out.append(("product_p6a_p6a", _product(P6A, P6A)))
    out.append(("product_p6b_p6b", _product(P6B, P6B)))
    out.append(("product_p6a_p3b", _product(P6A, P3B)))
    out.append(("product_p3a_p6b", _product(P3A, P6B)))
    out.append(("stripes_columns", _product(ONES, P2A)))
    out.append(("stripes_rows", _product(P2B, ONES)))
    y, x = np.mgrid[0:96, 0:96]
    out.append(("checkerboard", (((x + y) & 1) * 255).astype(np.uint8)))
    out.append(("flat_255", np.full((96, 96), 255, np.uint8)))
    out.append(("flat_0", np.zeros((96, 96), np.uint8)))
    for seed in (1, 2, 3):
        out.append(("noise_%d" % seed, np.random.RandomState(7000 + seed).randint(0, 256, (96, 96)).astype(np.uint8)))
    for _, p in out:
        p.setflags(write=False)
    return out


# ------------------------------------------------------------------ cases

QP = 26


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, ref bytes, cur bytes, hook arguments without window / lane group, result of the model)].
    On the pattern and noise pictures the input is the model's prediction at a sub-sample position next to the start (the position walks
    over the 5 x 5 quarter-sample offsets of -2 .. 2 with the case number), so that every plane of the stage is the winner's somewhere and
    its samples reach the output; on the smooth pictures every one of the 25 offsets is a case: there the cost has one valley, the
    full-sample scan ends on the sample next to the target and each of the seven probes -- and none -- wins in turn."""
    out = []
    n = 0

    def add(name, M, ref, px, py, w, h, start, off, noise=None):
        target = (start[0] + off[0], start[1] + off[1])
        cur = np.full((16, 16), 128, np.uint8)
        cur[py: py + h, px: px + w] = M.predict(px, py, w, h, target)
        if noise is not None:
            cur = np.clip(cur.astype(np.int32) + noise.randint(-3, 4, (16, 16)), 0, 255).astype(np.uint8)
        pred = (start[0] + 2 * off[1] - 3, start[1] - 2 * off[0] + 5)
        rng = (start[0] - 32, start[1] - 32, start[0] + 32, start[1] + 32)
        lim = (0, 0, 4 * 96, 4 * 96)
        sad0 = M._sad_full(cur, px, py, w, h, start) + (((K._se_len(start[0] - pred[0]) + K._se_len(start[1] - pred[1])) * LAMBDA_MV_Q4[QP]) >> 4)
        r = M.search(cur, px, py, w, h, start, pred, sad0, QP, 0, rng, lim)
        args = [px, py, w, h, start[0], start[1], pred[0], pred[1], sad0, QP, 0] + list(rng) + list(lim)
        out.append(("%s_%dx%d_%+d%+d" % (name, w, h, off[0], off[1]), ref.tobytes(), cur.tobytes(), args, r))

    for name, ref in pictures():
        M = Model(ref)
        for px, py, w, h in GEOMETRIES:
            start = (128 + 4 * ((n * 5) % 7 - 3), 128 + 4 * ((n * 3) % 5 - 2))
            add(name, M, ref, px, py, w, h, start, ((n * 7) % 5 - 2, (n * 7) // 5 % 5 - 2))
            n += 1
    for seed in (11, 12):
        ref = _smooth(seed)
        M = Model(ref)
        k = 0
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                px, py, w, h = GEOMETRIES[(k + seed) % 4]
                add("smooth_%d" % seed, M, ref, px, py, w, h, (128 + 4 * (k % 3 - 1), 128 + 4 * (k % 4 - 2)), (dx, dy), noise=np.random.RandomState(seed * 100 + k))
                k += 1
    return out


def coverage():
    """what the case list meets, for the assertions of test_emu_subpel_arith.py"""
    subs = [(c[3][2:4], c[4]["sub"]) for c in cases()]
    assert all(s is not None for _, s in subs), "a case whose sub-sample stage does not run"
    lo = lambda k: min(s[k][0] for _, s in subs)
    hi = lambda k: max(s[k][1] for _, s in subs)
    return dict(h1=(lo("h1"), hi("h1")), v1=(lo("v1"), hi("v1")), pair=(lo("pair"), hi("pair")), centre=(lo("centre"), hi("centre")),
                winners={s["winner"] for _, s in subs}, hp_ox={s["hp_ox"] for _, s in subs}, hp_oy={s["hp_oy"] for _, s in subs},
                pq_vertical={s["pq_vertical"] for _, s in subs}, geometries={tuple(g) for g, _ in subs},
                in_window={tuple(g) for g, s in subs if s["in_window"]}, out_of_window=sum(not s["in_window"] for _, s in subs))


def check_cases(run, groups=(0, 1, 2, 3)):
    """every case through stage hook 8 (`run` of test_stages._hook), from the LDS window (where the half-sample planes come from
    halfpel3_rows: a lane of a 16x16 partition owns four consecutive rows, of 16x8 / 8x16 two, of 8x8 one) and from memory, the first
    eight cases in every lane group: cost, vector, prediction rows.  Returns the number of hook calls"""
    calls = 0
    for window in (0, 1):
        for ci, (name, ref, cur, args, want) in enumerate(cases()):
            for grp in groups if ci < 8 else (ci % 4,):
                r = run(8, ref + cur, args + [window, grp], 16 + 256)
                got = np.frombuffer(r[:12], np.int32)
                assert (int(got[0]), (int(got[1]), int(got[2]))) == (want["cost"], tuple(want["mv"])), ("sub-sample search", name, window, grp, [int(v) for v in got], want["cost"], want["mv"], want["sub"])
                px, py, w, h = args[:4]
                rows = np.frombuffer(r[16:272], np.uint8).reshape(16, 16)[py: py + h, px: px + w]
                assert (rows == want["pred"]).all(), ("sub-sample search prediction", name, window, grp, want["sub"])
                calls += 1
    return calls


# ------------------------------------------------------------------ avg4_u8 (stage hook 16)

def avg4_all_pairs(run):
    """hook 16 writes avg4_u8 of every pair of bytes (pair n = 256 x + y in byte n of the output) in one launch; against the carry-free formula"""
    n = np.arange(65536, dtype=np.uint32)
    x, y = (n >> 8).astype(np.uint8).view(np.uint32), (n & 255).astype(np.uint8).view(np.uint32)
    want = (x | y) - (((x ^ y) >> 1) & 0x7f7f7f7f)
    got = np.frombuffer(run(16, b"\0" * 4, [], 65536), np.uint32)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("avg4_u8", int(bad[0]), hex(int(x[bad[0]])), hex(int(y[bad[0]])), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
    # (and the formula is the rounded average, byte by byte)
    assert (want.view(np.uint8) == (((n >> 8) + (n & 255) + 1) >> 1).astype(np.uint8)).all()
