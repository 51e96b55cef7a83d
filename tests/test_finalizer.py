"""The frame finalizer's own functions (h264-lab_amd/csrc/enc_finalize.h "slice splice": splice_frame / splice_words / splice_put / put_ue64,
clusters_step / clusters_walk_range / JobWalk / device_clusters_walk, the `moved` check of finalize_commit) and the host's clusters_walk,
run through the test hook h264e_hip_selftest_finalizer on operands chosen for their edges, bit exact against tests/finalizer_model.py
and tests/golden/finalizer.json (made by `oracle/stage_harness.c finalizer` from the reference's own mv_clusters_update and
mv_round_qpel).  Three ways like test_stage_edges.py: the oracle's restatement (CPU), the kernel sources in the lane-loop emulation
build (CPU), the same on the GPU (-m gpu, one test per group of cases)."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import finalizer_model as M
import oracle_lib
import pkg
from finalizer_model import Bits

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "finalizer.json")))
NARGS, HDR = 96, 128
GUARD = 64
RUNS = [0, 1, 2, 3, 6, 7, 14, 15, 30, 31, 62, 63, 126, 127, 254, 255, 510, 511, 1022, 1023, 1024]       # both sides of every ue length step


# ------------------------------------------------------------------ the hook

class Hook:
    """one pool per picture size, made on first use"""

    def __init__(self, libpath):
        P = pkg.load_pkg()
        self.P = P
        self.L = L = P.load(libpath) if libpath else P.load()
        L.h264e_hip_pool_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.h264e_hip_pool_destroy.argtypes = [C.c_void_p]
        L.h264e_hip_selftest_finalizer.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32]
        L.h264e_hip_selftest_host_clusters_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.h264e_hip_last_error.restype = C.c_char_p
        self.pools = {}

    def pool(self, nmbx, nmby):
        if (nmbx, nmby) not in self.pools:
            p = C.c_void_p()
            assert self.L.h264e_hip_pool_create(C.byref(p), 0, 16 * nmbx, 16 * nmby, 1, 1) == 0, self.L.h264e_hip_last_error()
            self.pools[nmbx, nmby] = p
        return self.pools[nmbx, nmby]

    def run(self, geom, mode, args, data, nout):
        a = (C.c_int * NARGS)(*(list(args) + [0] * (NARGS - len(args))))
        out = C.create_string_buffer(nout)
        assert self.L.h264e_hip_selftest_finalizer(self.pool(*geom), mode, a, data, len(data), out, nout) == 0, self.L.h264e_hip_last_error()
        return out.raw

    def close(self):
        for p in self.pools.values():
            self.L.h264e_hip_pool_destroy(p)
        self.pools = {}


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    h = Hook(pkg.EMU_LIB)
    yield h
    h.close()


@pytest.fixture(scope="module")
def gpu():
    h = Hook(None)
    yield h
    h.close()


def _i32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def _even_split(nmby, n):
    rows, r = [], 0
    for k in range(n):
        rows.append(r)
        r += (nmby - r) // (n - k)
    return rows + [nmby]


# ------------------------------------------------------------------ splice: cases

def _rbits(rng, n):
    return Bits(rng.getrandbits(n), n) if n else Bits()


def _case(nmbx, nmby, mbs, rng, slice_type=0, slice_row=None, hdr_nbits=None, **kw):
    hdr_nbits = rng.randint(0, 56) if hdr_nbits is None else hdr_nbits
    c = {"geom": (nmbx, nmby), "slice_type": slice_type, "hdr_nal": rng.choice((0x41, 0x61, 0x65, 0x25)), "hdr": _rbits(rng, hdr_nbits),
         "slice_row": slice_row or [0, nmby], "mbs": mbs, "arena_reset": 1, "cursor": 0, "short_words": 0, "row_overflow": [], "far": [0] * nmby}
    c.update(kw)
    assert len(mbs) == nmbx * nmby
    return c


def _sparse(nmb, coded, rng, lens=(1, 9, 33, 70)):
    """all skipped but the macroblocks `coded`, which carry a few random bits"""
    mbs = [(1, Bits())] * nmb
    for i in coded:
        mbs[i] = (0, _rbits(rng, rng.choice(lens)))
    return mbs


def _random_mbs(nmb, rng, p_coded, slice_type=0):
    return [(0, _rbits(rng, rng.choice((1, 2, 8, 31, 32, 33, 64, 65, 200)))) if slice_type == 2 or rng.random() < p_coded else (1, Bits()) for _ in range(nmb)]


def alignment_cases(geom, nfulls, rems):
    """the bit position in front of the first row takes every value 0..31, crossed with first rows of 32*nfull + rem bits; the rows below
    it each leave another carry"""
    nmbx, nmby = geom
    rng = random.Random(1000 + nmbx)
    for pos in range(32):
        for nfull in nfulls:
            for rem in rems:
                mbs = _random_mbs(nmbx * nmby, rng, 0.5)
                col = pos % nmbx
                for x in range(nmbx):
                    mbs[x] = (0, _rbits(rng, 32 * nfull + rem)) if x == col else (1, Bits())
                # in front of the row: NAL byte, ue(0) = 1 bit, the header bits, ue(col)
                hn = (pos - 9 - M.ue(col).n) % 32
                hn += 32 if hn <= 24 and pos % 3 else 0
                c = _case(nmbx, nmby, mbs, rng, hdr_nbits=hn)
                assert (9 + hn + M.ue(col).n) % 32 == pos and hn <= 56
                yield c


def _tune_tail(c, target, modulo):
    """lengthen the last coded macroblock so that the last slice has `target` bits (mod `modulo`) in front of its stop bit"""
    nmbx = c["geom"][0]
    m0 = c["slice_row"][-2] * nmbx
    last = max(i for i, (s, _) in enumerate(c["mbs"]) if not s)
    assert last >= m0
    n = M.slice_bits(c["slice_type"], c["hdr_nal"], m0, c["hdr"], c["mbs"][m0:])[0].n
    b = c["mbs"][last][1]
    c["mbs"][last] = (0, b + Bits(0, (target - n) % modulo))
    assert M.slice_bits(c["slice_type"], c["hdr_nal"], m0, c["hdr"], c["mbs"][m0:])[0].n % modulo == target
    return c


def tail_cases(geom):
    """the stop bit as the 32nd bit of a word and as the first of a new one; RBSPs that end on a byte boundary and that do not; with and
    without a run behind the last coded macroblock"""
    nmbx, nmby = geom
    rng = random.Random(2000 + nmbx)
    for target in (31, 0, 1, 7, 8, 15, 23, 24, 30):
        for trailing in (0, 1):
            mbs = _random_mbs(nmbx * nmby, rng, 0.6)
            mbs[-1] = (1, Bits()) if trailing and nmbx * nmby > 1 else (0, _rbits(rng, 40))
            if nmbx * nmby == 1:
                mbs[0] = (0, _rbits(rng, 40))
            else:
                mbs[-2] = (0, _rbits(rng, 40))
            yield _tune_tail(_case(nmbx, nmby, mbs, rng), target, 32)


def run_cases(geom):
    """runs of every length on both sides of the ue length steps: between two coded macroblocks (trail + wholly skipped rows + lead), in
    front of the first one, behind the last one"""
    nmbx, nmby = geom
    nmb = nmbx * nmby
    rng = random.Random(3000 + nmbx)
    for r in RUNS:
        if r + 2 <= nmb:
            a = max(nmbx - 1 - r // 2, 0) if r + 2 + nmbx - 1 <= nmb else 0
            yield _case(nmbx, nmby, _sparse(nmb, [a, a + r + 1], rng), rng)
        if r + 1 <= nmb:
            yield _case(nmbx, nmby, _sparse(nmb, [r], rng), rng)
            yield _case(nmbx, nmby, _sparse(nmb, [nmb - 1 - r], rng), rng)
    # everything skipped: all_skipped, the RBSP is header + ue(nmb) + stop bit; an I slice: no runs, all_skipped 0
    yield _case(nmbx, nmby, [(1, Bits())] * nmb, rng)
    yield _case(nmbx, nmby, _random_mbs(nmb, rng, 1, 2), rng, slice_type=2)
    # a row without bits between coded rows
    if nmby >= 3:
        for r in range(1, nmby - 1, max(1, nmby // 5)):
            mbs = _random_mbs(nmb, rng, 0.7)
            mbs[r * nmbx: (r + 1) * nmbx] = [(1, Bits())] * nmbx
            yield _case(nmbx, nmby, mbs, rng)


def slice_cases(geom):
    """row-band slices with uneven rows; runs on both sides of every boundary; everything skipped; the cursor and the row flags"""
    nmbx, nmby = geom
    nmb = nmbx * nmby
    rng = random.Random(4000 + nmbx)
    splits = [[0, nmby]]
    if nmby >= 4:
        splits += [[0, 1, nmby], [0, nmby - 1, nmby], [0, 2, 3, nmby], list(range(4)) + [nmby]]
    if nmby >= 32:
        splits += [[0, 1, 3, 4, 9, 10, 11, 20, 21, 22, 23, 50, 51, 60, 61, 127, nmby], sorted(rng.sample(range(1, nmby), 15) + [0, nmby])]
    for sr in splits:
        for p in (0.0, 0.05, 0.5, 1.0):
            mbs = _random_mbs(nmb, rng, p)
            for r in sr[1:-1]:                          # skipped macroblocks on both sides of every boundary
                if p and nmbx > 1:
                    mbs[r * nmbx - 1] = mbs[r * nmbx] = (1, Bits())
                    mbs[r * nmbx - 2 if nmbx > 2 else r * nmbx + 1] = (0, _rbits(rng, 12))
            yield _case(nmbx, nmby, mbs, rng, slice_row=sr, arena_reset=rng.choice((0, 1)), cursor=rng.choice((0, 1, 37, 48, 1000, 4095)),
                        far=[rng.randint(0, 1000) for _ in range(nmby)], row_overflow=[rng.randrange(nmby)] if rng.random() < 0.3 else [])
        yield _case(nmbx, nmby, _random_mbs(nmb, rng, 1, 2), rng, slice_type=2, slice_row=sr, arena_reset=0, cursor=17)
    yield _case(nmbx, nmby, _random_mbs(nmb, rng, 0.5), rng, arena_reset=0, cursor=37)
    yield _case(nmbx, nmby, _random_mbs(nmb, rng, 0.5), rng, row_overflow=[nmby - 1], far=[7] * nmby)


def capacity_cases(geom):
    """the capacity exactly enough, and short by one word (and by more, so that the cut falls into a row's words)"""
    nmbx, nmby = geom
    nmb = nmbx * nmby
    rng = random.Random(5000 + nmbx)
    for sr in ([0, nmby], [0, 1, nmby] if nmby > 1 else [0, nmby]):
        for tail in (0, 5, 31):
            for short in (0, 1, 2, 40):
                mbs = _random_mbs(nmb, rng, 0.6)
                mbs[-1] = (0, _rbits(rng, 3000))
                yield _tune_tail(_case(nmbx, nmby, mbs, rng, slice_row=sr, arena_reset=0, cursor=21, short_words=short), tail, 32)


def random_cases(geom, n):
    nmbx, nmby = geom
    rng = random.Random(6000 + nmbx)
    for _ in range(n):
        ns = rng.randint(1, min(nmby, 16))
        sr = sorted(rng.sample(range(1, nmby), ns - 1) + [0, nmby])
        st = rng.choice((0, 0, 0, 2))
        yield _case(nmbx, nmby, _random_mbs(nmbx * nmby, rng, rng.choice((0.02, 0.3, 0.9)), st), rng, slice_type=st, slice_row=sr,
                    arena_reset=rng.choice((0, 1)), cursor=rng.randint(0, 5000), far=[rng.randint(0, 99) for _ in range(nmby)])


def check_splice(hook, c):
    nmbx, nmby = c["geom"]
    st = c["slice_type"]
    rows = [M.row_wave(st, c["mbs"][r * nmbx: (r + 1) * nmbx]) for r in range(nmby)]
    # the capacity: what the frame needs in whole words (the model with room to spare says how much), less short_words
    free = M.frame(nmbx, st, c["hdr_nal"], c["hdr"], c["slice_row"], c["mbs"], c["arena_reset"], c["cursor"], 1 << 22, 0)
    last = free["nbytes"] - free["slice_nbytes"][-1]
    cap = free["start"] + last + (free["slice_nbytes"][-1] + 3) // 4 * 4 - 4 * c["short_words"]
    want = M.frame(nmbx, st, c["hdr_nal"], c["hdr"], c["slice_row"], c["mbs"], c["arena_reset"], c["cursor"], cap, GUARD, c["row_overflow"], c["far"])
    assert want["overflow"] == int(bool(c["short_words"] or c["row_overflow"]))
    meta = np.zeros((nmby, 4), np.int32)
    words = []
    for r, (lead, trail, bits) in enumerate(rows):
        meta[r] = [bits.n, lead, trail, int(r in c["row_overflow"])]
        words.append(np.frombuffer(bits.bytes(4), ">u4").astype("<u4").tobytes())
    sr = c["slice_row"] + [0] * (17 - len(c["slice_row"]))
    args = [st, c["hdr_nal"], c["hdr"].n, _i32(c["hdr"].v & 0xffffffff), _i32(c["hdr"].v >> 32), len(c["slice_row"]) - 1, c["arena_reset"], c["cursor"], cap, GUARD] + sr
    data = meta.tobytes() + np.array(c["far"], np.int32).tobytes() + b"".join(words)
    out = hook.run(c["geom"], 1, args, data, HDR + cap + GUARD)
    h = np.frombuffer(out[:HDR], np.int32)
    ns = len(c["slice_row"]) - 1
    got = {"start": int(h[1]), "nbytes": int(h[2]), "overflow": int(h[3]), "all_skipped": int(h[4]), "far_reads": int(h[5]), "slice_nbytes": [int(v) for v in h[8: 8 + ns]]}
    what = {k: v for k, v in c.items() if k not in ("mbs", "hdr")}
    assert h[0] == 0, what
    assert got == {k: v for k, v in want.items() if k != "arena"}, (what, [r[:2] + (r[2].n,) for r in rows])
    arena = out[HDR:]
    if arena != want["arena"]:
        i = next(i for i in range(len(arena)) if arena[i] != want["arena"][i])
        raise AssertionError(("arena differs from byte %d of %d" % (i, len(arena)), arena[i: i + 8].hex(), want["arena"][i: i + 8].hex(), got, what, [r[:2] + (r[2].n,) for r in rows]))
    # every slice starts 16-byte aligned, and nothing behind the capacity was touched
    assert want["start"] % 16 == 0 and arena[cap:] == bytes([M.SENTINEL]) * GUARD
    return want


SMALL, TALL, MID, WIDE = (1, 1), (1, 128), (4, 6), (480, 4)


def splice_alignment(hook, rem):
    for c in alignment_cases(MID, (0, 1, 63, 64, 65, 129), (rem,)):
        check_splice(hook, c)
    for c in alignment_cases(SMALL, (1, 64, 65), (rem,)):
        check_splice(hook, c)


def splice_tails_and_capacity(hook):
    for g in (SMALL, MID, TALL):
        for c in tail_cases(g):
            check_splice(hook, c)
    over = 0
    for g in (SMALL, MID, WIDE):
        for c in capacity_cases(g):
            over += check_splice(hook, c)["overflow"]
    assert over >= 30


def splice_runs(hook):
    seen = set()
    for g in (WIDE, TALL, MID, SMALL):
        for c in run_cases(g):
            w = check_splice(hook, c)
            seen.add((w["all_skipped"], c["slice_type"]))
    assert seen == {(0, 0), (1, 0), (0, 2)}


def splice_slices(hook):
    firsts = set()
    for g in (WIDE, TALL, MID, SMALL):
        for c in slice_cases(g):
            w = check_splice(hook, c)
            assert w["all_skipped"] == 0 or len(c["slice_row"]) == 2
            firsts |= {r * g[0] for r in c["slice_row"][:-1]}
        for c in random_cases(g, 12):
            check_splice(hook, c)
    assert firsts >= {0, 480, 960, 1440}


SPLICE_GROUPS = [("alignment, rem 0", lambda h: splice_alignment(h, 0)), ("alignment, rem 1", lambda h: splice_alignment(h, 1)),
                 ("alignment, rem 31", lambda h: splice_alignment(h, 31)), ("tails and capacity", splice_tails_and_capacity),
                 ("runs", splice_runs), ("slices", splice_slices)]


def test_splice_cases_contain_what_they_are_for():
    """the generators against the list of edges they exist for (no hook involved)"""
    pos = set()
    for c in alignment_cases(MID, (0, 1, 63, 64, 65, 129), (0, 1, 31)):
        nmbx = c["geom"][0]
        lead, _, bits = M.row_wave(0, c["mbs"][:nmbx])
        pos.add(((8 + 1 + c["hdr"].n + M.ue(lead).n) % 32, bits.n >> 5, bits.n & 31))
        carries = {M.row_wave(0, c["mbs"][r * nmbx: (r + 1) * nmbx])[2].n & 31 for r in range(c["geom"][1])}
    assert pos == {(p, f, r) for p in range(32) for f in (0, 1, 63, 64, 65, 129) for r in (0, 1, 31)}
    assert len(carries) > 1
    stops = {(M.slice_bits(0, c["hdr_nal"], 0, c["hdr"], c["mbs"])[0].n % 32, c["mbs"][-1][0]) for c in tail_cases(MID)}
    assert stops >= {(31, 0), (31, 1), (0, 0), (0, 1), (7, 0), (7, 1), (8, 0)}
    # runs as the serial writer meets them, on the widest pool: every value of the list, made from trail + skipped rows + lead
    got = set()
    for c in run_cases(WIDE):
        run, rows = 0, 0
        for s, _ in c["mbs"]:
            run = run + 1 if s else (got.add(run), 0)[1]
        got.add(run)
        rows = sum(M.row_wave(0, c["mbs"][r * 480: (r + 1) * 480])[0] == 480 for r in range(4))
        if len([1 for s, _ in c["mbs"] if not s]) == 2 and rows:
            got.add("chain")
    assert got >= set(RUNS) | {"chain", 1920}
    assert {c["short_words"] for c in capacity_cases(MID)} == {0, 1, 2, 40}
    assert any(len(c["slice_row"]) == 17 for c in slice_cases(TALL)) and {len(c["slice_row"]) - 1 for c in slice_cases(WIDE)} >= {1, 2, 3, 4}
    assert any(c["arena_reset"] == 0 and c["cursor"] % 16 for c in slice_cases(MID))


@pytest.mark.parametrize("name,group", SPLICE_GROUPS, ids=[g[0] for g in SPLICE_GROUPS])
def test_emulated_splice_matches_serial_writer(emu, name, group):
    group(emu)


@pytest.mark.gpu
@pytest.mark.parametrize("name,group", SPLICE_GROUPS, ids=[g[0] for g in SPLICE_GROUPS])
def test_gpu_splice_matches_serial_writer(gpu, name, group):
    group(gpu)


# ------------------------------------------------------------------ walk: cases

Z = ((0, 0), (0, 0))
S1 = ((1, 0), (33, -2))
WALK_POOLS = [(1, 5), (4, 4), (63, 3), (64, 3), (65, 3), (130, 3)]
BIG = (2048, -1024)


def _quiet(nmb, used_cand=1):
    """small vectors: from the zero state nothing moves"""
    return [((i % 7 - 3, i % 5 - 2), i % 5, used_cand) for i in range(nmb)]


def walk_cases(geom):
    """(name, records, slice rows, start state, consumed candidates, per-macroblock?)"""
    nmbx, nmby = geom
    nmb = nmbx * nmby
    rng = random.Random(7000 + nmbx)
    one = [0, nmby]
    rmv = lambda: (rng.randint(-2048, 2048), rng.randint(-2048, 2048))
    yield "nothing moves", _quiet(nmb), one, Z, Z, 0
    yield "everything moves", [(rmv(), 0, 0) for _ in range(nmb)], one, Z, Z, 0
    yield "everything moves, consumers", [(rmv(), i % 3, 1) for i in range(nmb)], one, S1, S1, 0
    for k in sorted({0, 63, 64, 127, 128, nmbx - 1, nmbx, nmbx + 63, nmbx + 64, 2 * nmbx, nmb - 1}):
        if k < nmb:
            # a lone mover; its own check sees the state in front of it, so nothing mismatches while nobody behind it consumes
            rec = _quiet(nmb, 0)
            rec[k] = (BIG, 0, 1)
            yield "lone mover at %d" % k, rec, one, Z, Z, 0
            # ... and the first consumer behind it, wherever in the batch / row it sits, does
            for d in (1, 20, 64):
                if k + d < nmb:
                    rec = _quiet(nmb, 0)
                    rec[k] = (BIG, 0, 1)
                    rec[k + d] = (rec[k + d][0], 0, 1)
                    if k + d + 1 < nmb:
                        rec[k + d + 1] = (rmv(), 0, 1)          # a second mismatch and mover behind the first: only the first is reported
                    yield "mover at %d, consumer at %d" % (k, k + d), rec, one, Z, Z, 0
    u = ((0, 1), (32, -3))
    assert u != S1 and all(M.rnd(a) == M.rnd(b) for a, b in zip(u, S1))
    yield "candidates differ but round alike", [((0, 0), 5, 1)] * nmb, one, S1, u, 0
    yield "differing candidates nobody consumed", _quiet(nmb, 0), one, Z, ((8, 8), (40, 40)), 0
    rec = [(BIG, 5 + i % 3, 1) for i in range(nmb)]
    yield "intra: checked, no update", rec, one, Z, Z, 0
    yield "intra: checked, mismatch", rec, one, Z, ((0, 0), (4, 0)), 0
    rnd_rec = [(rmv() if rng.random() < 0.1 else (rng.randint(-9, 9), rng.randint(-9, 9)), rng.randint(-1, 7), rng.randint(0, 1)) for _ in range(nmb)]
    yield "random, frame pair", rnd_rec, one, S1, S1, 0
    # a per-macroblock trajectory: the exact one (no mismatch), and with one entry off
    exact = M.walk(rnd_rec, nmbx, one, S1, S1, 0)[2]
    yield "exact trajectory", [(mv, t, 1) for mv, t, _ in rnd_rec], one, S1, exact, 1
    off = list(exact)
    k = nmb * 2 // 3
    off[k] = (off[k][0], (off[k][1][0] + 4, off[k][1][1]))
    yield "trajectory off at %d" % k, [(mv, t, 1) for mv, t, _ in rnd_rec], one, S1, off, 1
    for ns in (2, 3):
        for sr in {tuple(_even_split(nmby, ns)), tuple([0] + list(range(nmby - ns + 1, nmby)) + [nmby])}:
            yield "%d slices, movers" % ns, [(rmv(), 0, 0) for _ in range(nmb)], list(sr), S1, S1, 0
            yield "%d slices, random" % ns, rnd_rec, list(sr), S1, S1, 0
            ex = M.walk(rnd_rec, nmbx, list(sr), S1, S1, 0)[2]
            yield "%d slices, exact trajectory" % ns, [(mv, t, 1) for mv, t, _ in rnd_rec], list(sr), S1, ex, 1


def _groupings(nmby):
    """JobWalk::rows row by row, all rows at once, in uneven groups (and a call that has nothing new to walk)"""
    g = [list(range(nmby)), [nmby - 1], [0, nmby - 1]]
    if nmby >= 4:
        g.append([1, 1, 2, nmby - 1])
    return g


def check_walk(hook, geom, case):
    name, rec, sr, start, used, per_mb = case
    nmbx, nmby = geom
    nmb = nmbx * nmby
    want_fb, want_end, want_traj = M.walk(rec, nmbx, sr, start, used, per_mb)
    want_moved = 0 if per_mb else M.moved(rec, used)
    r = np.zeros(nmb, np.dtype([("mv", "<u4"), ("type", "i1"), ("used", "u1"), ("pad", "u1", 2)]))
    r["mv"], r["type"], r["used"] = [M.pack(x[0]) for x in rec], [x[1] for x in rec], [x[2] for x in rec]
    data = r.tobytes()
    pm = np.array([[M.pack(u[0]), M.pack(u[1])] for u in used], "<u4") if per_mb else None
    if per_mb:
        data += pm.tobytes()
    pair = Z if per_mb else used
    traj = np.array([[M.pack(t[0]), M.pack(t[1])] for t in want_traj], "<u4")
    want = (want_fb, M.pack(want_end[0]), M.pack(want_end[1]))
    for ups in _groupings(nmby):
        args = [0, per_mb, _i32(M.pack(start[0])), _i32(M.pack(start[1])), 0, len(sr) - 1, len(ups), _i32(M.pack(pair[0])), _i32(M.pack(pair[1])), 0]
        args += sr + [0] * (17 - len(sr)) + [0] * 5 + ups
        out = hook.run(geom, 2, args, data, HDR + 16 * nmb)
        h = np.frombuffer(out[:HDR], np.int32)
        t = np.frombuffer(out[HDR:], "<u4").reshape(2, nmb, 2)
        what = (name, geom, sr, ups)
        assert (int(h[0]), int(h[1]) & 0xffffffff, int(h[2]) & 0xffffffff) == want, ("JobWalk", what)
        assert (int(h[3]), int(h[4]) & 0xffffffff, int(h[5]) & 0xffffffff) == want, ("device_clusters_walk", what)
        assert (t[0] == traj).all(), ("JobWalk trajectory", what, np.argwhere(t[0] != traj)[:4])
        assert (t[1] == traj).all(), ("device_clusters_walk trajectory", what, np.argwhere(t[1] != traj)[:4])
        assert int(h[6]) == want_moved, ("moved", what)
    # the host's walk splits the rows evenly itself
    if sr == _even_split(nmby, len(sr) - 1):
        st = np.array([M.pack(start[0]), M.pack(start[1])], "<u4")
        uu = pm if per_mb else np.array([M.pack(used[0]), M.pack(used[1])], "<u4")
        ht = np.zeros((nmb, 2), "<u4")
        fb = hook.L.h264e_hip_selftest_host_clusters_walk(st.ctypes.data, r.ctypes.data, nmbx, nmby, len(sr) - 1, uu.ctypes.data, per_mb, ht.ctypes.data)
        assert (fb, int(st[0]), int(st[1])) == want and (ht == traj).all(), ("host clusters_walk", name, geom, sr)
    return want_fb, want_moved


def walk_pool(hook, geom):
    seen = {}
    for case in walk_cases(geom):
        seen[case[0]] = check_walk(hook, geom, case)
    nmb = geom[0] * geom[1]
    # the cases do what their names say
    assert seen["nothing moves"] == (-1, 0) and seen["everything moves"] == (-1, 1) and seen["everything moves, consumers"][0] == 1
    assert all(v == (-1, 1) for k, v in seen.items() if k.startswith("lone mover"))
    assert all(v[0] == int(k.split()[-1]) for k, v in seen.items() if k.startswith("mover at"))
    assert seen["candidates differ but round alike"][0] == -1 and seen["differing candidates nobody consumed"][0] == -1
    assert seen["intra: checked, no update"] == (-1, 0) and seen["intra: checked, mismatch"] == (0, 0)
    assert seen["exact trajectory"][0] == -1 and seen["trajectory off at %d" % (nmb * 2 // 3)][0] == nmb * 2 // 3
    assert seen["2 slices, exact trajectory"][0] == -1 and seen["3 slices, exact trajectory"][0] == -1


def step_cases():
    recs = [((r[0], r[1]), (r[2], r[3]), (r[4], r[5]), (r[6], r[7]), (r[8], r[9])) for r in FIX["steps"]]
    for q in FIX["sequences"]:
        st = q["steps"] + [q["end"] + [0, 0]]
        recs += [((a[0], a[1]), (a[2], a[3]), (a[4], a[5]), (b[0], b[1]), (b[2], b[3])) for a, b in zip(st, st[1:])]
    return recs


def check_steps(hook):
    recs = step_cases()
    data = np.array([[M.pack(c0), M.pack(c1), M.pack(mv)] for c0, c1, mv, _, _ in recs], "<u4").tobytes()
    out = np.frombuffer(hook.run(SMALL, 3, [len(recs)], data, 20 * len(recs)), "<u4").reshape(len(recs), 5)
    for (c0, c1, mv, o0, o1), got in zip(recs, out):
        assert [int(v) for v in got[:2]] == [M.pack(o0), M.pack(o1)], ("clusters_step", c0, c1, mv)
        assert [int(v) for v in got[2:]] == [M.pack(M.rnd(c0)), M.pack(M.rnd(c1)), M.pack(M.rnd(mv))], ("mvround", c0, c1, mv)
    # every component in -8..8, in x and in y, against the reference's rounding itself
    rd = np.array([[M.pack((v, -v)), 0, 0] for v, _, _ in FIX["round"]], "<u4").tobytes()
    out = np.frombuffer(hook.run(SMALL, 3, [17], rd, 20 * 17), "<u4").reshape(17, 5)
    assert [int(v) for v in out[:, 2]] == [M.pack((rx, ry)) for _, rx, ry in FIX["round"]]


def test_fixture_contains_what_it_is_for():
    assert [r[0] for r in FIX["round"]] == list(range(-8, 9))
    kinds, neg, ext = set(), 0, set()
    for r in FIX["steps"]:
        n, n0, n1 = r[4] ** 2 + r[5] ** 2, r[0] ** 2 + r[1] ** 2, r[2] ** 2 + r[3] ** 2
        kinds.add((n < n1, n >= n0))
        kinds.add("n == n0" if n == n0 and n0 else "n == n1" if n == n1 and n1 else None)
        neg += (n < n1 and 63 * r[0] + r[4] + 32 < 0) + (n >= n0 and 63 * r[3] + r[5] + 32 < 0)
        ext |= {v for v in r[:6] if abs(v) >= 2048}
    assert kinds >= {(True, True), (True, False), (False, True), (False, False), "n == n0", "n == n1"}
    assert neg >= 20 and ext >= {2048, -2048, 32767, -32768}
    assert [0, 0, 0, 0] in [r[:4] for r in FIX["steps"]] and all(len(q["steps"]) == 300 for q in FIX["sequences"]) and len(FIX["sequences"]) == 3
    assert os.path.getsize(os.path.join(HERE, "golden", "finalizer.json")) <= os.path.getsize(os.path.join(HERE, "golden", "stage_edges.json"))


def test_oracle_restatement_matches_reference_functions():
    L = oracle_lib.lib()
    L.h264o_test_clusters_update.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    L.h264o_test_mvround.argtypes = [C.c_int32]
    L.h264o_test_mvround.restype = C.c_int32
    for c0, c1, mv, o0, o1 in step_cases():
        c = (C.c_int32 * 2)(_i32(M.pack(c0)), _i32(M.pack(c1)))
        L.h264o_test_clusters_update(c, _i32(M.pack(mv)))
        assert [v & 0xffffffff for v in c] == [M.pack(o0), M.pack(o1)], (c0, c1, mv)
    for v, rx, ry in FIX["round"]:
        assert L.h264o_test_mvround(_i32(M.pack((v, -v)))) & 0xffffffff == M.pack((rx, ry))


def test_emulated_step_matches_reference_functions(emu):
    check_steps(emu)


@pytest.mark.parametrize("geom", WALK_POOLS, ids=["%dx%d" % g for g in WALK_POOLS])
def test_emulated_walks_match_model(emu, geom):
    walk_pool(emu, geom)


@pytest.mark.gpu
def test_gpu_step_matches_reference_functions(gpu):
    check_steps(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", WALK_POOLS, ids=["%dx%d" % g for g in WALK_POOLS])
def test_gpu_walks_match_model(gpu, geom):
    walk_pool(gpu, geom)
