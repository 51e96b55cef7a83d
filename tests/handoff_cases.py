"""The wave hand-offs of the macroblock step ("Two wavefronts per row"; h264e_kernels.hip SearchSignals / InterFromSearchWave,
enc_row.h mb_intra_decide) as cases for the emulation test (tests/test_emu_handoffs.py), where the arrival order is an input, and for the
GPU test (tests/test_gpu_handoffs.py), where it is whatever the clock produces.

With more than one wave per row the reconstruction wave decides the intra 4x4 candidates of a macroblock while the search wave is still at
work on it; intra4_choose gives up as soon as its growing cost reaches a bound, and that bound is the 16x16 intra cost alone, the bound
inter_choose announced (sig.bound(u)), the tighter one search_type writes behind the 16x16 partition, or the final inter cost -- depending
on how far the search wave has got.  The stream is the reference's only if (1) every published bound is an upper bound of the cost the
inter decision ends with and (2) the decision does not depend on which of them was seen.  The emulation's scripted policies
(tests/emu/emu_handoffs.h, H264E_EMU_HANDOFFS) show the reconstruction side a chosen part of what the search wave says, call by call of the
bound, and record what was said; the checks here hold the streams and decisions against the oracle and the two conditions against the
records.

The pictures are small (at most 6 x 3 macroblocks), 3 or 4 frames, one I frame in front: P frames with intra 4x4 on (speed 0 and 1) over
content where intra wins inside P frames (scene with its cut, noise, extremes) and where skips and long vectors meet (pan, synth), at
QP 10, 26, 40 and 51, once in two row-band slices and once under rate control; four more cases at other QPs hold the macroblocks where intra
4x4 wins by exactly one (kind f)."""
import contextlib
import functools
import os

import numpy as np

import clips
import oracle_lib

NONE = 0x7fffffff
NEVER = 99
FIELDS = ("flags", "u", "tight", "inter_type", "inter_cost", "min_gcost", "cost16", "cost4", "k_ready", "j_u", "j_tight", "calls", "arrived_at",
          "seen_min", "final_type", "final_cost")

# (content, width, height, frames, encoder arguments)
CASES = [
    ("scene", 64, 48, 4, dict(qp=26, speed=0)),
    ("scene", 96, 32, 4, dict(qp=40, speed=1)),
    ("scene", 50, 38, 4, dict(qp=10, speed=0)),
    ("noise", 48, 48, 3, dict(qp=40, speed=0)),
    ("noise", 50, 38, 3, dict(qp=51, speed=1)),
    ("noise", 64, 48, 3, dict(qp=26, speed=0, slices=2)),
    ("extremes", 48, 48, 3, dict(qp=51, speed=0)),
    ("extremes", 96, 32, 3, dict(qp=26, speed=1)),
    ("pan", 96, 32, 4, dict(qp=26, speed=0)),
    ("pan", 64, 48, 4, dict(qp=40, speed=1)),
    ("synth", 64, 48, 4, dict(qp=10, speed=1)),
    ("synth", 48, 48, 4, dict(qp=51, speed=0)),
    ("scene", 64, 48, 4, dict(speed=0, kbps=150)),
    # found by a search over QPs on the CPU: each has a macroblock whose intra 4x4 cost is ONE below its inter cost and below its 16x16
    # intra cost -- the only macroblocks that tell "cost >= bound" from "cost >= bound - 1" at the final inter cost (kind f below)
    ("scene", 50, 38, 4, dict(qp=44, speed=0)),
    ("scene", 96, 32, 4, dict(qp=28, speed=0)),
    ("synth", 48, 48, 4, dict(qp=11, speed=1)),
    ("synth", 48, 48, 4, dict(qp=16, speed=1)),
]
CASE_IDS = ["%s_%dx%d_%s" % (c[0], c[1], c[2], "-".join("%s%d" % (k, v) for k, v in sorted(c[4].items()))) for c in CASES]

SCHEDULES = (["plain", "late", "announced", "tightened@0", "tightened@3", "tightened@9"] + ["arrive@%d" % k for k in range(17)]
             + ["mixed:1", "mixed:2", "mixed:3"])
# ... and through the helper wave's request record (the three- and four-wave variants)
HELPER_SCHEDULES = ["plain+helper", "late+helper", "arrive@5+helper", "mixed:4+helper"]
ALL_SCHEDULES = SCHEDULES + HELPER_SCHEDULES

GOP = 30


@functools.lru_cache(maxsize=None)
def clip(i):
    name, w, h, n, _ = CASES[i]
    c = clips.make(name, w, h, n)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle(i):
    """(stream, frame sizes, per frame the trace [(type, mvx, mvy)]) of case i"""
    name, w, h, n, kw = CASES[i]
    want, sizes = oracle_lib.encode_clip(clip(i), w, h, gop=GOP, **kw)
    o = oracle_lib.Encoder(w, h, gop=GOP, **kw)
    parts, traces = [], []
    for t in range(n):
        parts.append(o.encode(clip(i)[t]))
        traces.append([(typ, mvx, mvy) for typ, _, mvx, mvy, _ in o.trace()])
    o.close()
    assert b"".join(parts) == want, "the oracle's two entry points disagree"
    return want, sizes, traces


@contextlib.contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def encode(P, lib, i, env):
    """case i through the clip encoder of `lib` (None = the product library on the GPU) with `env` set while its pool exists:
    (stream, frame sizes, per frame the macroblock records, per frame the hand-off records or None)"""
    import ctypes as C
    name, w, h, n, kw = CASES[i]
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    with environment(**env):
        ce = P.ClipEncoder(w, h, n, gop=GOP, lib=lib, keep_records=1, **kw)
        try:
            ce.upload(clip(i))
            out, sizes, st = ce.encode()
            assert st.spin_relaunches == 0
            recs = [ce.read_records(t) for t in range(n)]
            hand = None
            if "H264E_EMU_HANDOFFS" in env:
                f = ce.L.h264e_emu_handoff_records
                f.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_int]
                hand = []
                for t in range(n):
                    buf = np.zeros((nmb, len(FIELDS)), np.int32)
                    got = f(t, w * h * 3 // 2, buf.ctypes.data, nmb)
                    assert got in (0, nmb), "frame %d: %d hand-off records for %d macroblocks" % (t, got, nmb)
                    hand.append([dict(zip(FIELDS, map(int, row))) for row in buf] if got else None)
        finally:
            ce.close()
    return out, sizes, recs, hand


@functools.lru_cache(maxsize=None)
def scripted(lib, i, schedule):
    """case i through the emulation `lib` under `schedule`"""
    import pkg
    return encode(pkg.load_pkg(), lib, i, dict(H264E_TEST_KNOBS="1", H264E_EMU_HANDOFFS=schedule))


def check_stream(what, i, out, sizes, recs):
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


def records(hand):
    """(frame, macroblock, record) of every macroblock that left one"""
    for t, frame in enumerate(hand):
        for k, r in enumerate(frame or ()):
            if r["flags"] & 1:
                yield t, k, r


def check_bounds(what, i, hand):
    """condition (1) from the recorder: where bound(u) was called -- never for an early skip -- u and the tightened value are upper
    bounds of the cost inter_choose ended with, and the tightened one is the tighter"""
    n = 0
    for t, k, r in records(hand):
        where = "%s, %s: frame %d macroblock %d" % (CASE_IDS[i], what, t, k)
        early_skip = r["inter_type"] < 0
        assert bool(r["flags"] & 2) == (not early_skip), "%s: noskip() and the early skip disagree (type %d)" % (where, r["inter_type"])
        assert bool(r["flags"] & 4) == (not early_skip), "%s: bound() and the early skip disagree (type %d)" % (where, r["inter_type"])
        if early_skip:
            continue
        assert r["u"] >= r["inter_cost"], "%s: announced bound %d below the inter cost %d" % (where, r["u"], r["inter_cost"])
        assert r["tight"] >= r["inter_cost"], "%s: tightened bound %d below the inter cost %d" % (where, r["tight"], r["inter_cost"])
        assert r["tight"] <= r["u"], "%s: tightened bound %d above the announced one %d" % (where, r["tight"], r["u"])
        n += 1
    return n


def check_decisions(what, i, hand):
    """condition (2) from the recorder: the decision is the one the macroblock's own three costs give (h264-lab.h:5748-5762: 16x16 intra
    against the inter cost, then 4x4 intra against the better, both with a strict "<") -- whichever bound the scripted run saw"""
    for t, k, r in records(hand):
        if r["inter_type"] < 0:
            want = (-1, 0)
        else:
            want = (r["inter_type"], r["inter_cost"])
            if r["cost16"] < want[1]:
                want = (6, r["cost16"])
            if r["cost4"] < want[1]:
                want = (5, r["cost4"])
        got = (r["final_type"], r["final_cost"])
        assert got == want, ("%s, %s: frame %d macroblock %d: decided (type, cost) %s, its costs say %s (inter %d, intra16 %d, intra4 %d; script %d/%d/%d)"
                             % (CASE_IDS[i], what, t, k, got, want, r["inter_cost"], r["cost16"], r["cost4"], r["k_ready"], r["j_u"], r["j_tight"]))


KINDS = {
    "a": "intra4_choose gave up under an early bound (below the 16x16 intra cost) before the inter decision was there",
    "b": "intra4_choose ran to its last block with no bound but the 16x16 intra cost, and lost only in intra_merge",
    "c": "intra 4x4 won in a P frame",
    "d": "the inter decision arrived while the 4x4 blocks were being decided (behind block 1..15)",
    "e": "the inter decision ended with the skip vector's cost, not with the best partition type's",
    "f": "intra 4x4 won by one against an inter cost that arrived while its blocks were being decided",
    "h": "the 8x8 partition type was searched from the request record",
}
# how many macroblocks of every kind the case list has to hold at least.  f: exact coincidences -- the clips were searched for them, and each
# of the four cases added for it holds one
NEEDED = {"a": 20, "b": 20, "c": 20, "d": 20, "e": 20, "f": 4, "h": 20}


def kinds(r):
    """the kinds of KINDS this macroblock's record is one of"""
    out = set()
    if r["inter_type"] < 0:
        return out
    if r["flags"] & 8:
        out.add("h")
    if r["final_type"] == 5:
        out.add("c")
    if 1 <= r["arrived_at"] <= 15:
        out.add("d")
    if r["inter_cost"] != r["min_gcost"]:
        out.add("e")
    if r["cost4"] == r["inter_cost"] - 1 and r["cost4"] < r["cost16"] and r["arrived_at"] >= 0:
        out.add("f")
    if r["cost4"] == NONE:
        return out
    never = r["k_ready"] == NEVER
    # the bound at the last call in front of wait_ready: what intra4_choose's cost was held against
    if never and r["seen_min"] < r["cost16"] and (r["calls"] < 17 or r["cost4"] >= r["seen_min"]):
        out.add("a")
    if never and r["j_u"] == NEVER and r["calls"] == 17 and r["cost4"] < r["cost16"] and r["final_type"] != 5:
        out.add("b")
    return out
