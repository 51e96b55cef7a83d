"""CPU: the partition search's chain step (enc_mb.h diamond_g: the SAD cache as packed halfwords, the scan-order pick from a 4-bit mask,
the code lengths carried from centre to centre) in the lane-loop emulation, both lane orders.

  * the `diamond` cases of the stage fixtures (tests/golden/stages.json, stage_edges.json: recorded outputs of the reference's own
    me_search_diamond) through stage hook 8, all four partition geometries: vector, cost, prediction;
  * the small streams of tests/scan_step_cases.py against the oracle library: bytes, frame sizes, per-macroblock decision trace;
  * the full-sample cases of tests/scan_step_cases.py (stage hook 8 without the sub-sample stage) against the restatement of the
    reference's loop there -- the only place a cached cost reaches 0x10000 (see the note in scan_step_cases.py: no stream at QP 10 or
    QP 51 can), with eight cases in which the truncation decides the result.

What the searches met is counted by an emulation library built with counters (tests/emu/scan_counters.h through scan_counters.mk, read
under H264E_TEST_KNOBS=1; the product and the plain emulation libraries have none) and the minima are asserted.
Counts found (emulation, forward lane order):
  26 streams:  42386 partition searches; 6999 with a chain of three or more moves that changed direction (the corner path); 580 restarts
               from the diagonal probe; searches that met the x0 / x1 / y0 / y1 side of their range: 180 / 919 / 16 / 179;
               0 that cached a cost >= 0x10000
  88 full-sample stage cases (each from memory and from the window, the first ten in every lane group): 22 cache a cost >= 0x10000,
               8 of them end elsewhere with a full-width cache, 43 take the corner path."""
import ctypes as C
import os
import subprocess

import pytest

import pkg
import scan_step_cases as K
import test_stage_edges as E
import test_stages as S

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_LIB = os.path.join(HERE, "emu", "build", "libh264e_emu_scan.so")      # the forward lane order, with the counters
LIBS = [SCAN_LIB, pkg.EMU_REV_LIB]
LIB_IDS = ["forward", "reverse"]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu"), "-f", "scan_counters.mk"], stdout=subprocess.DEVNULL)


@pytest.fixture()
def counts(monkeypatch):
    """reader of the emulation's scan counters (reset on every read): [searches, truncated, corner path, restarts, x0, x1, y0, y1]"""
    monkeypatch.setenv("H264E_TEST_KNOBS", "1")
    f = pkg.load_pkg().load(SCAN_LIB).h264e_emu_scan_counts
    f.argtypes = [C.POINTER(C.c_longlong), C.c_int]

    def read():
        a = (C.c_longlong * 8)()
        f(a, 1)
        return list(a)

    read()
    return read


def diamond_fixture_cases(run):
    """hook 8 on the recorded `diamond` cases of both stage fixtures, from memory and from the window"""
    n = 0
    for window in (0, 1):
        for ci, c in enumerate(S.FIX["diamond"]):
            ref = S._b(S.FIX["diamond_refs"][c["ref"]]["pic"])
            args = [c["px"], c["py"], c["w"], c["h"]] + c["mv_in"] + c["mv_pred"] + [c["min_sad_in"], c["qp"], c["speed"]] + c["range"] + c["limit"] + [window, ci % 4]
            r = run(8, ref + S._b(c["cur"]), args, 16 + 256)
            cost, mx, my = S.np.frombuffer(r[:12], S.np.int32)
            assert (cost, [mx, my]) == (c["cost"], c["mv"]), ("stages.json", window, ci)
            got = S.np.frombuffer(r[16:272], S.np.uint8).reshape(16, 16)[c["py"]: c["py"] + c["h"], c["px"]: c["px"] + c["w"]]
            want = S.np.frombuffer(S._b(c["pred"]), S.np.uint8).reshape(16, 16)[: c["h"], : c["w"]]
            assert (got == want).all(), ("stages.json prediction", window, ci)
            n += 1
        ref = E._diamond_ref()
        for ci, c in enumerate(E.FIX["diamond"]):
            args = [c["px"], c["py"], c["w"], c["h"]] + c["mv_in"] + c["mv_pred"] + [c["min_sad_in"], c["qp"], c["speed"]] + c["range"] + c["limit"] + [window, ci % 4]
            r = run(8, ref + E._b(c["cur"]), args, 16 + 256)
            cost, mx, my = S.np.frombuffer(r[:12], S.np.int32)
            assert (cost, [mx, my]) == (c["cost"], c["mv"]), ("stage_edges.json", window, ci)
            assert E._rows(r[16 + 16 * c["py"] + c["px"]: 272] + bytes(256), 16, c["w"], c["h"]) == E._b(c["pred"]), ("stage_edges.json prediction", window, ci)
            n += 1
    return n


def test_fixtures_hold_all_four_partition_geometries():
    for fix in (S.FIX, E.FIX):
        assert {(c["w"], c["h"]) for c in fix["diamond"]} == {(16, 16), (16, 8), (8, 16), (8, 8)}


@pytest.mark.parametrize("lib", LIBS, ids=LIB_IDS)
def test_recorded_searches_of_the_reference(lib):
    run, close = S._hook(lib)
    try:
        assert diamond_fixture_cases(run) == 2 * (len(S.FIX["diamond"]) + len(E.FIX["diamond"]))
    finally:
        close()


@pytest.mark.parametrize("lib", LIBS, ids=LIB_IDS)
def test_full_sample_searches_where_the_truncation_shows(lib, counts):
    cases = K.stage_cases()
    assert sum(c[6]["trunc"] for c in cases) >= 8 and sum(c[6]["decisive"] for c in cases) >= 8 and sum(c[6]["corner"] for c in cases) >= 8
    run, close = S._hook(lib)
    try:
        K.check_stage_cases(run)
    finally:
        close()
    if lib == SCAN_LIB:
        got = counts()
        runs = 2 * (4 * 10 + len(cases) - 10)
        # every case ran `runs / len(cases)` times on average; the emulation must have seen what the restatement saw, per run
        assert got[0] == runs, got
        assert got[1] >= 2 * sum(c[6]["trunc"] for c in cases) >= 16, got
        assert got[2] >= 2 * sum(c[6]["corner"] for c in cases), got


def test_small_streams_against_the_oracle(counts):
    P = pkg.load_pkg()
    counts()
    for i in range(len(K.CASES)):
        out, sizes, recs = K.encode(P, SCAN_LIB, i)
        K.check("emulation", i, out, sizes, recs)
    searches, trunc, corner, restarts, x0, x1, y0, y1 = counts()
    print("scan counters over %d streams: %d searches, %d truncated, %d corner path, %d restarts, clipped x0 %d x1 %d y0 %d y1 %d"
          % (len(K.CASES), searches, trunc, corner, restarts, x0, x1, y0, y1))
    assert corner >= 8 and restarts >= 8 and min(x0, x1, y0, y1) >= 8, (corner, restarts, x0, x1, y0, y1)
    # (truncated costs: none in a stream at these QPs, for the reason given in scan_step_cases.py; asserted on the stage cases above)
    assert trunc == 0


@pytest.mark.parametrize("i", [0, 7, 9, 18, 25], ids=lambda i: K.CASE_IDS[i])
def test_small_streams_reverse_lane_order(i):
    out, sizes, recs = K.encode(pkg.load_pkg(), pkg.EMU_REV_LIB, i)
    K.check("emulation, reverse lane order", i, out, sizes, recs)
