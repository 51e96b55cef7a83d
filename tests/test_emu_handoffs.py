"""CPU: the wave hand-offs of the macroblock step in every arrival order (tests/handoff_cases.py) -- the product's inter_choose and
mb_intra_decide under the emulation's recording and scripted policies (tests/emu/emu_handoffs.h), both lane orders.  On the GPU the order
in which the search wave's bounds and decision reach the reconstruction wave is the clock's (tests/test_gpu_handoffs.py runs the same
cases there); here it is the schedule.  The helper wave's own loop (h264e_kernels.hip) stays GPU-only: the "+helper" schedules hand the
8x8 search over through a copy of its request record."""
import collections
import os
import subprocess

import pytest

import handoff_cases as K
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = [pkg.EMU_LIB, pkg.EMU_REV_LIB]
LIB_IDS = ["lanes_up", "lanes_down"]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("lib", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.CASE_IDS)
def test_every_arrival_order_gives_the_oracles_stream(i, lib):
    """under every schedule: bytes, frame sizes and every macroblock's type and mv[0] are the oracle's; every bound the search side
    published is an upper bound of the cost it ended with; and every decision is the one the macroblock's own costs give"""
    for schedule in K.ALL_SCHEDULES:
        out, sizes, recs, hand = K.scripted(lib, i, schedule)
        K.check_stream(schedule, i, out, sizes, recs)
        assert K.check_bounds(schedule, i, hand) > 0, "%s, %s: no macroblock published a bound" % (K.CASE_IDS[i], schedule)
        K.check_decisions(schedule, i, hand)


def test_the_schedules_are_what_the_reconstruction_side_saw():
    """the scripts reach mb_intra_decide: under arrive@K no macroblock has the decision before call K, under late / announced /
    tightened none ever has it before wait_ready, and the bounds handed out are the recorded ones, never earlier than scripted"""
    i = 0
    for schedule in K.SCHEDULES:
        _, _, _, hand = K.scripted(pkg.EMU_LIB, i, schedule)
        name, _, arg = schedule.partition("@")
        for t, k, r in K.records(hand):
            if r["inter_type"] < 0:
                assert r["calls"] == 0 and r["arrived_at"] == -1, "an early skip waits for nothing but the decision"
                continue
            where = "%s frame %d macroblock %d: %r" % (schedule, t, k, r)
            if name == "plain":
                assert (r["k_ready"], r["calls"], r["seen_min"]) == (-1, 0, K.NONE), where
            elif name in ("late", "announced", "tightened"):
                assert r["k_ready"] == K.NEVER and r["arrived_at"] == -1 and 1 <= r["calls"] <= 17, where
                want = {"late": (K.NEVER, K.NEVER), "announced": (0, K.NEVER), "tightened": (0, int(arg or 0))}[name]
                assert (r["j_u"], r["j_tight"]) == want, where
                if name == "late":
                    assert r["seen_min"] == K.NONE, where
                elif name == "announced" or r["calls"] <= int(arg):
                    assert r["seen_min"] == r["u"], where
                else:
                    assert r["seen_min"] == r["tight"], where
            elif name == "arrive":
                assert r["k_ready"] == int(arg) and r["arrived_at"] in (-1, int(arg)), where
                assert r["calls"] == int(arg) + 1 if r["arrived_at"] >= 0 else r["calls"] <= int(arg), where
            if r["j_u"] > r["j_tight"] and r["j_u"] != K.NEVER:
                pytest.fail("the tightened value in front of the announced one: " + where)


def test_the_cases_bite():
    """a condition, not a measurement: over the case list (lanes up, every schedule) there are enough macroblocks of every kind that
    makes a hand-off matter -- a clip that stops producing them has to be replaced, not the count lowered"""
    seen = collections.defaultdict(set)
    for i in range(len(K.CASES)):
        for schedule in K.ALL_SCHEDULES:
            for t, k, r in K.records(K.scripted(pkg.EMU_LIB, i, schedule)[3]):
                for kind in K.kinds(r):
                    seen[kind].add((i, t, k))
    counts = {kind: len(seen[kind]) for kind in sorted(K.KINDS)}
    short = ["%s (%s): %d macroblocks, %d needed" % (kind, K.KINDS[kind], counts[kind], K.NEEDED[kind]) for kind in sorted(K.KINDS) if counts[kind] < K.NEEDED[kind]]
    assert not short, "the case list is too weak; counts %s\n%s" % (counts, "\n".join(short))


def test_the_schedule_knob_is_the_emulations_and_needs_the_test_switch(monkeypatch):
    """without H264E_TEST_KNOBS=1 a stray H264E_EMU_HANDOFFS changes nothing and records nothing; an unknown schedule is refused"""
    P = pkg.load_pkg()
    monkeypatch.delenv("H264E_TEST_KNOBS", raising=False)
    out, sizes, recs, hand = K.encode(P, pkg.EMU_LIB, 0, dict(H264E_EMU_HANDOFFS="late"))
    K.check_stream("no switch", 0, out, sizes, recs)
    assert all(frame is None for frame in hand)
    with pytest.raises(P.H264EError, match="H264E_EMU_HANDOFFS"):
        K.encode(P, pkg.EMU_LIB, 0, dict(H264E_TEST_KNOBS="1", H264E_EMU_HANDOFFS="sooner"))
