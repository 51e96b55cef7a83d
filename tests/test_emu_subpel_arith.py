"""CPU: the sub-sample stage of the partition search on sample pairs (enc_kernels.h halfpel3_rows, wave.h pk16) and the packed byte
average (wave.h avg4_u8) in the lane-loop emulation, both lane orders, against the model of tests/subpel_cases.py.

  * the model first: it must reproduce every recorded search of the stage fixtures (the reference's own me_search_diamond);
  * the case list must reach what packed arithmetic can break on -- asserted here with the model, so that a pass cannot hide a gap:
    both first stages at 10710 and -2550, a second-stage pair sum at 21420 and -5100, the second stage's result below 0 and above 255
    before its clamp, every probe and "none" as the winner, both sides of the 2x2 cell in x and in y, the first probe direction
    vertical and horizontal, all four partition geometries (through the LDS window a lane of a 16x16 partition filters four consecutive
    rows that share their window rows, of 16x8 and 8x16 two; an 8x8 partition has one row per lane: nothing to share);
  * the cases through stage hook 8; every pair of bytes through stage hook 16."""
import os
import subprocess

import pytest

import pkg
import subpel_cases as K
import test_stages as S

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = [pkg.EMU_LIB, pkg.EMU_REV_LIB]
LIB_IDS = ["forward", "reverse"]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def test_model_reproduces_the_recorded_searches():
    n, ran = K.model_reproduces_fixtures()
    assert n == len(S.FIX["diamond"]) + len(K.E.FIX["diamond"]) and ran >= 8, (n, ran)


def test_case_list_reaches_the_extremes():
    c = K.coverage()
    print("sub-sample cases: %d; first stage horizontal %s vertical %s, second-stage pair sums %s, result before the clamp %s, winners %s"
          % (len(K.cases()), c["h1"], c["v1"], c["pair"], c["centre"], sorted(str(w) for w in c["winners"])))
    assert c["h1"] == (-2550, 10710) and c["v1"] == (-2550, 10710), c
    assert c["pair"] == (-5100, 21420), c
    assert c["centre"][0] < 0 and c["centre"][1] > 255, c
    assert c["winners"] == set(K.PROBES) | {None}, c
    assert c["hp_ox"] == {0, 1} and c["hp_oy"] == {0, 1} and c["pq_vertical"] == {0, 1}, c
    assert c["geometries"] == {(16, 16), (16, 8), (8, 16), (8, 8)}, c
    # every case's footprint lies inside the hook's window: with window = 1 all of them take halfpel3_rows (rows shared between a lane's
    # consecutive passes at 16x16, 16x8 and 8x16), with window = 0 all of them take interp_luma4
    assert c["in_window"] == c["geometries"] and c["out_of_window"] == 0, c


@pytest.mark.parametrize("lib", LIBS, ids=LIB_IDS)
def test_sub_sample_cases(lib):
    run, close = S._hook(lib)
    try:
        assert K.check_cases(run) == 2 * (len(K.cases()) + 3 * 8)
    finally:
        close()


@pytest.mark.parametrize("lib", LIBS, ids=LIB_IDS)
def test_avg4_every_pair_of_bytes(lib):
    run, close = S._hook(lib)
    try:
        K.avg4_all_pairs(run)
    finally:
        close()
