"""CPU, model only: the definition of the lookahead's motion search (tests/lookahead_motion_model.py) against the properties it is
meant to have, and against the pass without search (tests/lookahead_model.py)."""
import numpy as np
import pytest

import clips
import lookahead_model as M
import lookahead_motion_model as ML

CIF = (352, 288)


@pytest.mark.parametrize("name", ["synth", "pan", "scene", "ramp", "noise", "still"])
def test_range_0_is_todays_pass_and_a_search_never_costs_more(name):
    w, h, n = 176, 144, 4
    c = clips.make(name, w, h, n)
    zero = M.costs(c, w, h)
    rec0, fields0 = ML.analyse(c, w, h, 0)
    assert all(np.array_equal(a, b) for a, b in zip(rec0, zero))
    assert all(not mv.any() for mv, _ in fields0)
    for R in (1, 3, 8):
        rec, fields = ML.analyse(c, w, h, R)
        assert np.array_equal(rec[0], zero[0]), "I(f) is not searched"
        assert (rec[1] <= zero[1]).all(), "(0, 0) is a candidate"
        assert rec[1][0] == zero[1][0] and not fields[0][0].any()
        assert all(np.abs(mv).max() <= R and (cost <= fields0[f][1]).all() for f, (mv, cost) in enumerate(fields))


def test_still_pictures_give_no_vector():
    w, h, n = 176, 144, 4
    c = clips.make("still", w, h, n)
    rec, fields = ML.analyse(c, w, h, 8)
    zero = M.costs(c, w, h)
    for f in (1, 2):                                            # A, A, A, B: frames 1 and 2 repeat the frame before them
        assert not fields[f][0].any() and not fields[f][1].any() and rec[1][f] == zero[1][f] == 0
    held = np.stack([c[0]] * 3)
    rec, fields = ML.analyse(held, w, h, 8)
    assert all(not mv.any() for mv, _ in fields) and all(np.array_equal(a, b) for a, b in zip(rec, M.costs(held, w, h)))


def test_pan_of_12_is_found():
    w, h = CIF
    rec, fields = ML.analyse(clips.pan(w, h, 3), w, h, 8)
    for mv, cost in fields[1:]:
        # (6, 0) is a candidate of every block but those of the last column, whose block would leave the covered area
        assert (mv[:, :-1] == (6, 0)).all() and not cost[:, :-1].any()
        assert (mv[:, -1, 0] <= 0).all()
    assert rec[1][1] == 14799, "what the uncovered column costs"


def test_vertical_pan_of_8_is_found():
    w, h = CIF
    _, fields = ML.analyse(clips.vpan(w, h, 3, 8, lambda t: True), w, h, 8)
    for mv, cost in fields[1:]:
        assert (mv[:-1] == (0, 4)).all() and not cost[:-1].any()


def test_pan_of_20_is_beyond_the_range():
    w, h = CIF
    near = ML.costs(clips.pan(w, h, 3), w, h, 8)
    rec, fields = ML.analyse(clips.pan(w, h, 3, step=20), w, h, 8)
    assert all((cost > 0).all() for _, cost in fields[1:]), "no block finds a zero: (10, 0) is no candidate"
    assert rec[1][1] > 10 * near[1][1]


def test_ties_go_to_the_first_in_the_order():
    flat = np.full((32, 48), 77, np.int64)
    inter, mv = ML.search(flat, flat, 8)
    assert not mv.any() and not inter.any()
    assert ML.ranked(1) == [(0, 0), (0, -1), (-1, 0), (1, 0), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)]
    # one bright sample inside block (1, 1), and two in the previous picture that each match it under another displacement: both
    # candidates cost the other sample, 100, every other candidate 300
    for (ax, ay), (bx, by), want in (((13, 12), (12, 13), (1, 0)), ((11, 12), (13, 12), (-1, 0)), ((12, 11), (11, 12), (0, -1))):
        cur, prev = np.zeros((32, 32), np.int64), np.zeros((32, 32), np.int64)
        cur[12, 12] = 100
        prev[ay, ax] = prev[by, bx] = 100
        inter, mv = ML.search(cur, prev, 8)
        assert inter[1, 1] == 100 and tuple(mv[1, 1]) == want
        assert not np.delete(mv.reshape(-1, 2), 5, axis=0).any(), "the flat blocks around it stay at (0, 0)"


def test_candidates_that_leave_the_covered_area_are_left_out():
    """a picture of 24 x 16 half-resolution samples covers 3 x 2 blocks; with 27 x 19 the remainder is not searched either"""
    rng = np.arange(19 * 27).reshape(19, 27)
    prev = (rng * 2654435761 >> 7) & 255
    cur = np.roll(prev, (-3, -2), axis=(0, 1))                  # content moves up 3 and left 2: the match lies at (+2, +3)
    inter, mv = ML.search(cur, prev, 8)
    assert tuple(mv[0, 0]) == (2, 3) and inter[0, 0] == 0
    assert (mv[1, :, 1] <= 0).all() and (mv[:, 2, 0] <= 0).all(), "the bottom row cannot look down, the right column not right"
    assert inter[1, 2] > 0
