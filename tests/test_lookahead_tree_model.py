"""CPU: properties of the numpy model of the lookahead's cost tree (tests/lookahead_tree_model.py) -- the yardstick of the emulation and
GPU tests -- that follow from the definition alone, and that the test shapes take the paths they are for."""
import numpy as np
import pytest

import clips
import lookahead_model as M
import lookahead_motion_model as ML
import lookahead_tree_model as MT
from test_emu_lookahead_tree import IDS, SHAPES, analysed


def test_noise_inherits_nothing():
    """a block of noise against the co-located block of other noise: inter >= intra, nothing is passed on and S = 0 -- the one-block
    shape, whose only candidate is (0, 0).  With 289 candidates per block a few blocks of a larger picture find a displacement that beats
    their own mean by a little: S stays below I/8, where the largest strength still rounds to offset 0, and the plan is the flat one"""
    w, h, clip, n, R = SHAPES[0]
    _, rec, fields, intra = analysed(w, h, clip, n, R)
    maps, S, d = MT.windows(rec, fields, intra, [1] + [0] * (n - 1), 3, 16, 2)
    assert not S.any() and not d.any() and all(not m.any() for m in maps)
    w, h, n = 176, 144, 6
    c = clips.make("noise", w, h, n)
    rec, fields, intra = MT.analyse(c, w, h, 8)
    maps, S, d = MT.windows(rec, fields, intra, [1] + [0] * (n - 1), 3, 16, 3)
    assert (8 * S.astype(np.int64) < rec[0].astype(np.int64)).all() and not d.any()


def test_a_still_clip_hands_every_frames_cost_to_the_first():
    """one picture n times: inter = 0 and mv = (0, 0) everywhere, so amt = i + g and all of it lands on the same block with weight 64:
    nothing is floored away, and S(a) is the sum of I over the frames behind a"""
    w, h, n = 176, 144, 6
    c = np.repeat(clips.make("synth", w, h, 1), n, axis=0)
    rec, fields, intra = MT.analyse(c, w, h, 8)
    maps, sums, amts = MT.run(intra, fields, [1] + [0] * (n - 1), 0, n)
    I = int(rec[0][0])
    assert [sums[f] for f in range(n)] == [(n - 1 - f) * I for f in range(n)]
    assert np.array_equal(maps[0], (n - 1) * intra[0])
    assert MT.delta(I, sums[0], 4) == -((4 * MT.log2_256(I, sums[0]) + 512) >> 10) == -3 and MT.log2_256(I, 5 * I) == 2 * 256 + 128


def test_a_key_frame_passes_nothing_back_and_receives():
    w, h, clip, n, R = SHAPES[3]
    _, rec, fields, intra = analysed(w, h, clip, n, R)
    kinds = [1, 0, 0, 1, 0, 0]
    maps, sums, amts = MT.run(intra, fields, kinds, 0, n)
    assert sums[3] > 0 and sums[2] == 0 and 3 not in amts, "frame 3 received from 4 and 5 and gave nothing to 2"
    assert sums[0] > 0 and sums[5] == 0
    open_maps, open_sums, _ = MT.run(intra, fields, [1, 0, 0, 0, 0, 0], 0, n)
    assert open_sums[2] > 0 and open_sums[3] == sums[3] and open_sums[0] > sums[0]


@pytest.mark.parametrize("w,h,clip,n,R", SHAPES, ids=IDS)
def test_nothing_is_created_on_the_way(w, h, clip, n, R):
    """the four weights of a block sum to 64 and every contribution is floored: in_{f-1} gets at most what frame f passes on"""
    _, rec, fields, intra = analysed(w, h, clip, n, R)
    kinds = [1] + [0] * (n - 1)
    maps, sums, amts = MT.run(intra, fields, kinds, 0, n)
    for f in range(1, n):
        got = int(maps[f - 1].sum())
        assert got <= amts[f] and amts[f] - got <= 3 * intra[f].size, (f, got, amts[f])
        assert amts[f] <= int(rec[0][f]) + sums[f]


@pytest.mark.parametrize("w,h,clip,n,R", SHAPES[1:], ids=IDS[1:])
def test_the_shapes_take_the_paths_they_are_for(w, h, clip, n, R):
    """blocks with four targets, with two and with one, in every shape with more than one block"""
    _, _, fields, _ = analysed(w, h, clip, n, R)
    ox = np.concatenate([(f[0][:, :, 0] & 7).ravel() for f in fields[1:]]) != 0
    oy = np.concatenate([(f[0][:, :, 1] & 7).ravel() for f in fields[1:]]) != 0
    assert (ox & oy).any() and (ox ^ oy).any() and (~ox & ~oy).any()


def test_one_block_reaches_nothing():
    _, _, fields, _ = analysed(*SHAPES[0])
    assert all(not f[0].any() for f in fields)


def test_scatter_weights():
    """one block of amount 1000 displaced by (3, -2) from block (1, 1) of a 3 x 3 grid: x = 11, y = 6"""
    amt = np.zeros((3, 3), np.int64)
    mv = np.zeros((3, 3, 2), np.int8)
    amt[1, 1], mv[1, 1] = 1000, (3, -2)
    out = MT.scatter(amt, mv)
    want = np.zeros((3, 3), np.int64)
    want[0, 1], want[0, 2], want[1, 1], want[1, 2] = (1000 * 5 * 2) >> 6, (1000 * 3 * 2) >> 6, (1000 * 5 * 6) >> 6, (1000 * 3 * 6) >> 6
    assert np.array_equal(out, want)
    assert MT.amounts(np.array([[0, 100, 100]]), np.array([[0, 25, 200]]), np.array([[7, 50, 1 << 41]])).tolist() == [[7, 112, 0]]
    assert MT.amounts(np.array([[100]]), np.array([[0]]), np.array([[1 << 41]])).tolist() == [[100 + (1 << 40)]]


def test_offsets():
    assert MT.log2_256(0, 5) == 0 and MT.log2_256(7, 0) == 0 and MT.log2_256(100, 100) == 256 and MT.log2_256(100, 200) == 256 + 128
    assert MT.log2_256(1, MT.SUM_MAX) == 48 * 256
    assert [MT.delta(100, s, 4) for s in (0, 100, 300, 700, 10 ** 9)] == [0, -1, -2, -3, -6]
    assert MT.delta(100, 100, 1) == 0 and MT.delta(100, 100, 2) == -1 and MT.delta(100, 100, 16) == -4


def test_plan_without_offsets_is_the_plan_of_the_searched_costs():
    n, Wc, kbps = 24, 4, 120
    rng = np.random.default_rng(5)
    cost = (rng.integers(40000, 60000, n).astype(np.uint64), rng.integers(2000, 30000, n).astype(np.uint64), np.zeros(n, np.int32))
    kinds = [int(f % 8 == 0) for f in range(n)]
    bits = rng.integers(1000, 9000, n)
    for search in (8, 0):
        qp, base = MT.plan(cost, kinds, (40, 200), bits, kbps, Wc, np.zeros(n, np.int8), search=search)
        assert np.array_equal(qp, ML.plan(cost, kinds, (40, 200), bits, kbps, Wc, search=search)) and np.array_equal(qp, base)
    d = np.where(np.arange(n) % 8 == 0, -3, 0).astype(np.int8)
    qp, base = MT.plan(cost, kinds, (40, 200), bits, kbps, Wc, d)
    assert np.array_equal(qp, np.clip(base.astype(int) + d, 10, 50)) and (qp != base).any()
    assert all(abs(int(base[a]) - int(base[a - Wc])) <= M.QP_STEP for a in range(Wc, n, Wc)) and all(len(set(base[a:a + Wc])) == 1 for a in range(0, n, Wc))
