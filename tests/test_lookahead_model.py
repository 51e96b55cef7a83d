"""CPU: properties of the numpy model of the lookahead rate control (tests/lookahead_model.py), which the product is tested against."""
import numpy as np

import clips
import lookahead_model as M


def test_lowres_is_the_rounded_2x2_mean():
    y = np.array([[0, 1, 255, 255, 9], [2, 3, 255, 254, 9], [7, 7, 7, 7, 9]], np.uint8)
    assert M.lowres(y).tolist() == [[2, 255]]          # (6 + 2) >> 2 = 2, (1019 + 2) >> 2 = 255; odd row and column dropped


def test_still_clip_has_no_inter_cost():
    w, h, n = 64, 48, 4
    c = clips.make("still", w, h, n)
    c[:] = c[0]
    i, p, nb = M.costs(c, w, h)
    assert i[0] > 0 and p[0] == i[0], "frame 0: inter = intra"
    assert not p[1:].any() and not nb[1:].any()
    assert (i == i[0]).all()


def test_constant_picture_has_no_intra_cost():
    w, h = 50, 38
    c = np.full((3, w * h * 3 // 2), 77, np.uint8)
    i, p, nb = M.costs(c, w, h)
    assert not i.any() and not p.any() and not nb.any()


def test_only_whole_blocks_count():
    """18x18: L is 9x9, one block; the ninth row and column change nothing"""
    w, h = 18, 18
    c = clips.make("noise", w, h, 2)
    d = c.copy()
    y = d[:, : w * h].reshape(2, h, w)
    y[:, 16:, :] ^= 0x55
    y[:, :, 16:] ^= 0x55
    assert [a.tolist() for a in M.costs(c, w, h)] == [a.tolist() for a in M.costs(d, w, h)]


def _setup(n=24, w=176, h=144, gop=8):
    c = clips.make("synth", w, h, n)
    cost = M.costs(c, w, h)
    kinds = [int(f % gop == 0) for f in range(n)]
    return cost, kinds, (40, 40 + 8 * 20)


def test_a_larger_budget_never_raises_a_qp():
    """fixed k and costs: no frame has been coded, so every window is planned from K0 and no carry -- only the first window of each plan
    is free of the others' sizes, so each window is planned as a clip's first"""
    cost, kinds, hdr = _setup()
    n, W = len(kinds), 4
    prev = None
    for kbps in (20, 50, 100, 200, 400, 800, 1600, 5000):
        qp = []
        for a in range(0, n, W):
            sub = tuple(x[a:a + W] for x in cost)
            qp.append(int(M.plan(sub, kinds[a:a + W], hdr, [0] * W, kbps, W)[0]))
        if prev is not None:
            assert all(q <= p for q, p in zip(qp, prev)), (kbps, qp, prev)
        prev = qp
    assert max(prev) < 50, "the largest budget is not starved"


def test_qp_stays_inside_the_range_and_is_one_per_window():
    cost, kinds, hdr = _setup()
    n = len(kinds)
    rng = np.random.RandomState(3)
    for kbps, W, lo, hi in [(1, 4, 10, 50), (100000, 4, 10, 50), (100, 5, 24, 30), (100, 32, 51, 51), (60, 7, 10, 51)]:
        actual = rng.randint(0, 60000, n)
        qp = M.plan(cost, kinds, hdr, actual, kbps, W, lo, hi)
        assert qp.min() >= lo and qp.max() <= hi
        for a in range(0, n, W):
            assert len(set(qp[a:a + W].tolist())) == 1
    assert M.plan(cost, kinds, hdr, [10 ** 7] * n, 1, 4).tolist() == [50] * n          # nothing fits, and the windows overshoot: qp_max
    assert M.plan(cost, kinds, hdr, [0] * n, 100000, 4).tolist() == [10] * n           # everything fits: qp_min


def test_carry_is_clamped_to_half_a_window():
    cost, kinds, hdr = _setup()
    n, W, kbps = len(kinds), 4, 120
    T = 8 * (kbps * 1000 // 8 // 30) * W
    for actual in ([0] * n, [10 ** 7] * n):
        trace = []
        M.plan(cost, kinds, hdr, actual, kbps, W, trace=trace)
        assert trace[0][1] == 0
        assert all(abs(carry) <= T // 2 and Tj == T + carry for Tj, carry, _k in trace)
        assert abs(trace[-1][1]) == T // 2
    # the factors move by at most 4x per window and never reach 0
    trace = []
    M.plan(cost, kinds, hdr, [0] * n, kbps, W, trace=trace)
    for (_, _, k0), (_, _, k1) in zip(trace, trace[1:]):
        assert all(b >= max(1, a // 4) and b <= 4 * a for a, b in zip(k0, k1))
