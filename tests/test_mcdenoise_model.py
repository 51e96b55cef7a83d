"""CPU, model only: the motion-compensated temporal denoiser's definition (tests/mcdenoise_model.py) on hand-made cases, against the plain
denoiser's model where the two must agree, and what it is for: less error than the plain denoiser on noisy moving content."""
import numpy as np

import clips
import denoise_model as DM
import mcdenoise_model as M


def _planes(w, h, salt):
    return clips.noise(w, h, 1, salt)[0][: w * h].reshape(h, w)


def _brute(cur, prev, mv, mode):
    """luma vectors block by block, candidate by candidate, straight from the definition"""
    nby, nbx = mv.shape[:2]
    v, sad = np.zeros((nby, nbx, 2), np.int64), np.zeros((nby, nbx), np.int64)
    for by in range(nby):
        for bx in range(nbx):
            dx, dy = int(mv[by, bx, 0]), int(mv[by, bx, 1])
            best = None
            for c in (M.candidates(dx, dy) if mode == 2 else [(2 * dx, 2 * dy)]):
                s = M.block_sad(cur, prev, 16 * bx, 16 * by, 16, c)
                if s is not None and (best is None or s < best[0]):
                    best = (s, c)
            sad[by, bx], v[by, bx] = best
    return v, sad


def test_candidate_order():
    assert M.candidates(3, -2) == [(0, 0), (6, -4), (6, -5), (5, -4), (7, -4), (6, -3), (5, -5), (7, -5), (5, -3), (7, -3)]


def test_a_refinement_outside_the_plane_is_left_out():
    """32x32, block (1, 1) with the field (0, 0): prev is cur displaced so that (1, 1) would match exactly, but the block displaced by
    (1, 1) leaves the plane: the best candidate inside wins instead"""
    w = h = 32
    prev = _planes(w, h, 11)
    cur = np.zeros_like(prev)
    cur[:-1, :-1] = prev[1:, 1:]                        # cur(x, y) = prev(x + 1, y + 1)
    mv = np.zeros((2, 2, 2), np.int8)
    v, sad = M.luma_vectors(cur, prev, mv, 2)
    assert tuple(v[0, 0]) == (1, 1) and sad[0, 0] == 0, "inside: the exact match"
    assert tuple(v[1, 1]) != (1, 1) and sad[1, 1] > 0
    assert all(16 + v[1, 1][k] + 16 <= 32 for k in (0, 1))
    bv, bs = _brute(cur, prev, mv, 2)
    assert np.array_equal(v, bv) and np.array_equal(sad, bs)
    # mode 1 takes the field's vector as it stands
    v1, s1 = M.luma_vectors(cur, prev, mv, 1)
    assert not v1.any() and np.array_equal(s1, _brute(cur, prev, mv, 1)[1])


def test_ties_go_to_zero():
    w = h = 32
    flat = np.full((h, w), 90, np.uint8)
    mv = np.zeros((2, 2, 2), np.int8)
    mv[0, 0] = (1, 0)
    mv[1, 0] = (0, -8)
    v, sad = M.luma_vectors(flat, flat, mv, 2)
    assert not v.any() and not sad.any(), "every candidate ties: (0, 0) comes first"
    # ... and among the refinements the first in the order: cur = prev displaced by (2, 0) and by (3, 0) alike (columns repeat with period 1)
    v1, _ = M.luma_vectors(flat, flat, mv, 1)
    assert tuple(v1[0, 0]) == (2, 0) and tuple(v1[1, 0]) == (0, -16)


def test_the_centres_vector_applies_to_its_neighbours_across_a_block_edge():
    """two blocks side by side with different vectors: the sample in the last column of the left block takes its right neighbour's
    difference with the LEFT block's vector"""
    w, h = 32, 16
    cur, prev = _planes(w, h, 21), _planes(w, h, 22)
    vec = np.zeros((1, 2, 2), np.int64)
    vec[0, 0] = (3, 1)
    vec[0, 1] = (-2, 0)
    out = M.plane(cur, prev, vec, 16)
    x, y = 15, 7
    vx, vy = 3, 1
    c, p = int(cur[y, x]), int(prev[y + vy, x + vx])
    nsum = sum(int(cur[y + oy, x + ox]) - int(prev[y + oy + vy, x + ox + vx]) for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
    d, n = abs(c - p), abs(nsum) >> 2
    g = (255 - min(255, int(DM.GAIN[n]) << 2)) * (255 - int(DM.GAIN[d]))
    assert int(out[y, x]) == (p * g + (65535 - g) * c + 32768) >> 16
    wrong = sum(int(cur[y + oy, x + ox]) - int(prev[y + oy + (0 if ox == 1 else vy), x + ox + (-2 if ox == 1 else vx)]) for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
    assert wrong != nsum, "the case tells the two readings apart"


def test_prev_reads_are_clamped_at_the_plane_edge():
    w, h = 16, 16
    cur, prev = _planes(w, h, 31), _planes(w, h, 32)
    vec = np.zeros((1, 1, 2), np.int64)
    vec[0, 0] = (5, -4)
    out = M.plane(cur, prev, vec, 16)
    assert np.array_equal(out[0], cur[0]) and np.array_equal(out[-1], cur[-1]) and np.array_equal(out[:, 0], cur[:, 0]) and np.array_equal(out[:, -1], cur[:, -1])
    for x, y in ((13, 2), (1, 1), (14, 14)):
        cl = lambda a, hi: min(max(a, 0), hi)
        pr = lambda xx, yy: int(prev[cl(yy - 4, h - 1), cl(xx + 5, w - 1)])
        c, p = int(cur[y, x]), pr(x, y)
        nsum = sum(int(cur[y + oy, x + ox]) - pr(x + ox, y + oy) for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
        g = (255 - min(255, int(DM.GAIN[abs(nsum) >> 2]) << 2)) * (255 - int(DM.GAIN[abs(c - p)]))
        assert int(out[y, x]) == (p * g + (65535 - g) * c + 32768) >> 16, (x, y)


def test_samples_outside_the_blocks_take_the_zero_vector():
    w, h = 40, 24                                       # nbx = 2, nby = 1: columns 32.. and rows 16.. are outside
    cur, prev = _planes(w, h, 41), _planes(w, h, 42)
    vec = np.full((1, 2, 2), 3, np.int64)
    out = M.plane(cur, prev, vec, 16)
    zero = DM.plane(cur, prev)
    assert np.array_equal(out[17:, :], zero[17:, :]) and np.array_equal(out[:, 33:], zero[:, 33:])
    assert not np.array_equal(out[1:15, 1:31], zero[1:15, 1:31])


def test_an_all_zero_field_is_the_plain_denoiser():
    w, h, n = 202, 122, 4
    c = clips.make("scene", w, h, n)
    zero = [np.zeros(((h // 2) >> 3, (w // 2) >> 3, 2), np.int8)] * n
    want = DM.clip(c, w, h)
    got, cells = M.clip(c, w, h, 1, fields=zero)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert all(not v.any() for v, _ in cells)


def test_identical_frames_are_the_plain_denoiser_in_both_modes():
    w, h = 352, 288
    c = np.stack([clips.make("synth", w, h, 1)[0]] * 3)
    want = DM.clip(c, w, h)
    for mode in (1, 2):
        got, cells = M.clip(c, w, h, mode)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "mode %d" % mode
        assert all(not v.any() for v, _ in cells)


def _mse_pair(clean, w, h):
    noisy = M.hash_noise(clean)
    mc = M.luma_mse(M.clip(noisy, w, h, 2)[0][1:], clean[1:], w, h)
    plain = M.luma_mse(DM.clip(noisy, w, h)[1:], clean[1:], w, h)
    raw = M.luma_mse(noisy[1:], clean[1:], w, h)
    print("luma MSE of frames 1.. against the clean clip: raw %.2f, plain denoiser %.2f, motion-compensated (mode 2) %.2f" % (raw, plain, mc))
    return mc, plain


def test_noisy_pan_has_less_error_than_with_the_plain_denoiser():
    mc, plain = _mse_pair(clips.pan(352, 288, 6, step=5), 352, 288)
    assert mc < plain


def test_noisy_synth_has_less_error_than_with_the_plain_denoiser():
    mc, plain = _mse_pair(clips.make("synth", 352, 288, 6), 352, 288)
    assert mc < plain
