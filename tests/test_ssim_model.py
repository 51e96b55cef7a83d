"""CPU: the SSIM definition (tests/ssim_model.py) against hand-computed values and its own claims -- exact 1.0 for identical planes, the
closed form of the most unequal window, the size of the four factors, which samples take part."""
import numpy as np
import pytest

import clips
import ssim_model as SM


def noise(w, h, salt=1):
    return clips._hash_bytes(w * h, salt).reshape(h, w)


def checker(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


# the pairs at which a factor is largest or vars smallest
EXTREMES = {
    "0_255": lambda w, h: (np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)),
    "255_255": lambda w, h: (np.full((h, w), 255, np.uint8), np.full((h, w), 255, np.uint8)),
    "noise_inverse": lambda w, h: (noise(w, h), 255 - noise(w, h)),
    "checker_inverse": lambda w, h: (checker(w, h), 255 - checker(w, h)),
}


@pytest.mark.parametrize("w,h", [(8, 8), (18, 22), (9, 17), (272, 80)])
def test_identical_planes_give_exactly_one(w, h):
    for a in (noise(w, h), checker(w, h), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
        assert SM.plane(a, a.copy()) == 1.0
        assert (SM.window_values(a, a) == 1.0).all()


def test_zero_against_255_in_one_window():
    a, b = EXTREMES["0_255"](8, 8)
    n1, n2, d1, d2 = SM.factors(a, b)
    # s1 = 0, s2 = 64*255, ss = 64*255^2, s12 = 0: vars = 0, covar = 0
    assert (int(n1[0, 0]), int(n2[0, 0]), int(d1[0, 0]), int(d2[0, 0])) == (416, 235963, 16320 ** 2 + 416, 235963)
    assert SM.plane(a, b) == 416 / 266342816
    assert SM.plane(a, b) == (416.0 * 235963.0) / (266342816.0 * 235963.0)


@pytest.mark.parametrize("name", sorted(EXTREMES))
def test_factors_stay_below_2_30_and_vars_is_not_negative(name):
    for w, h in ((8, 8), (32, 24)):
        a, b = EXTREMES[name](w, h)
        n1, n2, d1, d2 = SM.factors(a, b)
        for f in (n1, n2, d1, d2):
            assert int(np.abs(f).max()) < 1 << 30
        assert int((d2 - SM.C2).min()) >= 0 and int(d1.min()) > 0            # vars >= 0: the denominator is positive
        v = SM.window_values(a, b)
        assert np.isfinite(v).all() and float(np.abs(v).max()) <= 1.0


@pytest.mark.parametrize("w,h,nx,ny", [(18, 22, 3, 4), (9, 17, 1, 3), (8, 8, 1, 1), (16, 16, 3, 3)])
def test_window_count_and_ragged_samples_take_no_part(w, h, nx, ny):
    assert SM.windows(w, h) == (nx, ny)
    a, b = noise(w, h, 3), noise(w, h, 4)
    assert SM.window_values(a, b).shape == (ny, nx)
    want = SM.plane(a, b)
    a2, b2 = a.copy(), b.copy()
    a2[4 * (h >> 2):, :] ^= 0xFF
    b2[:, 4 * (w >> 2):] ^= 0x55
    assert SM.plane(a2, b2) == want
    b3 = b.copy()
    b3[4 * (h >> 2) - 1, 4 * (w >> 2) - 1] ^= 0x80                          # the last sample that does take part
    assert SM.plane(a, b3) != want


def test_no_window_is_refused():
    with pytest.raises(AssertionError, match="no 8 x 8 window"):
        SM.plane(np.zeros((7, 16), np.uint8), np.zeros((7, 16), np.uint8))


def test_one_sample_moves_the_mean_far_beyond_the_tolerance():
    w, h = 272, 80
    a, b = noise(w, h, 5), noise(w, h, 6)
    b2 = b.copy()
    b2[40, 100] = b2[40, 100] + 1 if b2[40, 100] < 255 else 254
    assert abs(SM.plane(a, b2) - SM.plane(a, b)) > 100 * SM.tolerance(w, h)


def test_line_and_all():
    assert SM.all_of(1.0, 1.0, 1.0) == 1.0
    assert SM.line([[0.5, 0.25, 0.75], [0.5, 0.75, 0.25]]) == "SSIM Y=0.500000 U=0.500000 V=0.500000 All=0.500000 (3.01 db)"
    assert SM.line([[1.0, 1.0, 1.0]]) == "SSIM Y=1.000000 U=1.000000 V=1.000000 All=1.000000 (inf db)"
