"""CPU: the model of the 16-bit and 4:4:4 device input (tests/hbd_model.py) against exact arithmetic.

  - the quantiser is floor(v / 2^(d-8) + 1/2) clamped to 255, in exact integer arithmetic, over all 65536 words for every depth;
  - the area filter of tests/scale_model.py at 2:1 is the rounded mean of the 2x2 blocks -- which is what makes the 4:4:4 ingest at the
    picture's size and its path through a window agree."""
from fractions import Fraction

import numpy as np
import pytest

import hbd_model as HM
import scale_model as SM


@pytest.mark.parametrize("d", list(HM.DEPTHS))
def test_quantiser_is_round_half_up_clamped(d):
    v = np.arange(65536)
    got = HM.quantise(v, d)
    # floor(v / 2^(d-8) + 1/2) = floor((2 v + 2^(d-8)) / 2^(d-7)): Python integers, no rounding anywhere
    want = np.array([min(255, (2 * int(x) + (1 << (d - 8))) // (1 << (d - 7))) for x in v], np.uint8)
    assert np.array_equal(got, want)
    assert got[0] == 0 and got[(1 << d) - 1] == 255 and (got[1 << d:] == 255).all()
    assert np.all(np.diff(got.astype(int)) >= 0)
    # a few words against rationals, the halves included
    for x in (0, 1, (1 << (d - 9)) - 1, 1 << (d - 9), 3 << (d - 9), (1 << d) - 1 - (1 << (d - 9)), (1 << d) - (1 << (d - 9)), 65535):
        if x < 0:
            continue
        assert got[x] == min(255, int(Fraction(x, 1 << (d - 8)) + Fraction(1, 2)))
    # int16 tensors hold the same bits
    assert np.array_equal(HM.quantise(v.astype(np.uint16).view(np.int16), d), got)


def test_ten_bit_limited_range_maps_onto_eight_bit_limited_range():
    assert list(HM.quantise([64, 940, 960, 512, 1023, 1024, 65535], 10)) == [16, 235, 240, 128, 255, 255, 255]
    assert list(HM.quantise([64 << 6, 940 << 6, 0xffc0], 16)) == [16, 235, 255]        # the same picture as an MSB-aligned P010 surface


@pytest.mark.parametrize("w,h,cx,cy", [(2, 2, 0, 0), (6, 4, 0, 0), (64, 48, 0, 0), (30, 22, 6, 2)])
def test_area_filter_at_2_to_1_is_the_2x2_rounded_mean(w, h, cx, cy):
    rng = np.random.default_rng(w * h)
    src = rng.integers(0, 256, (h + cy + 3, w + cx + 5)).astype(np.uint8)
    src[cy:cy + 2, cx:cx + 2] = 255                 # a saturated block and one that rounds up from x.5
    if w > 2:
        src[cy:cy + 2, cx + 2:cx + 4] = [[1, 0], [0, 1]]
    got = SM.scale_plane(src, cx, cy, w, h, w // 2, h // 2)
    assert np.array_equal(got, HM.mean2x2(src[cy:cy + h, cx:cx + w]))
    assert np.array_equal(got, SM.scale_plane_direct(src, cx, cy, w, h, w // 2, h // 2))


def test_444_slot_at_size_equals_the_pure_crop_through_a_window():
    y, u, v = HM.picture(40, 24, "i444_16", 10)
    at_size = HM.slot((y[4:20, 6:30], u[4:20, 6:30], v[4:20, 6:30]), "i444_16", 10)
    assert np.array_equal(HM.slot((y, u, v), "i444_16", 10, 24, 16, (6, 4, 24, 16)), at_size)
    assert at_size.size == 24 * 16 * 3 // 2


def test_pictures_cover_the_range_and_the_garbage_bits():
    for fmt in HM.FORMATS:
        for d in (10, 12, 16):
            y, u, v = HM.picture(64, 48, fmt, d)
            assert u.shape == ((48, 64) if HM.is_444(fmt) else (24, 32))
            if HM.is_16(fmt):
                assert y.dtype == np.uint16 and (d == 16 or (y >> d).any())
                q = HM.quantise(y, d)
                assert q.min() == 0 and q.max() == 255
    y, u, v = HM.all_patterns_picture()
    assert np.array_equal(np.sort(y.reshape(-1)), np.repeat(np.arange(65536), 2))
    assert np.array_equal(np.sort(u.reshape(-1)), np.arange(32768)) and np.array_equal(np.sort(v.reshape(-1)), np.arange(32768, 65536))
