"""CPU: the HDR10 device input's definition and its tables.  The library's tables (H264E_tonemap_tables, a pure host function, here from
the emulation library) against the double-precision formulas of tests/tonemap_model.py; the properties the kernel's search rests on; and
what the definition does to a grey ramp.  The deviation from the same chain in float64 is printed: a property of the definition
(DESIGN.md 4.5p), not a pass mark."""
import os
import subprocess

import numpy as np
import pytest

import pkg
import tonemap_model as TM

HERE = os.path.dirname(os.path.abspath(__file__))
PARAMETERS = [(1000, 203), (4000, 100)]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def tables(curve, peak, white):
    return pkg.load_pkg().tonemap_tables({"transfer": "pq", "curve": curve, "peak": peak, "ref_white": white}, lib=pkg.EMU_LIB)


def ulps(a, b):
    """the distance of two arrays of finite float32 of one sign in units of the last place"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


def test_ycc_is_rint_of_its_expressions():
    ycc = tables("hable", 0, 0)[0]
    assert ycc.tolist() == [int(np.rint(16384 * x)) for x in TM.YCC_EXPR] + [64, 512, 14]
    assert ycc.tolist()[:5] == [19133, 27584, 3078, 10688, 35194]       # the integers the header lists
    # every product and sum of step 2 fits 32 bits: |y| < 2^10, |u|, |v| <= 2^9, the rounding constant 2^13
    assert 960 * ycc[0] + 512 * max(ycc[1], ycc[2] + ycc[3], ycc[4]) + 8192 < 2 ** 31


@pytest.mark.parametrize("curve", TM.CURVES)
@pytest.mark.parametrize("peak,white", PARAMETERS)
def test_tables_agree_with_the_double_precision_formulas(curve, peak, white):
    """both sides round a double whose libm error is far below a float32 ulp: they can differ only on a near-tie, by one ulp"""
    _, eotf, scale, thresh = tables(curve, peak, white)
    _, f_eotf, f_scale, f_thresh = TM.table_formulas(curve, peak, white)
    for name, a, b in (("eotf", eotf, f_eotf), ("scale", scale, f_scale), ("thresh", thresh, f_thresh)):
        assert np.isfinite(a).all() and (a >= 0).all()
        assert ulps(a, b.astype(np.float32)).max() <= 1, name
    assert (np.diff(eotf) >= 0).all() and (np.diff(thresh) >= 0).all() and eotf[0] == 0 and scale[0] == 1
    assert (np.diff(thresh[1:]) > 0).all()                              # the count of step 5 is a position in a strictly increasing list
    one_ulp_above_1 = np.nextafter(np.float32(1), np.float32(2))
    assert (scale * eotf <= one_ulp_above_1).all()                      # a float32 product, as the kernel forms it
    assert eotf[1023] == np.float32(10000 / white)


def test_defaults_are_1000_and_203():
    a, b = tables("hable", 0, 0), tables("hable", 1000, 203)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(tables("hable", 4000, 203)[2], a[2]) and not np.array_equal(tables("clip", 0, 0)[2], a[2])


@pytest.mark.parametrize("curve", TM.CURVES)
@pytest.mark.parametrize("peak,white", PARAMETERS)
def test_grey_ramp(curve, peak, white):
    """neutral chroma and the Y ramp 64 .. 940 with the library's tables: non-decreasing, R, G and B within 1 code of each other (the
    matrix rows sum to 1 +- 0.0001, so not exactly equal), black to black, and the code whose light is the peak to 255"""
    t = tables(curve, peak, white)
    ramp = np.arange(64, 941)
    y = np.repeat(np.concatenate([ramp, ramp[-1:]])[None], 2, axis=0).astype(np.uint16)     # an even width
    c = np.full((1, y.shape[1] // 2), 512, np.uint16)
    out = TM.rgb8((y, c, c), 10, t).astype(np.int64)[:, 0, :len(ramp)]
    assert np.abs(np.rint(TM.GAMUT * 10000).sum(axis=1) - 10000).max() <= 1         # the rows as printed, four decimals: sums within 0.0001 of 1
    assert (np.diff(out, axis=1) >= 0).all()
    assert np.abs(out - out[1]).max() <= 1
    assert out[:, 0].tolist() == [0, 0, 0]
    at_peak = int(np.searchsorted(t[1].astype(np.float64) * white, peak))        # the first code whose light reaches peak_nits
    rgb10 = np.full((3, 1, 1), at_peak)
    assert TM.sdr_codes(rgb10, t).ravel().tolist() == [255, 255, 255]
    luma = ramp[np.searchsorted(TM.rgb_codes(ramp, np.full(len(ramp), 512), np.full(len(ramp), 512), t[0])[0][0], at_peak)]
    assert out[:, luma - 64].tolist() == [255, 255, 255]


def test_deviation_from_the_float64_chain_is_reported():
    """the 8-bit R'G'B' against the same chain in float64 without the 10-bit code step: printed (pytest -s), recorded in DESIGN.md 4.5p"""
    worst = {}
    for curve in TM.CURVES:
        t = tables(curve, 0, 0)
        for depth in (10, 12, 16):
            d = 0
            for n in range(2):
                f = TM.picture(66, 48, depth, n)
                d = max(d, int(np.abs(TM.rgb8(f, depth, t).astype(np.int64) - TM.rgb8_float64(f, depth, curve).astype(np.int64)).max()))
            worst[(curve, depth)] = d
            print("tonemap: largest deviation from float64, %s at depth %d: %d codes" % (curve, depth, d))
    assert len(worst) == 9
