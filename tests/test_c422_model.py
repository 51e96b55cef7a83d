"""CPU: the 4:2:2 model (tests/c422_model.py) held to itself, without any library: a 4:2:2 frame that repeats the chroma rows of a 4:2:0
frame is that frame; the layouts of the same samples agree; the window formula at the picture's size IS (a + b + 1) >> 1, for every pair;
a pure crop is the ingest of the cropped region; a constant colour stays constant."""
import numpy as np
import pytest

import c422_model as CM
import hbd_model as HM
import scale_model as SM


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_repeated_chroma_rows_give_the_420_frames_slot(depth):
    fmt420, fmt = ("i420_16", "i422_16") if depth > 8 else ("i444", "i422")       # ("i444" draws 8-bit samples; only the luma's size matters here)
    y, u, v = HM.picture(64, 48, fmt420, depth, 1)
    u, v = u[:24, :32], v[:24, :32]
    want = HM.pack(*(HM.quantise(p, depth) if depth > 8 else p for p in (y, u, v)))
    assert np.array_equal(CM.slot(CM.from_420(y, u, v), fmt, depth), want)
    # ... through a window too: the chroma rows' pairs filter to what the single rows do
    assert np.array_equal(CM.slot(CM.from_420(y, u, v), fmt, depth, 32, 24), SM.scale_i420(*(HM.quantise(p, depth) if depth > 8 else p for p in (y, u, v)), 32, 24))


@pytest.mark.parametrize("sixteen", [False, True], ids=["u8", "u16"])
def test_layouts_of_the_same_samples_give_the_same_slot(sixteen):
    depth = 10 if sixteen else 8
    names = CM.FORMATS_16 if sixteen else CM.FORMATS_8
    planes = CM.picture(22, 6, names[0], depth, 2)
    want = CM.slot(planes, names[0], depth)
    want_win = CM.slot(planes, names[0], depth, 10, 4, (2, 0, 20, 6))
    for fmt in names:
        arrays = CM.layout(planes, fmt)
        assert len(arrays) == {"i422": 3, "nv16": 2}.get(CM.family(fmt), 1)
        back = CM.planes_of(arrays, fmt)
        assert all(np.array_equal(a, b) for a, b in zip(back, planes))
        assert np.array_equal(CM.slot(back, fmt, depth), want) and np.array_equal(CM.slot(back, fmt, depth, 10, 4, (2, 0, 20, 6)), want_win)
    y, u, v = planes
    yuyv, uyvy = CM.interleave_packed(y, u, v, "yuyv"), CM.interleave_packed(y, u, v, "uyvy")
    assert list(yuyv[0, :4]) == [y[0, 0], u[0, 0], y[0, 1], v[0, 0]] and list(uyvy[0, :4]) == [u[0, 0], y[0, 0], v[0, 0], y[0, 1]]
    assert list(CM.interleave_uv(u, v)[1, :4]) == [u[1, 0], v[1, 0], u[1, 1], v[1, 1]]


def test_window_formula_at_the_pictures_size_is_the_rounded_mean_of_every_pair():
    """all 65 536 pairs (a, b), one per column: the chroma window Sw/2 x Sh = 256 x 512 reduced to 256 x 256 against (a + b + 1) >> 1"""
    a, b = np.divmod(np.arange(65536, dtype=np.int64), 256)
    u = np.empty((512, 256), np.uint8)
    u[0::2] = a.reshape(256, 256)
    u[1::2] = b.reshape(256, 256)
    got = SM.scale_plane(u, 0, 0, 256, 512, 256, 256)
    assert np.array_equal(got, ((a + b + 1) >> 1).reshape(256, 256).astype(np.uint8))
    assert np.array_equal(got, CM.mean_rows(u))
    for aa, bb in ((0, 0), (0, 1), (1, 0), (254, 255), (255, 255), (7, 250)):       # ... and the text of the formula, sample by sample
        assert SM.scale_plane_direct(np.array([[aa], [bb]], np.uint8), 0, 0, 1, 2, 1, 1)[0, 0] == (aa + bb + 1) >> 1


@pytest.mark.parametrize("fmt", ["i422", "i422_16"])
def test_pure_crop_is_the_ingest_of_the_cropped_region(fmt):
    (sw, sh), (dw, dh), crop = CM.WINDOWS["pure_crop"]
    y, u, v = CM.picture(sw, sh, fmt, 12, 4)
    cx, cy, cw, ch = crop
    cut = (y[cy:cy + ch, cx:cx + cw], u[cy:cy + ch, cx // 2:(cx + cw) // 2], v[cy:cy + ch, cx // 2:(cx + cw) // 2])
    assert np.array_equal(CM.slot((y, u, v), fmt, 12, dw, dh, crop), CM.slot(cut, fmt, 12))
    assert np.array_equal(CM.slot(cut, fmt, 12, dw, dh), CM.slot(cut, fmt, 12))         # the at-size window is the plain ingest


@pytest.mark.parametrize("name", list(CM.WINDOWS))
def test_constant_colour_stays_constant(name):
    (sw, sh), (dw, dh), crop = CM.WINDOWS[name]
    for yv, uv, vv in ((16, 128, 128), (235, 16, 240), (0, 255, 1)):
        planes = (np.full((sh, sw), yv, np.uint8), np.full((sh, sw // 2), uv, np.uint8), np.full((sh, sw // 2), vv, np.uint8))
        got = CM.slot(planes, "i422", 8, dw, dh, crop)
        assert (got[:dw * dh] == yv).all() and (got[dw * dh:dw * dh * 5 // 4] == uv).all() and (got[dw * dh * 5 // 4:] == vv).all()
    planes16 = (np.full((sh, sw), 940, np.uint16), np.full((sh, sw // 2), 64, np.uint16), np.full((sh, sw // 2), 512, np.uint16))
    got = CM.slot(planes16, "nv16_16", 10, dw, dh, crop)
    assert (got[:dw * dh] == 235).all() and (got[dw * dh:dw * dh * 5 // 4] == 16).all() and (got[dw * dh * 5 // 4:] == 128).all()


def test_names():
    assert CM.FORMATS == ("i422", "nv16", "yuyv", "uyvy", "i422_16", "nv16_16", "yuyv_16", "uyvy_16")
    assert [CM.family(f) for f in ("p210", "y216", "yuy2", "uyvy_16")] == ["nv16", "yuyv", "yuyv", "uyvy"]
    assert CM.is_16("p216") and CM.is_16("y210") and not CM.is_16("yuy2")
