"""GPU: the sliding reference window (enc_kernels.h wave_slide_window) on the MI355X, where the frames of a launch overlap in time: a strip
loaded one macroblock early, or from the dword where the previous load ended instead of the one that holds the first newly valid column,
would read samples the frame in front has not finished.  Both window geometries against the oracle, byte for byte, on a picture of 21
macroblocks per row, on one whose first strip directly follows the clamped load at the left border, and on a general small one; no
dependency wait may have needed its bounded spin to expire."""
import functools

import pytest

import clips
import oracle_lib
import pkg

pytestmark = pytest.mark.gpu

QP, FRAMES = 26, 8
SIZES = [(336, 64), (96, 64), (176, 144)]
CLIPS = ["pan", "noise", "synth"]


@functools.lru_cache(maxsize=None)
def make_clip(name, w, h):
    c = clips.pan(w, h, FRAMES, step=20) if name == "pan" else clips.make(name, w, h, FRAMES)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, w, h, slices):
    """the oracle's stream, computed once and shared by both window geometries"""
    return oracle_lib.encode_clip(make_clip(name, w, h), w, h, gop=30, qp=QP, slices=slices)


@pytest.mark.parametrize("geometry", ["narrow", "wide"])
@pytest.mark.parametrize("slices", [0, 2])
@pytest.mark.parametrize("name", CLIPS)
@pytest.mark.parametrize("w,h", SIZES)
def test_sliding_window_matches_oracle(monkeypatch, w, h, name, slices, geometry):
    if geometry == "wide":
        monkeypatch.setenv("H264E_WIDE_WINDOW", "1")
    want, want_sizes = reference(name, w, h, slices)
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, FRAMES, gop=30, qp=QP, slices=slices)
    ce.upload(make_clip(name, w, h))
    out, sizes, st = ce.encode()
    ce.close()
    assert sizes == want_sizes and out == want
    assert st.spin_relaunches == 0
