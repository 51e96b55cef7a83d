"""CPU emulation: the search wave's reference window slides along the macroblock row -- one strip of newly valid columns per macroblock
instead of the whole window (enc_kernels.h wave_slide_window, enc_row.h row_prefetch) -- and every stream stays the oracle's, byte for
byte.  Picture widths: narrower than or as wide as the window (never slides); wide enough that the first strip directly follows a clamped
load at the left border; 21 macroblocks (many slides between both borders).  Content: a pan of 20 samples per frame (vectors that use
the strip just loaded, and reads that leave the window), noise (no macroblock is skipped), synth_v1 (skipped and searched macroblocks
alternate).  Both window geometries, one and two slices, and a relaunch that starts at a macroblock row greater than 0."""
import functools
import subprocess
import os

import pytest

import clips
import launch_lines
import oracle_lib
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
QP = 26
SIZES = [(16, 16, 8), (48, 32, 8), (64, 48, 8), (80, 48, 8), (96, 64, 8), (176, 144, 6), (336, 64, 8)]
CLIPS = ["pan", "noise", "synth"]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@functools.lru_cache(maxsize=None)
def make_clip(name, w, h, n):
    c = clips.pan(w, h, n, step=20) if name == "pan" else clips.make(name, w, h, n)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, w, h, n, slices, gop=30):
    """the oracle's stream, computed once and shared by both window geometries"""
    return oracle_lib.encode_clip(make_clip(name, w, h, n), w, h, gop=gop, qp=QP, slices=slices)


def encode(name, w, h, n, slices, gop=30, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, gop=gop, qp=QP, slices=slices, **kw)
    ce.upload(make_clip(name, w, h, n))
    out, sizes, st = ce.encode()
    ce.close()
    return out, sizes, st


def cases():
    for w, h, n in SIZES:
        for slices in (0, 2):
            if slices and h < 32:
                continue            # two slices need two macroblock rows
            for name in CLIPS:
                yield name, w, h, n, slices


@pytest.mark.parametrize("geometry", ["narrow", "wide"])
@pytest.mark.parametrize("name,w,h,n,slices", list(cases()), ids=lambda v: str(v))
def test_sliding_window_matches_oracle(monkeypatch, geometry, name, w, h, n, slices):
    if geometry == "wide":
        monkeypatch.setenv("H264E_WIDE_WINDOW", "1")
    want, want_sizes = reference(name, w, h, n, slices)
    out, sizes, _ = encode(name, w, h, n, slices, lib=pkg.EMU_LIB)
    assert sizes == want_sizes and out == want


@pytest.mark.parametrize("geometry", ["narrow", "wide"])
def test_relaunch_from_a_lower_row_loads_the_whole_window_first(monkeypatch, capfd, geometry):
    """a mis-speculated frame is encoded again from the macroblock row of its first wrong macroblock: the workgroups of that launch start
    below row 0 with nothing in their windows.  (The launch lines of H264E_DEBUG say at which row a launch started.)"""
    if geometry == "wide":
        monkeypatch.setenv("H264E_WIDE_WINDOW", "1")
    monkeypatch.setenv("H264E_DEBUG", "1")
    name, w, h, n, gop = "pan", 176, 144, 8, 30
    want, want_sizes = reference(name, w, h, n, 0, gop)
    out, sizes, st = encode(name, w, h, n, 0, gop, lib=pkg.EMU_LIB)
    first_rows = [l.first_row for l in launch_lines.parse(capfd.readouterr().err)]
    assert st.reencoded_gops > 0 and max(first_rows) > 0, first_rows
    assert sizes == want_sizes and out == want
