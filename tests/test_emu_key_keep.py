"""CPU emulation: a key frame that a cleanly stopped launch had (partly) encoded is not encoded again (h264e_host.c clip_keep_collect,
clip_plan_launch).  The emulation runs the jobs of a launch one after the other, so behind the frame that did not fit the
caller's buffer every key frame of the launch has finished (its done word is up, which is how h264e_hip_stream_rows_complete knows a whole
frame; the emulation's rows publish no counters): the next call starts them at first_row = nmby, where only the finalizer runs
(splice, walk and export from counters that all say complete), or -- with the row count capped by a test knob -- at a row in between.
Every stream stays the oracle's, byte for byte, and is the same with H264E_KEEP_KEY_ROWS=0."""
import functools
import os
import subprocess

import pytest

import key_keep_cases as cases
import launch_lines
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
N = 24

# (clip, width, height, stream parameters)
FULL_BUFFER = [(name, 96, 80, dict(gop=gop, qp=26)) for name in ("pan", "synth_v1") for gop in (4, 7)] + \
              [(name, 64, 48, dict(gop=4, qp=26, slices=2)) for name in ("pan", "synth_v1")]
IDS = ["%s-%dx%d-gop%d%s" % (c[0], c[1], c[2], c[3]["gop"], "-2slices" if c[3].get("slices") else "") for c in FULL_BUFFER]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@functools.lru_cache(maxsize=None)
def _run(i, keep):
    name, w, h, kw = FULL_BUFFER[i]
    want, want_sizes = cases.reference(name, w, h, N, **kw)
    return cases.encode(pkg.load_pkg(), cases.clip(name, w, h, N), w, h, cap=cases.cap_for_three(want_sizes), keep=keep, lib=pkg.EMU_LIB, **kw)


@pytest.mark.parametrize("i", range(len(FULL_BUFFER)), ids=IDS)
def test_full_buffer_stops_keep_key_frames_and_the_stream_is_the_oracles(i):
    name, w, h, kw = FULL_BUFFER[i]
    want, want_sizes = cases.reference(name, w, h, N, **kw)
    out, sizes, tot = _run(i, True)
    assert sizes == want_sizes and out == want
    assert tot["calls"] > 1                         # the buffer did stop launches
    assert tot["kept_key_frames"] > 0
    # the emulation leaves every frame of a launch complete: a kept key frame is kept whole
    assert tot["kept_key_rows"] == tot["kept_key_frames"] * ((h + 15) // 16)


@pytest.mark.parametrize("i", range(len(FULL_BUFFER)), ids=IDS)
def test_switched_off_nothing_is_kept_and_the_bytes_are_the_same(i):
    out, sizes, tot = _run(i, False)
    assert (out, sizes) == _run(i, True)[:2]
    assert tot["kept_key_frames"] == 0 and tot["kept_key_rows"] == 0
    assert tot["calls"] == _run(i, True)[2]["calls"]


def test_launches_with_hedge_leaves_keep_nothing():
    # rate control, 8 slots: room for hedge leaves behind the 6 frames of a launch (tests/geometry_switch_cases.py)
    w, h, kw = 96, 80, dict(gop=4, kbps=300)
    want, want_sizes = cases.reference("pan", w, h, N, **kw)

    def go():
        with launch_lines.captured_stderr() as err:
            res = cases.encode(pkg.load_pkg(), cases.clip("pan", w, h, N), w, h, cap=cases.cap_for_three(want_sizes), lib=pkg.EMU_LIB, max_chains=8, **kw)
        return res, launch_lines.parse(err[0])
    (out, sizes, tot), launches = cases.with_env({"H264E_DEBUG": "1"}, go)
    assert sizes == want_sizes and out == want
    assert any(l.hedged for l in launches) and tot["calls"] > 1
    assert tot["kept_key_frames"] == 0 and tot["kept_key_rows"] == 0


@pytest.mark.parametrize("rows", [0, 2, 5])
def test_partly_kept_key_frame_restarts_below_the_kept_rows(rows):
    # 80 rows of samples = 5 macroblock rows; the knob caps the rows reported complete: none, the upper two (the frame goes again from
    # row 2, which reads the pending lines and records of row 1), all five (the uncapped answer)
    name, w, h, kw = "pan", 96, 80, dict(gop=4, qp=26)
    want, want_sizes = cases.reference(name, w, h, N, **kw)
    out, sizes, tot = cases.encode(pkg.load_pkg(), cases.clip(name, w, h, N), w, h, cap=cases.cap_for_three(want_sizes), lib=pkg.EMU_LIB,
                                   knobs={"H264E_TEST_KEEP_ROWS_CAP": str(rows)}, **kw)
    assert sizes == want_sizes and out == want
    assert tot["calls"] > 1
    if rows == 0:
        assert tot["kept_key_frames"] == 0
    else:
        assert tot["kept_key_frames"] > 0 and tot["kept_key_rows"] == rows * tot["kept_key_frames"]
