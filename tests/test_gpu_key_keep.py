"""GPU: key frames that a stopped launch had (partly) encoded are kept across the relaunch (h264e_host.c clip_keep_collect,
clip_plan_launch) on the MI355X, where the frames of a launch really run beside each other: a mis-speculated mv_clusters state
stops the launch while the key frames behind the failed frame are somewhere between their first and their last row.  Short GOPs put a key
frame next to nearly every event.  How many rows were complete at the abort depends on timing, so for those clips only the bytes are
checked -- against the oracle, and with the switch off; the counts are printed.  The full-buffer stop of tests/test_emu_key_keep.py is
deterministic enough on the device too: the frames behind the one that did not fit are long complete when the host notices."""
import pytest

import key_keep_cases as cases
import pkg

pytestmark = pytest.mark.gpu

CIF = ("pan", 352, 288, 90, dict(gop=6, qp=26))
SMALL = ("pan", 96, 80, 60, dict(gop=4, qp=26))


def _encode(case, **run):
    name, w, h, n, kw = case
    out, sizes, tot = cases.encode(pkg.load_pkg(), cases.clip(name, w, h, n), w, h, **run, **kw)
    print("%dx%d x %d gop %d %s: %s" % (w, h, n, kw["gop"], run, tot))
    return out, sizes, tot


@pytest.mark.parametrize("case", [CIF, SMALL], ids=["352x288x90-gop6", "96x80x60-gop4"])
def test_events_next_to_key_frames_stream_is_the_oracles(case):
    name, w, h, n, kw = case
    want, want_sizes = cases.reference(name, w, h, n, **kw)
    out, sizes, tot = _encode(case)
    assert sizes == want_sizes and out == want
    assert tot["spin_relaunches"] == 0
    assert tot["reencoded_gops"] > 0                # the clip does mis-speculate: launches were stopped with key frames behind


def test_keeping_on_and_off_give_the_same_bytes():
    on, off = _encode(CIF), _encode(CIF, keep=False)
    assert on[:2] == off[:2]
    assert off[2]["kept_key_frames"] == 0 and off[2]["kept_key_rows"] == 0
    assert on[2]["spin_relaunches"] == 0 and off[2]["spin_relaunches"] == 0


def test_full_buffer_stops_keep_key_frames():
    name, w, h, n, kw = SMALL
    want, want_sizes = cases.reference(name, w, h, n, **kw)
    out, sizes, tot = _encode(SMALL, cap=cases.cap_for_three(want_sizes))
    assert sizes == want_sizes and out == want
    assert tot["calls"] > 1 and tot["spin_relaunches"] == 0
    assert tot["kept_key_frames"] > 0
