"""GPU: the coming key frames' row workgroups at the front of a launch's dispatch order (h264e_pool.h lead_jobs / order_by_start_step,
DESIGN.md 5) on the MI355X.  Leading is on only where a launch's grid exceeds the resident workgroups of its kernel variant (1536), so the
shapes here are launches of 2000+ workgroups with key frames in the middle: the led rows run beside the chain from the launch's start,
a mis-speculation or a full buffer stops the launch, and the next one starts the key frames at the rows they got to.  Each shape is
encoded with the lead on and with H264E_KEY_LEAD=0: the bytes are the oracle's both times and no bounded wait expires.  How many frames
were led and kept depends on timing: printed, not asserted."""
import pytest

import key_keep_cases as cases
import key_lead_cases as lead

pytestmark = pytest.mark.gpu

CIF = ("pan", 352, 288, 120, dict(gop=6, qp=26))               # 120 x 19 = 2280 workgroups
TALL = ("pan", 16, 2048, 16, dict(gop=4, qp=26))               # 16 x 129 = 2064 workgroups
SHAPES = [CIF, TALL, CIF[:4] + (dict(gop=6, qp=26, slices=2),)]
IDS = ["352x288x120-gop6", "16x2048x16-gop4", "352x288x120-gop6-2slices"]


@pytest.mark.parametrize("case", SHAPES, ids=IDS)
@pytest.mark.parametrize("on", [None, 0], ids=["lead", "lead-off"])
def test_stream_is_the_oracles_with_and_without_the_lead(case, on):
    name, w, h, n, kw = case
    want, want_sizes = cases.reference(name, w, h, n, **kw)
    out, sizes, tot = lead.encode(name, w, h, n, lead=on, **kw)
    print("%dx%d x %d %s lead %s: %s" % (w, h, n, kw, on, tot))
    assert sizes == want_sizes and out == want
    assert tot["spin_relaunches"] == 0
    if on == 0:
        assert tot["led_frames"] == 0 and tot["led_rows"] == 0


@pytest.mark.parametrize("on", [None, 0], ids=["lead", "lead-off"])
def test_launch_group_of_two_clips(on):
    w, h = 352, 288
    specs = [("pan", 90, dict(gop=6, qp=26)), ("pan", 90, dict(gop=5, qp=26))]
    res, led = lead.encode_pair(specs, w, h, lead=on)
    print("group of two 352x288 x 90, lead %s: led %s, %s" % (on, led, [r[2] for r in res]))
    for (out, sizes, tot), (name, n, kw) in zip(res, specs):
        want, want_sizes = cases.reference(name, w, h, n, **kw)
        assert sizes == want_sizes and out == want
        assert tot["spin_relaunches"] == 0
    if on == 0:
        assert led == (0, 0)


@pytest.mark.parametrize("on", [None, 0], ids=["lead", "lead-off"])
def test_stops_by_a_full_buffer_of_three_frames(on):
    name, w, h, n, kw = "pan", 352, 288, 90, dict(gop=6, qp=26)
    want, want_sizes = cases.reference(name, w, h, n, **kw)
    out, sizes, tot = lead.encode(name, w, h, n, lead=on, cap=cases.cap_for_three(want_sizes), **kw)
    print("352x288 x 90 through a buffer of 3 frames, lead %s: %s" % (on, tot))
    assert sizes == want_sizes and out == want
    assert tot["calls"] > 1 and tot["spin_relaunches"] == 0
    if on == 0:
        assert tot["led_frames"] == 0 and tot["led_rows"] == 0
