"""GPU: the lookahead's cost pass with a motion search (h264e_lookahead_search_kernel, enc_lookahead_search.h) on the MI355X: records and
motion fields against the numpy model (tests/lookahead_motion_model.py) at the shapes of the emulation test, device input against host
upload, the default (search off) against what the commit before the search recorded (tests/golden/lookahead_off.json), the controller
against the model's plan, and its bitrate against the target with the bound of tests/test_gpu_lookahead.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import clips
import lookahead_model as M
import pkg
from test_emu_lookahead_motion import CTL, IDS, SHAPES, analyse_twice, check_controller, check_shape, model, same, same_fields

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = json.load(open(os.path.join(HERE, "golden", "lookahead.json")))
OFF = json.load(open(os.path.join(HERE, "golden", "lookahead_off.json")))


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("w,h,clip,n,R", SHAPES, ids=IDS)
def test_records_and_fields_equal_the_model_twice(P, w, h, clip, n, R):
    """two encoders, so the kernel runs twice: its sums are atomics from hundreds of workgroups, in any order"""
    check_shape(P, None, w, h, clip, n, R)
    check_shape(P, None, w, h, clip, n, R)


def test_1080p_sums_from_a_thousand_workgroups(P):
    """1920x1080: 60 x 67 blocks, 8 strips x 67 rows of single-wave workgroups adding to one record; the last strip holds 4 blocks"""
    check_shape(P, None, 1920, 1080, "scene", 3, 8)


def test_device_input_gives_the_fields_of_host_upload(P):
    import torch
    w, h, clip, n, R = 176, 144, "ramp", 5, 8
    c, rec, fields = model(w, h, clip, n, R)
    srcs = []
    for f in c:
        y, u, v = f[: w * h].reshape(h, w), f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)
        srcs.append((torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(np.stack([u, v], axis=-1).reshape(h // 2, w).copy()).cuda()))
    ce = P.ClipEncoder(w, h, n, gop=4, qp=30, abr_kbps=100, lookahead=2, lookahead_search=R)
    ce.upload_device(srcs, "nv12")
    out, sizes, st = ce.encode()
    got_rec, qp = ce.read_lookahead()
    got_fields = [ce.read_lookahead_motion(f) for f in range(n)]
    ce.close()
    host = analyse_twice(P, None, w, h, c, R)
    assert st.spin_relaunches == 0
    assert same(got_rec, rec) and same_fields(got_fields, fields) and same_fields(got_fields, host[1])
    assert np.array_equal(qp, host[2]) and (out, sizes) == host[3:]


def test_search_off_keeps_every_record_and_byte(P):
    """after a clip with search has run in this process (the new kernel is loaded and the rings exist): the default is the pass and the
    stream of the commit before"""
    g = OFF
    w, h, n = g["w"], g["h"], g["frames"]
    c = clips.make(g["clip"], w, h, n)
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    check_shape(P, None, *SHAPES[1])
    for kw in (dict(), dict(lookahead_search=0)):
        ce = P.ClipEncoder(w, h, n, gop=g["gop"], qp=30, abr_kbps=g["kbps"], lookahead=g["window"], **kw)
        ce.upload(c)
        out, sizes, st = ce.encode()
        (i, p, nb), qp = ce.read_lookahead()
        with pytest.raises(P.H264EError):
            ce.read_lookahead_motion(1)
        ce.close()
        assert (i.tolist(), p.tolist(), nb.tolist()) == (g["intra"], g["inter"], g["intra_blocks"]) and same((i, p, nb), M.costs(c, w, h))
        assert qp.tolist() == g["qp"] and sizes == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"] and st.spin_relaunches == 0


def test_controller_is_the_models_plan_on_searched_costs(P):
    w, h, n, gop, W, kbps, R = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R"))
    c = clips.make("synth", w, h, n)
    rec, _, qp, out, sizes = analyse_twice(P, None, w, h, c, R, frames=[], gop=gop, abr_kbps=kbps, lookahead=W)
    check_controller(dict(P=P, clip=c, out=out, sizes=sizes, rec=rec, qp=qp), None)


@pytest.mark.parametrize("g", [g for g in RATES if g["kbps"] == 300], ids=lambda g: "%s_%dkbps" % (g["clip"], g["kbps"]))
def test_bitrate_with_search_stays_within_one_window_of_the_target(P, g):
    """the bound of test_gpu_lookahead.test_bitrate_stays_within_one_window_of_the_target -- |actual - target| over the clip <= one
    window's budget (8*dfb*W bits) + the reference controller's own absolute deviation for the same clip and target -- at CIF x 128,
    GOP 30, W = 16, with search 8"""
    w, h, n, W = g["w"], g["h"], g["frames"], 16
    c = clips.make(g["clip"], w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=g["gop"], qp=30, abr_kbps=g["kbps"], lookahead=W, lookahead_search=8)
    ce.upload(c)
    out, sizes, st = ce.encode()
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    dfb = g["kbps"] * 1000 // 8 // 30
    target, actual, ref = 8 * dfb * n, 8 * len(out), 8 * g["bytes"]
    bound = 8 * dfb * W + abs(ref - target)
    print("%s %d kbps, search 8: target %d bits, actual %d, reference %d, deviation %d, bound %d, QPs per window %s, %d launches" %
          (g["clip"], g["kbps"], target, actual, ref, abs(actual - target), bound, qp[::W].tolist(), st.rounds))
    assert st.spin_relaunches == 0 and sizes and len(sizes) == n
    assert abs(actual - target) <= bound
