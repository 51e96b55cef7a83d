"""GPU: the lookahead's cost tree (h264e_lookahead_tree_kernel, enc_lookahead_tree.h) on the MI355X: block maps, sums, offsets and
the plan against the numpy model (tests/lookahead_tree_model.py) at the shapes of the emulation test, a 1080p window, strength 0 against
the clip without the option, the controller with offsets against the model's plan, and its bitrate against the target with the bound of
tests/test_gpu_lookahead_motion.py."""
import json
import os

import numpy as np
import pytest

import clips
import pkg
from test_emu_lookahead_motion import same
from test_emu_lookahead_tree import AHEADS, GOP, IDS, KBPS, SHAPES, STRENGTH, W, analysed, check_controller, check_shape, encode_twice, model

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RATES = json.load(open(os.path.join(HERE, "golden", "lookahead.json")))


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("w,h,clip,n,R", SHAPES, ids=IDS)
def test_maps_sums_offsets_and_plan_equal_the_model_twice(P, w, h, clip, n, R, ahead):
    """two encoders of two passes each: the maps are 64-bit atomics from up to nine blocks per cell, in any order"""
    check_shape(P, None, w, h, clip, n, R, ahead)
    check_shape(P, None, w, h, clip, n, R, ahead, plan=False)


def test_1080p_window_of_four_frames(P):
    """1920x1080: 60 x 67 = 4020 blocks, 503 single-wave workgroups adding to one sum, the last one with 4 blocks; one window of 4 frames"""
    w, h, n, R = 1920, 1080, 4, 4
    c, rec, kinds, maps, S, delta = model(w, h, "scene", n, R, 0, 30, 4, STRENGTH)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=30, abr_kbps=4000, lookahead=4, lookahead_search=R, lookahead_tree=(STRENGTH, 0))
    ce.upload(c)
    for _ in range(2):
        ce.encode()
        got_s, got_d, _ = ce.read_lookahead_tree_sums()
        assert np.array_equal(got_s, S) and np.array_equal(got_d, delta), (got_s, S)
        assert all(np.array_equal(ce.read_lookahead_tree(f), maps[f]) for f in range(n))
    rec_got, _ = ce.read_lookahead()
    ce.close()
    assert same(rec_got, rec) and S[0] > 0 and S[3] == 0, "the model's sums: the first frame inherits, nothing follows the last"


def test_controller_is_the_models_plan_with_offsets(P):
    check_controller(P, None)


def test_strength_0_keeps_every_record_and_byte(P):
    """after clips with the tree have run in this process (the kernel is loaded): strength 0 is the clip without the option"""
    w, h, clip, n, R = SHAPES[3]
    c = analysed(w, h, clip, n, R)[0]
    on = encode_twice(P, None, w, h, c, R, (STRENGTH, 2))
    plain = encode_twice(P, None, w, h, c, R, 0)
    assert on[4] != plain[4]
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W, lookahead_search=R, lookahead_tree=(STRENGTH, 2))
    ce.set_lookahead_tree(0)
    ce.upload(c)
    out, sizes, st = ce.encode()
    rec, qp = ce.read_lookahead()
    with pytest.raises(P.H264EError):
        ce.read_lookahead_tree(1)
    assert ce.lookahead_tree_time() == (0.0, 0)
    ce.close()
    assert (out, sizes) == plain[4:] and same(rec, plain[0]) and np.array_equal(qp, plain[3]) and st.spin_relaunches == 0


@pytest.mark.parametrize("g", [g for g in RATES if g["kbps"] == 300 and g["clip"] in ("synth", "pan")], ids=lambda g: "%s_%dkbps" % (g["clip"], g["kbps"]))
def test_bitrate_with_the_tree_stays_within_one_window_of_the_target(P, g):
    """the bound of test_gpu_lookahead_motion.test_bitrate_with_search_stays_within_one_window_of_the_target -- |actual - target| over the
    clip <= one window's budget (8*dfb*W bits) + the reference controller's own absolute deviation for the same clip and target -- at
    CIF x 128, GOP 30, W = 16, search 8, with the tree at strength 4 and the default 16 frames ahead"""
    w, h, n, Wc = g["w"], g["h"], g["frames"], 16
    c = clips.make(g["clip"], w, h, n)
    ce = P.ClipEncoder(w, h, n, gop=g["gop"], qp=30, abr_kbps=g["kbps"], lookahead=Wc, lookahead_search=8, lookahead_tree=4)
    ce.upload(c)
    out, sizes, st = ce.encode()
    _, qp = ce.read_lookahead(costs=False)
    _, delta, base = ce.read_lookahead_tree_sums()
    ce.close()
    dfb = g["kbps"] * 1000 // 8 // 30
    target, actual, ref = 8 * dfb * n, 8 * len(out), 8 * g["bytes"]
    bound = 8 * dfb * Wc + abs(ref - target)
    print("%s %d kbps, search 8, tree 4: target %d bits, actual %d, reference %d, deviation %d, bound %d, base QPs per window %s, offsets of the first window %s, %d launches" %
          (g["clip"], g["kbps"], target, actual, ref, abs(actual - target), bound, base[::Wc].tolist(), delta[:Wc].tolist(), st.rounds))
    assert st.spin_relaunches == 0 and sizes and len(sizes) == n
    assert abs(actual - target) <= bound
