"""CPU: the lookahead's cost tree (H264E_clip_set_lookahead_tree, enc_lookahead_tree.h) in the lane-loop emulation of the kernels
(tests/emu): block maps, sums, offsets, base QPs and the plan against the numpy model (tests/lookahead_tree_model.py) on shapes that take
every path of the kernel, with the tree cut at the window's end and two frames behind it; strength 0, bounded rings, a re-upload, and
what is refused."""
import functools
import os
import subprocess

import numpy as np
import pytest

import clips
import lookahead_tree_model as MT
import pkg
import scenecut_model
from test_emu_lookahead_motion import header_bits, same

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = pkg.EMU_LIB


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


# 16x16: one block, which nothing reaches; 48x32: 3 x 2 blocks, every block at a border; 144x144: 9 x 9, a wave of one block behind ten
# full ones; 176x144: 11 x 9 = 99 blocks, the last wave holds three; 208x160: range 3; 352x288: a pan of 6 samples, two targets per block;
# still: everything is inherited.  GOP 4 and windows of 3: frame 4 is a key frame inside window [3, 6) and, with ahead 2, behind window [0, 3)
SHAPES = [(16, 16, "noise", 5, 8), (48, 32, "ramp", 6, 8), (144, 144, "synth", 5, 8), (176, 144, "ramp", 6, 8), (208, 160, "scene", 6, 3),
          (352, 288, "pan", 5, 8), (176, 144, "still", 6, 8)]
IDS = ["%dx%d_%s_r%d" % (s[0], s[1], s[2], s[4]) for s in SHAPES]
AHEADS = (0, 2)
GOP, W, STRENGTH, KBPS = 4, 3, 4, 100


@functools.lru_cache(maxsize=None)
def analysed(w, h, clip, n, R):
    """the clip and the model's records, fields and intra costs, made once for every test (GPU tests included) that asks"""
    c = clips.make(clip, w, h, n)
    c.setflags(write=False)
    return (c,) + MT.analyse(c, w, h, R)


@functools.lru_cache(maxsize=None)
def model(w, h, clip, n, R, ahead, gop=GOP, window=W, strength=STRENGTH):
    """(clip, records, kinds, maps, S, delta) of the model"""
    c, rec, fields, intra = analysed(w, h, clip, n, R)
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    return (c, rec, kinds) + MT.windows(rec, fields, intra, kinds, window, strength, ahead)


def encode_twice(P, lib, w, h, c, R, tree, maps=True, **kw):
    """records, block maps (all frames), (S, delta, base), QPs, stream and sizes; a second, rewound pass must give all of it again"""
    kw = dict(dict(gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W, lookahead_search=R, lookahead_tree=tree), **kw)
    ce = P.ClipEncoder(w, h, len(c), lib=lib, **kw)
    ce.upload(c)
    res = []
    for _ in range(2):
        out, sizes, _ = ce.encode()
        rec, qp = ce.read_lookahead()
        res.append((rec, [ce.read_lookahead_tree(f) for f in range(len(c))] if maps and tree else [], ce.read_lookahead_tree_sums() if tree else None, qp, out, sizes))
    ce.close()
    a, b = res
    assert same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and np.array_equal(a[3], b[3]) and a[4:] == b[4:], "a rewound pass gives the same"
    assert a[2] is None or all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    return a


def check_plan(P, lib, w, h, c, rec, kinds, deltas, got, kbps=KBPS, window=W, gop=GOP):
    """the QPs are the model's plan on the model's offsets, and the stream is the stream of that QP schedule"""
    _, _, (_, _, base), qp, out, sizes = got
    want_qp, want_base = MT.plan(rec, kinds, header_bits(P, lib, w, h, c), [8 * s for s in sizes], kbps, window, deltas)
    assert np.array_equal(qp, want_qp) and np.array_equal(base, want_base), (qp, want_qp, base, want_base)
    ce = P.ClipEncoder(w, h, len(c), lib=lib, gop=gop, qp=30, qp_schedule=qp)
    ce.upload(c)
    out2, sizes2, _ = ce.encode()
    ce.close()
    assert out2 == out and sizes2 == sizes, "the stream is the stream of that QP schedule"


def check_shape(P, lib, w, h, clip, n, R, ahead, plan=True):
    c, rec, kinds, maps, S, delta = model(w, h, clip, n, R, ahead)
    got = encode_twice(P, lib, w, h, c, R, (STRENGTH, ahead))
    assert same(got[0], rec)
    for f in range(n):
        assert got[1][f].shape == ((h // 2) >> 3, (w // 2) >> 3) and got[1][f].dtype == np.uint64
        assert np.array_equal(got[1][f], maps[f]), "block map of frame %d" % f
    assert np.array_equal(got[2][0], S) and np.array_equal(got[2][1], delta), (got[2], S, delta)
    if plan:
        check_plan(P, lib, w, h, c, rec, kinds, delta, got)


@pytest.mark.parametrize("ahead", AHEADS)
@pytest.mark.parametrize("w,h,clip,n,R", SHAPES, ids=IDS)
def test_maps_sums_offsets_and_plan_equal_the_model(w, h, clip, n, R, ahead):
    check_shape(pkg.load_pkg(), LIB, w, h, clip, n, R, ahead)


@pytest.mark.parametrize("ahead", AHEADS)
def test_lane_order_does_not_matter(ahead):
    check_shape(pkg.load_pkg(), pkg.EMU_REV_LIB, *SHAPES[3], ahead)
    check_shape(pkg.load_pkg(), pkg.EMU_REV_LIB, *SHAPES[5], ahead, plan=False)


# ---- a controller whose QPs are not at the end of the range, so the offsets show

CTL = dict(w=176, h=144, n=24, gop=8, W=4, kbps=120, R=8, tree=(8, 2))


def check_controller(P, lib):
    w, h, n, gop, Wc, kbps, R, tree = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R", "tree"))
    c, rec, kinds, _, S, delta = model(w, h, "synth", n, R, tree[1], gop, Wc, tree[0])
    got = encode_twice(P, lib, w, h, c, R, tree, maps=False, gop=gop, abr_kbps=kbps, lookahead=Wc)
    assert np.array_equal(got[2][0], S) and np.array_equal(got[2][1], delta)
    assert delta.min() < 0 and len(set((got[3].astype(int) - got[2][2]).tolist())) > 1, "frames of one window get different QPs"
    assert got[3].min() > 10 and got[3].max() < 50, "no QP at the end of the range"
    check_plan(P, lib, w, h, c, rec, kinds, delta, got, kbps, Wc, gop)
    return c, got


@pytest.fixture(scope="module")
def controlled():
    return check_controller(pkg.load_pkg(), LIB)


def test_controller_is_the_models_plan_with_offsets(controlled):
    pass


def test_controller_does_not_depend_on_the_call_pattern(controlled):
    """uploads of 3 frames at a time into a ring of 8: a window starts only when the frames up to its horizon are there"""
    c, want = controlled
    P = pkg.load_pkg()
    w, h, n, gop, Wc, kbps, R, tree = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R", "tree"))
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, resident=8, abr_kbps=kbps, lookahead=Wc, lookahead_search=R, lookahead_tree=tree)
    parts, sizes, progress = [], [], []
    for f0 in range(0, n, 3):
        ce.upload(c[f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
        progress.append(len(sizes))
    assert progress[:3] == [0, 4, 4], "window [0, 4) waits for frame 5, window [4, 8) for frame 9"
    S, delta, base = ce.read_lookahead_tree_sums()
    _, qp = ce.read_lookahead(costs=False)
    # the maps of the last 8 - 2 frames are still in the ring (the last run had no frames ahead), frames in front of them are named
    assert np.array_equal(ce.read_lookahead_tree(n - 1), np.zeros_like(ce.read_lookahead_tree(n - 1)))
    with pytest.raises(P.H264EError) as e:
        ce.read_lookahead_tree(n - 9)
    assert "frame %d has no block map" % (n - 9) in str(e.value) and "frames %d..%d have" % (n - 8, n - 1) in str(e.value), str(e.value)
    ce.close()
    assert b"".join(parts) == want[4] and sizes == want[5] and np.array_equal(qp, want[3])
    assert np.array_equal(S, want[2][0]) and np.array_equal(delta, want[2][1]) and np.array_equal(base, want[2][2])


def test_reupload_before_the_window_is_planned_takes_effect():
    P = pkg.load_pkg()
    w, h, n, R, ahead = 48, 32, 6, 8, 2
    c = clips.make("ramp", w, h, n)
    c2 = c.copy()
    c2[2] = clips.make("noise", w, h, 1)[0]
    want = encode_twice(P, LIB, w, h, c2, R, (STRENGTH, ahead))
    assert not np.array_equal(want[2][0], encode_twice(P, LIB, w, h, c, R, (STRENGTH, ahead))[2][0]), "the new picture changes the sums"
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W, lookahead_search=R, lookahead_tree=(STRENGTH, ahead))
    ce.upload(c[:4])
    assert ce.encode(rewind=False)[1] == [], "window [0, 3) waits for frame 4"
    with pytest.raises(P.H264EError) as e:
        ce.read_lookahead_tree(0)
    assert "no frame has" in str(e.value)
    ce.upload(c2[2:3], first=2)
    ce.upload(c[4:], first=4)
    out, sizes, _ = ce.encode(rewind=False)
    got = ce.read_lookahead_tree_sums()
    maps = [ce.read_lookahead_tree(f) for f in range(n)]
    ce.close()
    assert (out, sizes) == want[4:] and all(np.array_equal(x, y) for x, y in zip(got, want[2])) and all(np.array_equal(x, y) for x, y in zip(maps, want[1]))


def test_strength_0_is_the_clip_without_the_option():
    P = pkg.load_pkg()
    w, h, clip, n, R = SHAPES[3]
    c = analysed(w, h, clip, n, R)[0]
    plain = encode_twice(P, LIB, w, h, c, R, 0)
    assert encode_twice(P, LIB, w, h, c, R, (STRENGTH, 2))[4] != plain[4], "the clip tells the tree from no tree"
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W, lookahead_search=R, lookahead_tree=(STRENGTH, 2))
    ce.set_lookahead_tree(0, 0)
    ce.upload(c)
    out, sizes, _ = ce.encode()
    rec, qp = ce.read_lookahead()
    for call in (lambda: ce.read_lookahead_tree(1), ce.read_lookahead_tree_sums):
        with pytest.raises(P.H264EError) as e:
            call()
        assert "the cost tree is off" in str(e.value)
    assert ce.lookahead_tree_time() == (0.0, 0)
    ce.close()
    assert (out, sizes) == plain[4:] and same(rec, plain[0]) and np.array_equal(qp, plain[3])


def test_refusals_change_nothing():
    P = pkg.load_pkg()
    w, h, n, R = 48, 32, 6, 8
    c = clips.make("ramp", w, h, n)
    want = encode_twice(P, LIB, w, h, c, R, (STRENGTH, 2))
    kw = dict(lib=LIB, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W, lookahead_search=R)

    def refused(ce, args, text):
        with pytest.raises(P.H264EError) as e:
            ce.set_lookahead_tree(*args)
        assert text in str(e.value), str(e.value)

    ce = P.ClipEncoder(w, h, n, lookahead_tree=(STRENGTH, 2), **kw)
    for bad in (17, -1, 400):
        refused(ce, (bad, 2), "strength %d is outside 0..16" % bad)
    refused(ce, (STRENGTH, 256), "ahead 256 is outside 0..255")
    for call, text in ((lambda: ce.set_lookahead(0), "kbps 0 while the cost tree (strength %d)" % STRENGTH),
                       (lambda: ce.set_lookahead_search(0), "range 0 while the cost tree (strength %d)" % STRENGTH)):
        with pytest.raises(P.H264EError) as e:
            call()
        assert text in str(e.value), str(e.value)
    ce.upload(c[:5])
    part = ce.encode(rewind=False)[0]
    refused(ce, (STRENGTH, 2), "not at frame 3")
    refused(ce, (0, 0), "not at frame 3")
    with pytest.raises(P.H264EError) as e:
        ce.read_lookahead_tree(3)
    assert "frame 3 has no block map" in str(e.value) and "frames 0..2 have" in str(e.value), str(e.value)
    assert ce.L.H264E_clip_read_lookahead_tree_sums(ce.c, 0, 4, None, None, None) == -1
    assert b"the windows of frames 0..3 have not been planned (3 frames have)" in ce.L.H264E_last_error()
    ce.upload(c[5:], first=5)
    assert part + ce.encode(rewind=False)[0] == want[4]
    ce.L.H264E_clip_rewind(ce.c)
    out, sizes, _ = ce.encode()
    assert (out, sizes) == want[4:] and all(np.array_equal(x, y) for x, y in zip(ce.read_lookahead_tree_sums(), want[2])), "the setting is kept across a rewind"
    ce.close()
    # the controller off, the search off
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=GOP, qp=30)
    refused(ce, (STRENGTH, 2), "the lookahead controller is off")
    ce.set_lookahead_tree(0, 0)
    ce.close()
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=GOP, qp=30, abr_kbps=KBPS, lookahead=W)
    refused(ce, (STRENGTH, 2), "lookahead search range 0")
    ce.close()
    # GOP shards (the controller itself refuses them: the tree names them first)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=GOP, qp=30, keep_records=1)
    refused(ce, (STRENGTH, 2), "keep_records")
    ce.close()
    # a bounded input ring: W + ahead frames must fit; the default takes what is left
    ce = P.ClipEncoder(w, h, n, resident=4, **kw)
    refused(ce, (STRENGTH, 2), "a window of 3 frames and 2 ahead do not fit the input ring (4 resident frames)")
    ce.set_lookahead_tree(STRENGTH)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead(KBPS, 4)
    assert "a window of 4 frames and the cost tree's 1 ahead do not fit the input ring (4 resident frames)" in str(e.value), str(e.value)
    ce.close()
    with pytest.raises(P.H264EError):
        P.ClipEncoder(w, h, n, lookahead_tree=17, **kw)
