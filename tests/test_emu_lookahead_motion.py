"""CPU: the lookahead's cost pass with a motion search (H264E_clip_set_lookahead_search, enc_lookahead_search.h) in the lane-loop
emulation of the kernels (tests/emu): records and motion fields against the numpy model (tests/lookahead_motion_model.py) on shapes that
take every path of the kernel, bounded rings and re-uploads, what is refused, and the controller fed the searched costs."""
import functools
import os
import subprocess

import numpy as np
import pytest

import clips
import lookahead_model as M
import lookahead_motion_model as ML
import pkg
import scenecut_model

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = pkg.EMU_LIB


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


# 16x16: one block, only (0, 0); 48x32: 3 x 2 blocks, every block at a border; 144x144: 9 x 9, a strip of one block behind a full one;
# 176x144: 11 x 9, w2 = 88 no multiple of 16; 208x160: 13 x 10 with a range whose candidates fill two rounds of lanes but not three
SHAPES = [(16, 16, "noise", 4, 8), (48, 32, "ramp", 5, 8), (144, 144, "synth", 4, 8), (176, 144, "ramp", 5, 8), (208, 160, "scene", 6, 3),
          (352, 288, "pan", 4, 8), (352, 288, "scene", 6, 8)]
IDS = ["%dx%d_%s_r%d" % (s[0], s[1], s[2], s[4]) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def model(w, h, clip, n, R):
    """the clip and the model's records and fields for it, made once for every test (GPU tests included) that asks"""
    c = clips.make(clip, w, h, n)
    c.setflags(write=False)
    rec, fields = ML.analyse(c, w, h, R)
    return c, rec, fields


def same(rec, model_rec):
    return all(np.array_equal(a, b) for a, b in zip(rec, model_rec))


def same_fields(got, want):
    return len(got) == len(want) and all(np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) for g, w in zip(got, want))


def analyse_twice(P, lib, w, h, c, R, frames=None, **kw):
    """records, fields of `frames` (all), QPs, stream and sizes with search R; a second, rewound pass must give all of it again"""
    kw = dict(dict(gop=4, qp=30, abr_kbps=100, lookahead=2, lookahead_search=R), **kw)
    ce = P.ClipEncoder(w, h, len(c), lib=lib, **kw)
    ce.upload(c)
    res = []
    for _ in range(2):
        out, sizes, _ = ce.encode()
        rec, qp = ce.read_lookahead()
        res.append((rec, [ce.read_lookahead_motion(f) for f in (range(len(c)) if frames is None else frames)], qp, out, sizes))
    ce.close()
    a, b = res
    assert same(a[0], b[0]) and same_fields(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:], "a rewound pass gives the same"
    return a


def check_shape(P, lib, w, h, clip, n, R):
    c, rec, fields = model(w, h, clip, n, R)
    got_rec, got_fields, _, _, _ = analyse_twice(P, lib, w, h, c, R)
    assert same(got_rec, rec), (got_rec, rec)
    for f in range(n):
        assert got_fields[f][0].shape == ((h // 2) >> 3, (w // 2) >> 3, 2) and got_fields[f][0].dtype == np.int8 and got_fields[f][1].dtype == np.uint16
        assert np.array_equal(got_fields[f][0], fields[f][0]), "vectors of frame %d" % f
        assert np.array_equal(got_fields[f][1], fields[f][1]), "costs of frame %d" % f
    assert not got_fields[0][0].any() and got_rec[0][0] == got_rec[1][0], "frame 0: inter = intra, no vector"


@pytest.mark.parametrize("w,h,clip,n,R", SHAPES, ids=IDS)
def test_records_and_fields_equal_the_model(w, h, clip, n, R):
    check_shape(pkg.load_pkg(), LIB, w, h, clip, n, R)


def test_the_shapes_take_the_paths_they_are_for():
    _, rec, fields = model(352, 288, "pan", 4, 8)
    assert all((fields[f][0][:, :-1] == (6, 0)).all() and not fields[f][1][:, :-1].any() for f in range(1, 4)), "the pan is found"
    assert int(rec[1][1]) < int(M.costs(model(352, 288, "pan", 4, 8)[0], 352, 288)[1][1]) // 10
    _, _, fields = model(16, 16, "noise", 4, 8)
    assert all(not f[0].any() for f in fields)
    moved = [np.abs(model(*s)[2][1][0]).max() for s in SHAPES[1:]]
    assert all(m > 0 for m in moved), moved
    assert np.abs(model(208, 160, "scene", 6, 3)[2][2][0]).max() <= 3


def test_lane_order_does_not_matter():
    w, h, clip, n, R = SHAPES[3]
    check_shape(pkg.load_pkg(), pkg.EMU_REV_LIB, w, h, clip, n, R)


def test_search_off_is_the_pass_without_search():
    P = pkg.load_pkg()
    w, h, n = 176, 144, 4
    c = clips.make("ramp", w, h, n)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, abr_kbps=100, lookahead=2, lookahead_search=0)
    ce.set_lookahead_search(0)
    ce.upload(c)
    out, _, _ = ce.encode()
    rec, _ = ce.read_lookahead()
    with pytest.raises(P.H264EError) as e:
        ce.read_lookahead_motion(1)
    assert "search is off" in str(e.value)
    ce.close()
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload(c)
    assert ce.encode()[0] == out
    ce.close()
    assert same(rec, M.costs(c, w, h))


def test_bounded_ring_reupload_and_reads_outside_the_ring():
    """a ring of four frames fed three at a time, windows of two; frame 2 is uploaded a second time, with another picture, after it has
    been analysed (with the window in front of it) and before its own window is encoded: records and fields from 2 onward are those of
    the new clip"""
    P = pkg.load_pkg()
    w, h, n, R = 48, 32, 11, 8
    c = clips.make("ramp", w, h, n)
    c2 = c.copy()
    c2[2] = clips.make("noise", w, h, 1)[0]
    rec_m, fields_m = ML.analyse(c2, w, h, R)
    want = analyse_twice(P, LIB, w, h, c2, R)
    assert same(want[0], rec_m) and same_fields(want[1], fields_m)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, resident=4, abr_kbps=100, lookahead=2, lookahead_search=R)
    parts, sizes = [], []
    for f0 in range(0, n, 3):
        ce.upload(c[f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
        if f0 == 0:
            assert len(sizes) == 2 and same_fields([ce.read_lookahead_motion(2)], ML.analyse(c[:3], w, h, R)[1][2:])
            ce.upload(c2[2:3], first=2)
            with pytest.raises(P.H264EError) as e:
                ce.read_lookahead_motion(2)                 # its field is stale
            assert "frames 0..1 have" in str(e.value), str(e.value)
    rec, qp = ce.read_lookahead()
    assert same(rec, rec_m) and np.array_equal(qp, want[2]) and b"".join(parts) == want[3] and sizes == want[4]
    assert same_fields([ce.read_lookahead_motion(f) for f in range(7, n)], fields_m[7:])
    for f in (0, 6, n, -1):
        with pytest.raises(P.H264EError) as e:
            ce.read_lookahead_motion(f)
        assert "frame %d has no motion field" % f in str(e.value) and "frames 7..10 have" in str(e.value), str(e.value)
    ce.close()


def test_refusals_change_nothing():
    P = pkg.load_pkg()
    w, h, n, R = 48, 32, 6, 8
    c = clips.make("ramp", w, h, n)
    want = analyse_twice(P, LIB, w, h, c, R)
    plain = analyse_twice(P, LIB, w, h, c, 0, frames=[])
    assert not same(want[0], plain[0]), "the clip tells the two passes apart"
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, abr_kbps=100, lookahead=2, lookahead_search=R)
    for bad in (9, -1, 289):
        with pytest.raises(P.H264EError) as e:
            ce.set_lookahead_search(bad)
        assert "range %d is outside 0..8" % bad in str(e.value), str(e.value)
    with pytest.raises(P.H264EError):
        ce.read_lookahead_motion(0)                         # nothing has been analysed
    ce.upload(c[:4])
    part = ce.encode(rewind=False)[0]
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead_search(R)
    assert "frame 0" in str(e.value)
    ce.upload(c[4:], first=4)
    assert part + ce.encode(rewind=False)[0] == want[3]
    ce.L.H264E_clip_rewind(ce.c)
    # the records belong to range 8: no other range, not even off; the same range again is no change
    for other in (0, 3):
        with pytest.raises(P.H264EError) as e:
            ce.set_lookahead_search(other)
        assert "range %d after frames have been analysed with range %d" % (other, R) in str(e.value), str(e.value)
    ce.set_lookahead_search(R)
    out, sizes, _ = ce.encode()
    rec, qp = ce.read_lookahead()
    assert (out, sizes) == want[3:] and same(rec, want[0]) and np.array_equal(qp, want[2])
    assert same_fields([ce.read_lookahead_motion(f) for f in range(n)], want[1])
    ce.close()
    # a clip analysed without search stays without
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, abr_kbps=100, lookahead=2)
    ce.upload(c)
    ce.encode()
    ce.L.H264E_clip_rewind(ce.c)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead_search(R)
    assert "range %d after frames have been analysed with range 0" % R in str(e.value)
    out, sizes, _ = ce.encode()
    rec, _ = ce.read_lookahead()
    ce.close()
    assert (out, sizes) == plain[3:] and same(rec, plain[0])
    # GOP shards
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, keep_records=1)
    ce.upload(c)
    shard = ce.encode()[0]
    ce.L.H264E_clip_rewind(ce.c)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead_search(R)
    assert "keep_records" in str(e.value)
    assert ce.encode()[0] == shard
    ce.close()
    with pytest.raises(P.H264EError):
        P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, keep_records=1, lookahead_search=R)


# ---- the controller

CTL = dict(w=176, h=144, n=24, gop=8, W=4, kbps=120, R=8)


@pytest.fixture(scope="module")
def controlled():
    P = pkg.load_pkg()
    w, h, n, gop, W, kbps, R = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R"))
    c = clips.make("synth", w, h, n)
    rec, _, qp, out, sizes = analyse_twice(P, LIB, w, h, c, R, frames=[], gop=gop, abr_kbps=kbps, lookahead=W)
    return dict(P=P, clip=c, out=out, sizes=sizes, rec=rec, qp=qp)


def header_bits(P, lib, w, h, c):
    ce = P.ClipEncoder(w, h, 1, lib=lib, qp=26)
    ce.upload(c[:1])
    out, _, _ = ce.encode()
    ce.close()
    return 40, 40 + 8 * M.parameter_set_bytes(out)


def check_controller(d, lib):
    w, h, n, gop, W, kbps, R = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R"))
    kinds = [int(k) for k in scenecut_model.kinds(n, gop, [])]
    hdr, bits = header_bits(d["P"], lib, w, h, d["clip"]), [8 * s for s in d["sizes"]]
    assert same(d["rec"], ML.costs(d["clip"], w, h, R))
    plan = ML.plan(d["rec"], kinds, hdr, bits, kbps, W)
    assert np.array_equal(d["qp"], plan), (d["qp"], plan)
    assert d["qp"][0] != ML.plan(d["rec"], kinds, hdr, bits, kbps, W, search=0)[0], "the first window shows which K0 was in force"
    ce = d["P"].ClipEncoder(w, h, n, lib=lib, gop=gop, qp=30, qp_schedule=d["qp"])
    ce.upload(d["clip"])
    out, sizes, _ = ce.encode()
    ce.close()
    assert out == d["out"] and sizes == d["sizes"], "the stream is the stream of that QP schedule"


def test_controller_is_the_models_plan_on_searched_costs(controlled):
    check_controller(controlled, LIB)


def test_controller_does_not_depend_on_the_call_pattern(controlled):
    d = controlled
    w, h, n, gop, W, kbps, R = (CTL[k] for k in ("w", "h", "n", "gop", "W", "kbps", "R"))
    ce = d["P"].ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, abr_kbps=kbps, lookahead=W, lookahead_search=R)
    parts, sizes = [], []
    for f0 in range(0, n, 3):
        ce.upload(d["clip"][f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    assert b"".join(parts) == d["out"] and sizes == d["sizes"] and np.array_equal(qp, d["qp"])
