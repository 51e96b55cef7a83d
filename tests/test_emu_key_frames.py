"""CPU: the clip encoder's key-frame schedule (H264E_clip_set_key_frames) and scene-cut detection (H264E_clip_set_scenecut,
enc_scenecut.h) in the lane-loop emulation of the kernels (tests/emu).

  - every case of tests/golden/key_frames.json -- streams of the REFERENCE with H264E_FRAME_TYPE_KEY on a list of frames -- through the
    clip encoder with that list, through H264E_encode frame by frame, and through the oracle: exact bytes and frame sizes;
  - the detector against the numpy model (tests/scenecut_model.py): D(f) and cuts exactly, and the stream of the explicit list that the
    model's cuts make; device input, bounded input rings, re-uploads, rewinds, list and detector together;
  - what is refused is refused and leaves the encoder producing the plain stream;
  - a clip encoder on which neither call is made writes the reference's recorded bytes with the launches it took before;
  - the CLI's --keyframes / --scenecut."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import clips
import ingest_model as IM
import pkg
import run_param_cases as R
import scenecut_model as M
from test_emu_device_input import DevMem

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = json.load(open(os.path.join(HERE, "golden", "key_frames.json")))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
LIB = pkg.EMU_LIB


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def clip_kw(case):
    """ClipEncoder arguments of a golden case"""
    w, h, gop, _vbv, _cinp, den, slices = case["create"]
    c = case["clip"]
    return dict(gop=gop, qp=c["qp"], kbps=c["kbps"], speed=c["speed"], slices=slices if slices > 1 else 0, denoise=bool(den))


def check_case(case, out, sizes, what):
    assert sizes == case["sizes"], "%s: frame sizes %r, the reference %r" % (what, sizes, case["sizes"])
    assert (len(out), hashlib.md5(out).hexdigest()) == (case["bytes"], case["stream_md5"]), "%s: same sizes, other bytes than the reference" % what
    pos = 0
    for i, n in enumerate(sizes):
        assert hashlib.md5(out[pos:pos + n]).hexdigest() == case["md5"][i], "%s: frame %d differs" % (what, i)
        pos += n


def test_fixture_covers_what_it_is_for():
    names = set(CASES)
    assert {"cif_gop30_mid_gop", "qcif_gop8_before_and_on_periodic", "qcif_gop10_two_in_a_row", "qcif_gop1_quirk", "tiny_gop0", "cif_kbps300",
            "qcif_2_slices", "cif_8_slices_kbps400", "qcif_denoise", "strip_640x16", "tiny_cropped_34x18", "cropped_200x120"} <= names
    for name, c in CASES.items():
        n, gop = len(c["frames"]), c["create"][2]
        assert [l[0] for l in c["frames"]] == [M.KEY if t in c["forced"] else M.DEFAULT for t in range(n)], name
        assert c["key"] == [int(k) for k in M.kinds(n, gop, c["forced"])], "%s: the model's schedule is not the reference's" % name
    q = CASES["qcif_gop1_quirk"]
    assert q["key"][3:6] == [1, 1, 0], "gop 1: the frame behind a forced key frame is a P frame in the reference"
    assert sum(CASES["tiny_gop0"]["key"]) == 1 + len(CASES["tiny_gop0"]["forced"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_clip_encoder_with_key_frames_matches_reference(name):
    P = pkg.load_pkg()
    case = CASES[name]
    w, h = case["create"][:2]
    n = len(case["frames"])
    raw, _ = R.pictures(case)
    ce = P.ClipEncoder(w, h, n, lib=LIB, key_frames=case["forced"], **clip_kw(case))
    ce.upload(raw)
    out, sizes, st = ce.encode()
    again, _, _ = ce.encode()                   # a rewind keeps the schedule
    ce.close()
    check_case(case, out, sizes, name)
    assert again == out
    assert st.next_idr_pic_id_state == sum(case["key"]) & 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_per_frame_encoder_and_oracle_match_reference(name):
    P = pkg.load_pkg()
    case = CASES[name]
    R.compare(case, R.replay_product(P, case, lib=LIB), name + " (H264E_encode)")
    R.compare(case, R.replay_oracle(case), name + " (oracle)")


def encode(P, w, h, c, feed=None, **kw):
    ce = P.ClipEncoder(w, h, len(c), lib=LIB, **kw)
    (feed or (lambda e: e.upload(c)))(ce)
    out, sizes, st = ce.encode()
    sc = ce.read_scenecut() if kw.get("scenecut") else None
    ce.close()
    return out, sizes, st, sc


@pytest.mark.parametrize("clip,n", [("scene", 12), ("synth", 8), ("pan", 8), ("noise", 4)])
def test_scenecut_equals_model_and_the_explicit_list_stream(clip, n):
    P = pkg.load_pkg()
    w, h, gop = 352, 288, 30
    c = clips.make(clip, w, h, n)
    dist, is_cut, merged = M.detect(c, w, h, gop)
    out, sizes, st, (d, k) = encode(P, w, h, c, gop=gop, qp=30, scenecut=P.H264E_SCENECUT_DEFAULT)
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut), (d, dist, k, is_cut)
    if clip == "scene":
        assert list(np.flatnonzero(k)) == [n // 2] and dist[n // 2] == 280 and max(np.delete(dist, n // 2)) <= 21
    else:
        assert not k.any()
    want, want_sizes, _, _ = encode(P, w, h, c, gop=gop, qp=30, key_frames=merged)
    assert out == want and sizes == want_sizes
    plain, _, _, _ = encode(P, w, h, c, gop=gop, qp=30)
    assert (out != plain) == bool(is_cut.any())


def _dev_feed(mem, c, w, h, fmt):
    """(feed function, the packed I420 frames the encoder sees) for frames handed over from device memory"""
    if fmt == "i420":
        srcs = [mem.put(f.reshape(h * 3 // 2, w)) for f in c]
        return (lambda e: e.upload_device(srcs, "i420")), c
    if fmt == "nv12":
        pairs = [IM.i420_to_nv12(f, w, h) for f in c]
        srcs = [(mem.put(y, w + 5, 1), mem.put(uv, w + 2, 2)) for y, uv in pairs]
        return (lambda e: e.upload_device(srcs, "nv12")), c
    rgb = IM.rgb_clip(w, h, len(c), 3)
    rgb[len(c) // 2:] = rgb[len(c) // 2:] // 4 + 20           # a hard cut to a dark scene
    srcs = [mem.put(f, w * 3 + 7, 3) for f in rgb]
    return (lambda e: e.upload_device(srcs, "rgb")), np.stack([IM.rgb_to_i420(f) for f in rgb])


@pytest.mark.parametrize("fmt", ["i420", "nv12", "rgb"])
def test_scenecut_on_device_input(fmt):
    P = pkg.load_pkg()
    w, h, n, gop = 176, 144, 8, 30
    mem = DevMem(LIB)
    try:
        feed, model = _dev_feed(mem, clips.make("scene", w, h, n), w, h, fmt)
        dist, is_cut, merged = M.detect(model, w, h, gop)
        assert is_cut.any()
        out, _, _, (d, k) = encode(P, w, h, model, feed=feed, gop=gop, qp=30, scenecut=128)
        assert np.array_equal(d, dist) and np.array_equal(k, is_cut)
        want, _, _, _ = encode(P, w, h, model, gop=gop, qp=30, key_frames=merged)
        assert out == want
    finally:
        mem.close()


@pytest.mark.parametrize("kw", [dict(), dict(kbps=200), dict(denoise=True), dict(slices=2)], ids=["cqp", "kbps", "denoise", "slices"])
def test_scenecut_with_a_bounded_ring_and_several_encode_calls(kw):
    """frames arrive three at a time in a ring of four: cuts are decided launch by launch, from histograms of frames whose pictures have
    left the ring (one record per frame), and under rate control the kind of a frame that has not arrived yet is not guessed"""
    P = pkg.load_pkg()
    w, h, n, gop = 176, 144, 14, 5
    c = np.concatenate([clips.make("scene", w, h, 8), clips.make("synth", w, h, 6)])      # cuts at 4 and 8; 5 and 10 are periodic
    dist, is_cut, merged = M.detect(c, w, h, gop)
    assert list(np.flatnonzero(is_cut)) == [4, 8]
    want, want_sizes, _, _ = encode(P, w, h, c, gop=gop, qp=30, key_frames=merged, **kw)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, resident=4, scenecut=128, **kw)
    parts, sizes = [], []
    for f0 in range(0, n, 3):
        ce.upload(c[f0:f0 + 3], first=f0)
        out, s, _ = ce.encode(rewind=False)
        parts.append(out)
        sizes += s
    d, k = ce.read_scenecut()
    ce.close()
    assert np.array_equal(d, dist) and np.array_equal(k, is_cut)
    assert b"".join(parts) == want and sizes == want_sizes


def test_reupload_changes_the_cuts_and_rewind_reproduces_the_bytes():
    P = pkg.load_pkg()
    w, h, n, gop = 176, 144, 10, 30
    c = clips.make("scene", w, h, n)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, scenecut=128)
    ce.upload(c)
    first, _, _ = ce.encode()
    d1, k1 = ce.read_scenecut()
    again, _, _ = ce.encode()                   # rewound: the records are kept
    assert again == first and list(np.flatnonzero(k1)) == [n // 2]
    c2 = c.copy()
    c2[3:] = clips.make("synth", w, h, n)[3:]   # another cut, at frame 3, and none at n // 2
    ce.upload(c2[3:], first=3)
    changed, _, _ = ce.encode()
    d2, k2 = ce.read_scenecut()
    ce.close()
    dist, is_cut, merged = M.detect(c2, w, h, gop)
    assert np.array_equal(d2, dist) and np.array_equal(k2, is_cut) and list(np.flatnonzero(k2)) == [3]
    assert np.array_equal(d2[:3], d1[:3])
    want, _, _, _ = encode(P, w, h, c2, gop=gop, qp=30, key_frames=merged)
    assert changed == want and changed != first


def test_explicit_list_and_detector_together():
    """a listed frame is left alone by the detector (is_cut 0), a cut right behind a listed frame is still a cut; threshold 0 = off"""
    P = pkg.load_pkg()
    w, h, n, gop = 176, 144, 12, 30
    c = clips.make("scene", w, h, n)
    for forced in ([6], [2, 5], [5, 7]):
        dist, is_cut, merged = M.detect(c, w, h, gop, forced=forced)
        out, _, _, (d, k) = encode(P, w, h, c, gop=gop, qp=30, key_frames=forced, scenecut=128)
        assert np.array_equal(d, dist) and np.array_equal(k, is_cut)
        assert bool(k[6]) == (6 not in forced)
        want, _, _, _ = encode(P, w, h, c, gop=gop, qp=30, key_frames=merged)
        assert out == want
    # a low threshold: every frame whose D exceeds it, except those that are key frames already (gop 4)
    dist, is_cut, merged = M.detect(c, w, h, 4, threshold=10)
    assert is_cut.sum() > 2
    out, _, _, (d, k) = encode(P, w, h, c, gop=4, qp=30, scenecut=10)
    want, _, _, _ = encode(P, w, h, c, gop=4, qp=30, key_frames=merged)
    assert np.array_equal(k, is_cut) and out == want
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=gop, qp=30, scenecut=128)
    ce.set_scenecut(0)
    ce.upload(c)
    off, _, _ = ce.encode()
    ce.close()
    assert off == encode(P, w, h, c, gop=gop, qp=30)[0]


def test_refusals_leave_the_encoder_usable():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 6
    c = clips.make("synth", w, h, n)
    plain, _, _, _ = encode(P, w, h, c, gop=4, qp=30)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30)
    ce.upload(c)

    def still_plain():
        out, _, _ = ce.encode()
        assert out == plain

    for bad in ([n], [-1], [3, 2], [2, 2]):                     # outside the clip, not ascending
        with pytest.raises(P.H264EError):
            ce.set_key_frames(bad)
        assert ce.L.H264E_last_error()
        still_plain()
    with pytest.raises(P.H264EError):
        ce.set_scenecut(-1)
    with pytest.raises(P.H264EError):
        ce.read_scenecut()                                      # the detector was never on
    still_plain()
    ce.close()
    # not at frame 0
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30)
    ce.upload(c[:3])
    part1, _, _ = ce.encode(rewind=False)
    for call in (lambda: ce.set_key_frames([4]), lambda: ce.set_scenecut(128)):
        with pytest.raises(P.H264EError):
            call()
    ce.upload(c[3:], first=3)
    part2, _, _ = ce.encode(rewind=False)
    assert part1 + part2 == plain
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_key_frames([4])                                      # rewound: allowed
    ce.set_key_frames([])                                       # ... and cleared again
    assert ce.encode()[0] == plain
    ce.close()
    # keep_records (GOP shards)
    ce = P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, keep_records=1)
    ce.upload(c)
    for call in (lambda: ce.set_key_frames([2]), lambda: ce.set_scenecut(128)):
        with pytest.raises(P.H264EError):
            call()
    assert ce.encode()[0] == plain
    ce.close()
    with pytest.raises(P.H264EError):
        P.ClipEncoder(w, h, n, lib=LIB, gop=4, qp=30, key_frames=[n + 3])


def test_without_the_new_calls_nothing_changes():
    """bytes from the reference's recorded stream (tests/golden/golden.json); launches and rounds as recorded on the commit before this
    feature (one launch, one round, no relaunch for 8 CIF frames in the emulation)"""
    P = pkg.load_pkg()
    g = next(x for x in GOLDEN if (x["clip"], x["w"], x["frames"], x["flags"]) == ("synth", 352, 8, "--qp 26 --gop 30"))
    c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], lib=LIB, gop=30, qp=26)
    ce.upload(c)
    out, sizes, st = ce.encode(profile=True)
    ce.close()
    assert sizes == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"]
    assert (st.kernel_launches, st.rounds, st.reencoded_gops, st.frames, st.next_idr_pic_id_state) == (1, 1, 0, 8, 1)


def _app(tmp_path, c, w, h, args, name="o.264"):
    yuv = tmp_path / ("kf_%dx%d.yuv" % (w, h))
    c.tofile(yuv)
    out = tmp_path / name
    r = subprocess.run([APP, "--input", str(yuv), "--output", str(out), "--stats", "x"] + args, capture_output=True, text=True, timeout=600)
    return r, (out.read_bytes() if out.exists() else b"")


@pytest.mark.parametrize("name", ["qcif_gop10_two_in_a_row", "qcif_gop1_quirk", "qcif_2_slices", "qcif_kbps150_gop0"])
def test_cli_keyframes_matches_reference(tmp_path, name):
    case = CASES[name]
    w, h, gop, _vbv, _cinp, _den, slices = case["create"]
    raw, _ = R.pictures(case)
    k = case["clip"]
    args = ["--gop", str(gop), "--keyframes", ",".join(str(f) for f in case["forced"])] + (["--kbps", str(k["kbps"])] if k["kbps"] else ["--qp", str(k["qp"])])
    if slices > 1:
        args += ["--threads", str(slices)]
    r, out = _app(tmp_path, raw, w, h, args)
    assert r.returncode == 0, r.stdout + r.stderr
    sizes = [int(l.split("bytes=")[1]) for l in r.stdout.splitlines() if l.startswith("frame=")]
    check_case(case, out, sizes, name)
    assert "scene cuts" not in r.stdout


def test_cli_scenecut_and_refusals(tmp_path):
    P = pkg.load_pkg()
    w, h, n = 176, 144, 10
    c = clips.make("scene", w, h, n)
    dist, is_cut, merged = M.detect(c, w, h, 30)
    want, _, _, _ = encode(P, w, h, c, gop=30, qp=30, key_frames=merged)
    plain, _, _, _ = encode(P, w, h, c, gop=30, qp=30)
    base = ["--gop", "30", "--qp", "30"]
    for value in ("x", "128"):
        r, out = _app(tmp_path, c, w, h, base + ["--scenecut", value])
        assert r.returncode == 0 and out == want, r.stdout + r.stderr
        assert [l for l in r.stdout.splitlines() if l.startswith("scene cuts")] == ["scene cuts: %d" % (n // 2)]
    r, out = _app(tmp_path, c, w, h, base + ["--scenecut", "900"])
    assert r.returncode == 0 and out == plain and "scene cuts: none" in r.stdout.splitlines()
    r, out = _app(tmp_path, c, w, h, base)
    assert r.returncode == 0 and out == plain and "scene cuts" not in r.stdout
    for extra in (["--gpus", "2"], ["--clip", "0"]):
        for opt in (["--scenecut", "x"], ["--keyframes", "3"]):
            r, _ = _app(tmp_path, c, w, h, base + opt + extra, name="refused.264")
            assert r.returncode == 1 and "ERROR" in r.stdout, (extra, opt, r.stdout)
    for bad in ("3,2", "99", "a,b"):
        r, _ = _app(tmp_path, c, w, h, base + ["--keyframes", bad], name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout
