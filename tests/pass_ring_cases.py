"""The bookkeeping that the frame passes share -- scene-cut detection, the lookahead's cost pass with its motion search, the plain and
the motion-compensated denoiser ("Frame passes") -- as cases for the emulation test (tests/test_emu_pass_rings.py) and the
GPU test (tests/test_gpu_pass_rings.py): every check takes the package and the library to load (None = the product library on the
GPU).  Nothing here knows what a pass computes; a clip whose rings wrap is compared with one whose rings never do.

Every case is a 48x32 picture (3 x 2 cost blocks, so rows and columns of the block grid cannot be mixed up), 7 frames, speed 0 and a
constant QP; the one exception is the refusal "would be analysed again", which needs the lookahead controller, because with the
motion-compensated denoiser the denoiser's own refusal comes first."""
import functools

import numpy as np
import pytest

import clips
import synth
from scenecut_model import SCENECUT_DEFAULT

W, H, N = 48, 32, 7
KW = dict(gop=30, qp=26, speed=0)
RANGE = 4                       # the cost pass' search range
CHUNKS = (2, 3, 2)              # frames per upload + encode; on a ring of 3 the second call's passes cover slots and entries 2, 0, 1
CUT = 4                         # the clip changes its content here: the detector has a cut to find
SYNTH_T0 = 40                   # the synth_v1 frame that generate_synth puts in a frame's place

# the passes of a case, as constructor arguments; "motion" runs the cost pass (for its field alone), "plain" has none
PASSES = {
    "motion": dict(KW, scenecut=SCENECUT_DEFAULT, lookahead_search=RANGE, denoise_motion=1),
    "plain": dict(KW, scenecut=SCENECUT_DEFAULT, denoise=True),
}
WRAPS = [("motion", 3, CHUNKS), ("plain", 3, CHUNKS), ("plain", 1, (1,) * N)]          # resident 1: the denoiser's ping-pong
WRAP_IDS = ["%s_resident%d" % (w[0], w[1]) for w in WRAPS]


@functools.lru_cache(maxsize=None)
def source():
    c = clips.make("ramp", W, H, N).copy()
    c[CUT:] = clips.make("noise", W, H, N)[CUT:]
    c.setflags(write=False)
    return c


def feed(P, lib, c, chunks, **kw):
    """the clip fed and encoded chunk by chunk: (the open encoder, stream, frame sizes)"""
    ce = P.ClipEncoder(W, H, len(c), lib=lib, **kw)
    parts, sizes, f0 = [], [], 0
    for k in chunks:
        ce.upload(c[f0:f0 + k], first=f0)
        out, s, st = ce.encode(rewind=False)
        assert st.spin_relaunches == 0
        parts.append(out)
        sizes += s
        f0 += k
    assert f0 == len(c) and len(sizes) == len(c)
    return ce, b"".join(parts), sizes


def window(entries, chunks):
    """[lo, hi): the frames whose ring entries are intact after the passes ran chunk by chunk, each call over [a, limit): what was
    intact in front of a still is, from limit - entries on"""
    lo = a = 0
    for k in chunks:
        lo = max(min(lo, a), a + k - entries)
        a += k
    return lo, a


def same_cells(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def check_wrap(P, lib, name, resident, chunks):
    """a ring of `resident` frames against a fully resident clip fed in the same chunks: streams, distances and cuts, cost records, and
    every picture, field and vector cell that both still hold"""
    kw, costs = PASSES[name], name == "motion"
    c = source()
    ring, out, sizes = feed(P, lib, c, chunks, resident=resident, **kw)
    full, want, want_sizes = feed(P, lib, c, chunks, **kw)
    try:
        assert (out, sizes) == (want, want_sizes)
        d, cut = ring.read_scenecut()
        wd, wcut = full.read_scenecut()
        assert len(d) == N and np.array_equal(d, wd) and np.array_equal(cut, wcut)
        assert wcut[CUT] and wcut.sum() == 1, "the clip has its cut"
        if costs:
            rec, wrec = ring.read_lookahead(qp=False)[0], full.read_lookahead(qp=False)[0]
            assert all(len(r) == N and np.array_equal(r, w) for r, w in zip(rec, wrec))
            assert int(wrec[2].sum()) > 0 and any(int(p) < int(i) for i, p in zip(wrec[0], wrec[1])), "the cost pass measured something"
        lo, hi = window(resident, chunks)
        assert (lo, hi) == (N - resident, N)
        for f in range(lo, hi):
            assert np.array_equal(ring.read_denoised(f), full.read_denoised(f)), "read_denoised(%d)" % f
        assert not np.array_equal(full.read_denoised(N - 1), c[N - 1]), "the denoiser filters"
        if costs:
            lo, hi = window(max(resident, 2), chunks)
            for f in range(lo, hi):
                assert same_cells(ring.read_lookahead_motion(f), full.read_lookahead_motion(f)), "read_lookahead_motion(%d)" % f
                assert same_cells(ring.read_denoise_motion(f), full.read_denoise_motion(f)), "read_denoise_motion(%d)" % f
            assert full.read_lookahead_motion(1)[0].shape == ((H // 2) >> 3, (W // 2) >> 3, 2)
            assert any(full.read_lookahead_motion(f)[0].any() for f in range(1, N)), "the search found motion"
    finally:
        ring.close()
        full.close()


def check_windows(P, lib, name, resident, chunks):
    """after the ring's run the readers succeed exactly for the frames whose entries are on the device, and say which those are"""
    kw, costs = PASSES[name], name == "motion"
    ring, _, _ = feed(P, lib, source(), chunks, resident=resident, **kw)
    readers = [(ring.read_denoised, "denoised picture", resident)]
    if costs:
        readers += [(ring.read_denoise_motion, "vectors", resident), (ring.read_lookahead_motion, "motion field", max(resident, 2))]
    try:
        for read, what, entries in readers:
            lo, hi = window(entries, chunks)
            assert 0 < lo < hi == N
            for f in range(-1, N + 1):
                if lo <= f < hi:
                    read(f)
                    continue
                with pytest.raises(P.H264EError) as e:
                    read(f)
                assert "frame %d has no %s on the device" % (f, what) in str(e.value) and "frames %d..%d have" % (lo, hi - 1) in str(e.value), str(e.value)
    finally:
        ring.close()


def put_upload(ce, f, picture):
    ce.upload(picture[None], first=f)


def put_device(ce, f, picture):
    """from device memory: a packed I420 frame as an explicit (pointer, row stride)"""
    picture = np.ascontiguousarray(picture, np.uint8)
    p = ce.L.H264E_dev_malloc(0, picture.size)
    assert p
    try:
        assert ce.L.H264E_dev_memcpy(p, picture.ctypes.data, picture.size, 1) == 0
        ce.upload_device([(p, W)], "i420", first=f)
    finally:
        ce.L.H264E_dev_free(p)


def put_synth(ce, f, picture):
    assert np.array_equal(picture, synth.frame(W, H, SYNTH_T0))
    ce.generate_synth(f, 1, t0=SYNTH_T0)


PRODUCERS = {"upload": put_upload, "upload_device": put_device, "generate_synth": put_synth}


def check_stale(P, lib, put):
    """all three passes on, the whole clip resident and encoded; frame 4 replaced through put(ce, frame, picture): the next pass over
    the clip is the stream, and leaves the records, of a fresh clip that had the new frame from the start"""
    kw = PASSES["motion"]
    c = source()
    c2 = c.copy()
    c2[4] = synth.frame(W, H, SYNTH_T0)
    assert not np.array_equal(c2[4], c[4])
    fresh, want, want_sizes = feed(P, lib, c2, (N,), **kw)
    ce, first, _ = feed(P, lib, c, (N,), **kw)
    try:
        assert first != want, "the new frame changes the stream"
        put(ce, 4, c2[4])
        out, sizes, st = ce.encode()
        assert (out, sizes) == (want, want_sizes) and st.spin_relaunches == 0
        assert all(np.array_equal(a, b) for a, b in zip(ce.read_scenecut(), fresh.read_scenecut()))
        assert all(np.array_equal(a, b) for a, b in zip(ce.read_lookahead(qp=False)[0], fresh.read_lookahead(qp=False)[0]))
        for f in range(N):
            assert np.array_equal(ce.read_denoised(f), fresh.read_denoised(f)), "read_denoised(%d)" % f
            assert same_cells(ce.read_lookahead_motion(f), fresh.read_lookahead_motion(f)), "read_lookahead_motion(%d)" % f
            assert same_cells(ce.read_denoise_motion(f), fresh.read_denoise_motion(f)), "read_denoise_motion(%d)" % f
    finally:
        ce.close()
        fresh.close()


# ---- refusals (emulation only: nothing here launches a kernel that the cases above have not)

DENOISED_AGAIN = "frame 3 would be denoised again, but the denoised picture in front of it has left the input ring"
ANALYSED_AGAIN = "frame 3 would be analysed again, but the half-resolution picture in front of it has left the ring"
CONTROLLER = dict(KW, abr_kbps=100, lookahead=2)         # the cost pass without a denoiser in front of its refusal


def refused(P, call, *texts):
    with pytest.raises(P.H264EError) as e:
        call()
    assert all(t in str(e.value) for t in texts), str(e.value)


def encoded_ring(P, lib, **kw):
    """all 7 frames through a ring of 3: (the open encoder, its stream)"""
    ce, out, sizes = feed(P, lib, source(), CHUNKS, resident=3, **kw)
    return ce, (out, sizes)


def check_predecessor_has_left(P, lib, put):
    """frame 3 again after the ring has moved on to 4..6: the pass would start from a picture that is gone.  Refused, and the clip is
    what it was: from frame 0 it gives its stream again."""
    c = source()
    for kw, text in ((PASSES["plain"], DENOISED_AGAIN), (PASSES["motion"], DENOISED_AGAIN), (CONTROLLER, ANALYSED_AGAIN)):
        ce, want = encoded_ring(P, lib, **kw)
        try:
            refused(P, lambda: put(ce, 3, c[3]), text, "rewind and upload from frame 0")
            ce.L.H264E_clip_rewind(ce.c)
            ce.restart(0, (0, 0))                           # a ring: no frame counts as uploaded any more
            parts, sizes, f0 = [], [], 0
            for k in CHUNKS:
                ce.upload(c[f0:f0 + k], first=f0)
                out, s, _ = ce.encode(rewind=False)
                parts.append(out)
                sizes += s
                f0 += k
            assert (b"".join(parts), sizes) == want
        finally:
            ce.close()


def check_ring_full(P, lib, put_range):
    """put_range(ce, first, n) puts n frames in"""
    ce = P.ClipEncoder(W, H, N, lib=lib, resident=3, **KW)
    try:
        refused(P, lambda: put_range(ce, 0, 4), "input ring full", "frames 0.. are not encoded yet")
        put_range(ce, 0, 3)
        refused(P, lambda: put_range(ce, 3, 1), "input ring full", "frames 0.. are not encoded yet")
        assert len(ce.encode(rewind=False)[1]) == 3
        put_range(ce, 3, 3)
        refused(P, lambda: put_range(ce, 6, 1), "input ring full", "frames 3.. are not encoded yet")
    finally:
        ce.close()


def check_do_not_fit(P, lib):
    """Reachable: an upload is checked against the frames not encoded yet only at its upper end, so frame 1 may be put again (over the
    slot of frame 4) while frames 3.. wait; the pass then has more frames to make than the input ring holds, and says so."""
    c = source()
    for kw, word, last in ((dict(KW, scenecut=SCENECUT_DEFAULT), "scenecut", 5), (dict(KW, denoise=True), "denoise", 5)):
        ce = P.ClipEncoder(W, H, N, lib=lib, resident=3, **kw)
        try:
            ce.upload(c[0:3])
            assert len(ce.encode(rewind=False)[1]) == 3
            ce.upload(c[3:6], first=3)
            ce.upload(c[1:2], first=1)
            refused(P, lambda: ce.encode(rewind=False), "%s: frames 1..%d do not fit the input ring" % (word, last))
        finally:
            ce.close()
    # the controller plans window 1 (frames 2, 3) once frames 3 and 4 are there; frames 0 and 1 are encoded, 0..2 analysed
    ce = P.ClipEncoder(W, H, N, lib=lib, resident=3, **CONTROLLER)
    try:
        ce.upload(c[0:3])
        assert len(ce.encode(rewind=False)[1]) == 2
        ce.upload(c[3:5], first=3)
        ce.upload(c[1:2], first=1)
        refused(P, lambda: ce.encode(rewind=False), "lookahead: frames 1..4 do not fit the input ring")
    finally:
        ce.close()
