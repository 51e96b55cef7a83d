"""The cases of the motion-compensated temporal denoiser (H264E_clip_set_denoise_motion, enc_mcdenoise.h) that the emulation test
(tests/test_emu_mcdenoise.py) and the GPU test (tests/test_gpu_mcdenoise.py) share: every check takes the package and the library to
load (None = the product library on the GPU).  The model's pictures are made once per process and handed out read-only."""
import functools

import numpy as np
import pytest

import clips
import denoise_model
import lookahead_motion_model as ML
import mcdenoise_model as M

R = 8               # the lookahead's search range of every case

# (w, h, frames, clip, resident, chunk)
#   64x48: single-slot pool with ping-pong, nbx = 4, nby = 3
#   202x122 noise: 101-byte chroma rows, blocks cover 192x112 only: the strips that no block covers
#   352x288 noisy pan: the refinement is nonzero in nearly every block
#   352x288 scene: chroma motion, a scene cut
#   1920x1080 synth: the product's own row geometry, 1072 of 1080 rows covered
#   16x16 and 18x34: one block / one column of blocks, every window at the plane's edge; 9x17 chroma planes with a strip of one sample
PLANES = [(16, 16, 3, "noise", 2, 2), (18, 34, 3, "ramp", 2, 1), (64, 48, 3, "synth", 1, 1), (202, 122, 4, "noise", 2, 1),
          (352, 288, 5, "noisy_pan", 3, 2), (352, 288, 5, "scene", 5, 5), (1920, 1080, 3, "synth", 3, 3)]
PLANE_IDS = ["%dx%d_%s" % (c[0], c[1], c[3]) for c in PLANES]

STREAM = dict(w=352, h=288, n=8, gop=30, qp=26, clip="noisy_pan")


@functools.lru_cache(maxsize=None)
def source(name, w, h, n):
    c = M.hash_noise(clips.pan(w, h, n, step=5)) if name == "noisy_pan" else clips.make(name, w, h, n)
    c = np.ascontiguousarray(c)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def fields(name, w, h, n):
    """the motion fields of the searched cost pass' model, one search for both modes"""
    return tuple(f[0] for f in ML.analyse(source(name, w, h, n), w, h, R)[1])


@functools.lru_cache(maxsize=None)
def model(name, w, h, n, mode):
    """(the clip, the model's filtered pictures, its vector cells)"""
    c = source(name, w, h, n)
    pics, cells = M.clip(c, w, h, mode, fields=fields(name, w, h, n))
    for p in pics:
        p.setflags(write=False)
    return c, pics, cells


def check_planes(lib, case, mode):
    w, h, n, name, resident, chunk = case
    c, pics, cells = model(name, w, h, n, mode)
    got, got_cells = M.device_planes(lib, c, w, h, resident, chunk, mode, R)
    for f in range(n):
        assert got_cells[f][0].shape == ((h // 2) >> 3, (w // 2) >> 3, 2)
        assert np.array_equal(got_cells[f][0], cells[f][0]), "vectors of frame %d" % f
        assert np.array_equal(got_cells[f][1], cells[f][1]), "sads of frame %d" % f
        assert got[f] is not None and np.array_equal(got[f], pics[f]), "frame %d differs from the model" % f
    assert not got_cells[0][0].any(), "frame 0: zero field, every candidate ties, (0, 0) stays"


def plain_stream(P, lib, pics, w, h, **kw):
    """the stream of a plain clip encoder fed these pictures"""
    ce = P.ClipEncoder(w, h, len(pics), lib=lib, **kw)
    ce.upload(np.stack(pics))
    out, sizes, st = ce.encode()
    ce.close()
    return out, sizes


def stream_case():
    s = STREAM
    c, pics, cells = model(s["clip"], s["w"], s["h"], s["n"], 2)
    return s["w"], s["h"], s["n"], dict(gop=s["gop"], qp=s["qp"]), c, pics, cells


def check_stream(P, lib):
    """constant QP, controller off: the bytes are those of a plain encoder fed the MODEL's filtered frames -- first pass, after a rewind,
    through a 3-frame ring in chunks, after re-uploading frames 4..7, and as one member of an encode_multi pair"""
    w, h, n, kw, c, pics, cells = stream_case()
    want = plain_stream(P, lib, pics, w, h, **kw)
    raw = plain_stream(P, lib, list(c), w, h, **kw)
    assert want[0] != raw[0], "the filter changes the stream"
    ce = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, denoise_motion=2, **kw)
    ce.upload(c)
    out, sizes, st = ce.encode()
    assert (out, sizes) == want and st.spin_relaunches == 0
    out, sizes, st = ce.encode()                    # rewound: cost records, fields and pictures are kept
    assert (out, sizes) == want and st.spin_relaunches == 0
    (i, p, nb), _ = ce.read_lookahead(qp=False)     # the cost pass ran for its field alone: costs, no QPs
    rec = ML.costs(c, w, h, R)
    assert np.array_equal(i, rec[0]) and np.array_equal(p, rec[1]) and np.array_equal(nb, rec[2])
    with pytest.raises(P.H264EError) as e:
        ce.read_lookahead(costs=False)
    assert "no QP" in str(e.value)
    for f in range(n):
        assert np.array_equal(ce.read_denoised(f), pics[f]), "read_denoised(%d)" % f
        mv, sad = ce.read_denoise_motion(f)
        assert np.array_equal(mv, cells[f][0]) and np.array_equal(sad, cells[f][1]), "read_denoise_motion(%d)" % f
    # frames 4..7 again, with other content: cost records, fields and pictures from 4 onward are new, the state in front of 4 is kept
    c2 = np.array(c)
    c2[4:] = source("scene", w, h, n)[4:]
    pics2, cells2 = M.clip(c2, w, h, 2, R)
    want2 = plain_stream(P, lib, pics2, w, h, **kw)
    ce.upload(c2[4:], first=4)
    with pytest.raises(P.H264EError) as e:
        ce.read_denoised(5)
    assert "frames 0..3 have" in str(e.value), str(e.value)
    out, sizes, st = ce.encode()
    assert (out, sizes) == want2 and want2 != want and st.spin_relaunches == 0
    assert np.array_equal(ce.read_denoised(6), pics2[6]) and np.array_equal(ce.read_denoise_motion(6)[0], cells2[6][0])
    ce.close()
    # a bounded input ring of 3 frames, fed while the stream is encoded
    ring = P.ClipEncoder(w, h, n, lib=lib, resident=3, lookahead_search=R, denoise_motion=2, **kw)
    parts, rs = [], []
    for f0 in range(0, n, 3):
        ring.upload(c[f0:f0 + 3], first=f0)
        out, sizes, st = ring.encode(rewind=(f0 == 0))
        assert st.spin_relaunches == 0
        parts.append(out)
        rs += sizes
    assert (b"".join(parts), rs) == want
    # a frame that has left the ring is refused, and the message names the readable frames
    assert np.array_equal(ring.read_denoised(n - 1), pics[n - 1]) and np.array_equal(ring.read_denoised(n - 3), pics[n - 3])
    for f in (0, n - 4, n):
        with pytest.raises(P.H264EError) as e:
            ring.read_denoised(f)
        assert "frame %d has no denoised picture" % f in str(e.value) and "frames %d..%d have" % (n - 3, n - 1) in str(e.value), str(e.value)
        with pytest.raises(P.H264EError) as e:
            ring.read_denoise_motion(f)
        assert "frames %d..%d have" % (n - 3, n - 1) in str(e.value), str(e.value)
    ring.close()
    # one member of a launch group; the other is a plain clip
    a = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, denoise_motion=2, **kw)
    b = P.ClipEncoder(w, h, n, lib=lib, **kw)
    a.upload(c)
    b.upload(c)
    res = P.ClipEncoder.encode_multi([a, b])
    a.close()
    b.close()
    assert res[0][:2] == want and res[1][:2] == raw and res[0][2].spin_relaunches == 0 and res[1][2].spin_relaunches == 0


def check_controller(P, lib):
    """the lookahead controller on: the planned QPs read back, the model's filtered frames encoded with that schedule -- the same bytes"""
    w, h, n, kw, c, pics, _ = stream_case()
    ce = P.ClipEncoder(w, h, n, lib=lib, gop=4, qp=30, abr_kbps=150, lookahead=4, lookahead_search=R, denoise_motion=2)
    ce.upload(c)
    out, sizes, st = ce.encode()
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    assert st.spin_relaunches == 0 and len(sizes) == n
    assert plain_stream(P, lib, pics, w, h, gop=4, qp=30, qp_schedule=qp) == (out, sizes)


def check_mode_1_stream(P, lib):
    w, h, n, kw, c, _, _ = stream_case()
    pics = model(STREAM["clip"], w, h, n, 1)[1]
    ce = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, denoise_motion=1, **kw)
    ce.upload(c)
    out, sizes, _ = ce.encode()
    assert (out, sizes) == plain_stream(P, lib, pics, w, h, **kw)
    # another mode at frame 0: every picture is made again
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise_motion(2)
    out, sizes, _ = ce.encode(rewind=False)
    assert (out, sizes) == plain_stream(P, lib, model(STREAM["clip"], w, h, n, 2)[1], w, h, **kw)
    ce.close()


def check_ssd_is_against_the_raw_input(P, lib):
    w, h, n, kw, c, pics, _ = stream_case()
    ce = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, denoise_motion=2, quality=dict(ssd=True, ssim=False), **kw)
    ce.upload(c)
    ce.encode()
    ssd, _ = ce.read_quality()
    recs = [ce.read_recon(f) for f in range(n)]
    ce.close()
    cw, chh = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    for f in range(n):
        raw, r = c[f].astype(np.int64), recs[f].astype(np.int64)
        planes = [(raw[: w * h].reshape(h, w), r[: cw * chh].reshape(chh, cw)[:h, :w])]
        o, ro = w * h, cw * chh
        for _ in range(2):
            planes.append((raw[o: o + w * h // 4].reshape(h // 2, w // 2), r[ro: ro + cw * chh // 4].reshape(chh // 2, cw // 2)[: h // 2, : w // 2]))
            o += w * h // 4
            ro += cw * chh // 4
        assert [int(x) for x in ssd[f]] == [int(((a - b) ** 2).sum()) for a, b in planes], "frame %d" % f


def check_refusals(P, lib):
    """every refusal names its value and leaves the clip as it was: the stream afterwards is the one without the refused call"""
    w, h, n = 64, 48, 4
    c = source("synth", w, h, n)
    kw = dict(gop=30, qp=26)
    plain = plain_stream(P, lib, list(c), w, h, **kw)
    den = plain_stream(P, lib, list(c), w, h, denoise=True, **kw)
    mc = plain_stream(P, lib, model("synth", w, h, n, 2)[1], w, h, **kw)
    assert len({plain[0], den[0], mc[0]}) == 3, "the clip tells the three apart"

    def refused(ce, mode, text, want):
        with pytest.raises(P.H264EError) as e:
            ce.set_denoise_motion(mode)
        assert text in str(e.value), str(e.value)
        ce.upload(c)
        assert ce.encode()[:2] == want
        for f in (0, n - 1):
            with pytest.raises(P.H264EError):
                ce.read_denoise_motion(f)

    ce = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, **kw)
    for bad in (3, -1):
        refused(ce, bad, "mode %d is outside 0..2" % bad, plain)
    ce.close()
    ce = P.ClipEncoder(w, h, n, lib=lib, **kw)
    refused(ce, 2, "call H264E_clip_set_lookahead_search first", plain)
    ce.close()
    ce = P.ClipEncoder(w, h, n, lib=lib, denoise=True, **kw)           # the plain denoiser stays what it was
    refused(ce, 1, "call H264E_clip_set_lookahead_search first", den)
    ce.close()
    ce = P.ClipEncoder(w, h, n, lib=lib, keep_records=1, **kw)
    refused(ce, 2, "keep_records = 1", plain)
    ce.close()
    for speed in (2, 8):
        fast = plain_stream(P, lib, list(c), w, h, speed=speed, **kw)
        ce = P.ClipEncoder(w, h, n, lib=lib, speed=speed, lookahead_search=R, **kw)
        refused(ce, 2, "speed %d" % speed, fast)
        ce.close()
    small = clips.make("ramp", 8, 8, 2)
    ce = P.ClipEncoder(8, 8, 2, lib=lib, lookahead_search=R, **kw)
    with pytest.raises(P.H264EError) as e:
        ce.set_denoise_motion(2)
    assert "below 16x16" in str(e.value) and "8x8" in str(e.value)
    ce.upload(small)
    assert ce.encode()[:2] == plain_stream(P, lib, list(small), 8, 8, **kw)
    ce.close()
    with pytest.raises(P.H264EError):
        P.ClipEncoder(w, h, n, lib=lib, denoise_motion=2, **kw)         # no search range
    # not at frame 0; kept across a rewind; set_denoise(False) switches it off too; range 0 is refused while it is on
    ce = P.ClipEncoder(w, h, n, lib=lib, lookahead_search=R, **kw)
    ce.upload(c)
    ce.encode(rewind=False)
    with pytest.raises(P.H264EError) as e:
        ce.set_denoise_motion(2)
    assert "frame 0" in str(e.value)
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise_motion(2)
    with pytest.raises(P.H264EError) as e:
        ce.set_lookahead_search(0)
    assert "H264E_clip_set_denoise_motion(clip, 0) first" in str(e.value)
    assert ce.encode()[:2] == mc and ce.encode()[:2] == mc
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise(True)                            # on is on already: the mode stays
    assert ce.encode()[:2] == mc
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise(False)
    assert ce.encode()[:2] == plain
    with pytest.raises(P.H264EError) as e:
        ce.read_denoised(0)
    assert "denoiser is off" in str(e.value)
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise_motion(2)
    ce.set_denoise_motion(0)
    assert ce.encode()[:2] == plain
    ce.L.H264E_clip_rewind(ce.c)
    ce.set_denoise(True)
    ce.set_denoise_motion(0)                        # mode 0 leaves the plain denoiser alone
    assert ce.encode()[:2] == den and np.array_equal(ce.read_denoised(n - 1), denoise_model.clip(c, w, h)[n - 1])
    ce.close()

