"""Clips and configurations that make the streaming clip encoder change its window geometry in the middle of a stream (h264e_host.c
clip_adapt), shared by tests/test_emu_geometry_switch.py and tests/test_gpu_geometry_switch.py.

The clip: synth_v1 luma moving down 40 samples per frame -- beyond the narrow window's reach, so the search reads the reference through
the far path -- for frames 0..12, still for 27 frames, moving again from frame 40.  The encoder goes wide after 8 delivered frames of the
first spell, back to narrow when its 30 frames of wide are over (about frame 40), and wide again, for a doubled spell, when the second
spell of motion has delivered 8 frames."""
import functools

import clips
import oracle_lib

W, H, N, DY = 96, 80, 60, 40


def two_spells(t):
    return t < 13 or t >= 40


# name -> (ClipEncoder arguments, instalments).  The stream's own parameters (what the oracle gets too) and how it is run: the ring of
# frames in flight, the input ring, uploads in instalments through a small output buffer.
# (kbps: with max_chains=6 the ring has no spare slot for a hedge leaf behind the 6 frames of a rate-controlled launch; 8 has.)
SOLO = {
    "cqp": (dict(gop=30, qp=30, max_chains=4), 0),
    "two_slices": (dict(gop=30, qp=30, max_chains=4, slices=2), 0),
    "kbps": (dict(gop=30, kbps=300, max_chains=8), 0),
    "gop7_speed9": (dict(gop=7, qp=24, speed=9, max_chains=4), 0),
    "input_ring_of_9": (dict(gop=30, qp=30, max_chains=4, resident=9), 8),
}
RUN_ONLY = ("max_chains", "resident")          # not the stream's: the oracle does not know them
# pictures wider than the window, where it slides along the macroblock row (tests/test_emu_sliding_window.py): 11 and 21 macroblocks
SLIDING = [(176, 144, 48), (336, 64, 48)]


@functools.lru_cache(maxsize=None)
def clip(w=W, h=H, n=N, dy=DY, moving=two_spells):
    c = clips.vpan(w, h, n, dy, moving)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, w=W, h=H, n=N, moving=two_spells):
    """the oracle's (stream, frame sizes) for a SOLO configuration"""
    kw = {k: v for k, v in SOLO[name][0].items() if k not in RUN_ONLY}
    return oracle_lib.encode_clip(clip(w, h, n, DY, moving), w, h, **kw)


def encode(P, c, w, h, instalments=0, cap=3000, **kw):
    """(stream, frame sizes, spin relaunches) of clip `c` through a ClipEncoder; instalments > 0: uploaded in that many parts (an input ring smaller than
    the clip), every part encoded through an output buffer of `cap` bytes before the next one is uploaded"""
    n = len(c)
    ce = P.ClipEncoder(w, h, n, **kw)
    try:
        if not instalments:
            ce.upload(c)
            out, sizes, st = ce.encode()
            return out, sizes, st.spin_relaunches
        out, sizes, spins, per = b"", [], 0, -(-n // instalments)
        for a in range(0, n, per):
            b = min(n, a + per)
            ce.upload(c[a:b], first=a)
            while len(sizes) < b:
                o, s, st = ce.encode(rewind=False, cap=cap)
                out += o
                sizes += s
                spins += st.spin_relaunches
        return out, sizes, spins
    finally:
        ce.close()


def always(t):
    return True


def late(t):
    return t >= 20


# a launch group whose members disagree about the geometry: wide for life, two that switch at different frames, one that never far-reads
GROUP = [("forced_wide", two_spells, dict(gop=30, qp=30, max_chains=4)),
         ("adaptive", two_spells, dict(gop=30, qp=30, max_chains=4)),
         ("adaptive_late", late, dict(gop=30, qp=30, max_chains=4)),
         ("intra_only", two_spells, dict(gop=1, qp=30, max_chains=4))]


def open_group(P, setenv, delenv, **kw):
    """the four members with their clips uploaded, the first one opened while H264E_WIDE_WINDOW is set and the others after it was
    deleted (H264E_clip_open reads it once; the rewinds of encode_multi and encode do not ask again); setenv / delenv: monkeypatch's, or
    os.environ's __setitem__ / pop"""
    encs = []
    for name, moving, par in GROUP:
        if name == "forced_wide":
            setenv("H264E_WIDE_WINDOW", "1")
        else:
            delenv("H264E_WIDE_WINDOW", None)
        e = P.ClipEncoder(W, H, N, **par, **kw)
        e.upload(clip(W, H, N, DY, moving))
        encs.append(e)
    return encs


def came_back(launches):
    """narrow, later wide, later narrow again: the positions of the three launches, or None"""
    g = "".join(l.geometry[0] for l in launches)
    a = g.find("n")
    b = g.find("w", a + 1) if a >= 0 else -1
    c = g.find("n", b + 1) if b >= 0 else -1
    return (a, b, c) if c >= 0 else None
