"""Content that stands still, through the real kernel: wholly skipped P frames (one run over the whole picture, the frame's "everything
skipped" flag, which enters the rate controller) and wholly skipped macroblock rows above coded ones (runs that the finalizer adds up
over row boundaries).  tests/golden/still.json holds the reference's own streams (tests/golden/make_golden.py); the oracle (CPU), the
kernel sources in the emulation build (CPU) and the GPU (-m gpu) must give the same bytes, through the drop-in encoder and the clip
encoder.  Every case first shows, from the oracle's macroblock trace, that the clip contains what it is for."""
import hashlib
import json
import os
import subprocess

import pytest

import clips
import oracle_lib
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
STILL = json.load(open(os.path.join(HERE, "golden", "still.json")))
IDS = ["%s_%dx%d_%s" % (g["clip"], g["w"], g["h"], g["flags"].replace("--", "").replace(" ", "")) for g in STILL]


def _flags(s):
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), kbps=int(d.get("--kbps", 0)), slices=int(d.get("--threads", 0)))


_ORACLE = {}


def _oracle(g):
    """the oracle's frames of a case and, per frame, how many macroblock rows it skipped entirely -- computed once per case"""
    key = IDS[STILL.index(g)]
    if key not in _ORACLE:
        c = clips.make(g["clip"], g["w"], g["h"], g["frames"])
        e = oracle_lib.Encoder(g["w"], g["h"], **_flags(g["flags"]))
        nmbx, frames, skipped_rows = (g["w"] + 15) // 16, [], []
        for t in range(g["frames"]):
            frames.append(e.encode(c[t]))
            types = [m[0] for m in e.trace()]
            skipped_rows.append(sum(all(v == -1 for v in types[r: r + nmbx]) for r in range(0, len(types), nmbx)))
        e.close()
        _ORACLE[key] = (c, frames, skipped_rows)
    return _ORACLE[key]


def _contains_what_it_is_for(g):
    skipped = _oracle(g)[2]
    nmby = (g["h"] + 15) // 16
    whole = any(s == nmby for s in skipped[1:-1]) and skipped[-1] < nmby        # a wholly skipped P frame with a coded frame behind it
    part = any(0 < s < nmby for s in skipped[1:])                                # wholly skipped rows next to coded ones in one frame
    assert whole if g["clip"] == "still" and (g["w"], g["h"]) == (64, 48) else whole or part, skipped


@pytest.mark.parametrize("g", STILL, ids=IDS)
def test_oracle_matches_reference_on_still_content(g):
    _contains_what_it_is_for(g)
    _, frames, _ = _oracle(g)
    assert [len(f) for f in frames] == g["frame_bytes"]
    assert hashlib.md5(b"".join(frames)).hexdigest() == g["md5"]


def _check(g, **lib):
    _contains_what_it_is_for(g)
    P = pkg.load_pkg()
    c, frames, _ = _oracle(g)
    f = _flags(g["flags"])
    e = P.Encoder(g["w"], g["h"], **f, **lib)
    parts = [e.encode(c[t]) for t in range(g["frames"])]
    e.close()
    assert [len(p) for p in parts] == g["frame_bytes"]
    assert hashlib.md5(b"".join(parts)).hexdigest() == g["md5"] and parts == frames
    ce = P.ClipEncoder(g["w"], g["h"], g["frames"], **f, **lib)
    ce.upload(c)
    out, fs, _ = ce.encode()
    ce.close()
    assert fs == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"]


@pytest.mark.parametrize("g", STILL, ids=IDS)
def test_emulated_kernels_match_reference_on_still_content(g):
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    _check(g, lib=pkg.EMU_LIB)


@pytest.mark.gpu
@pytest.mark.parametrize("g", STILL, ids=IDS)
def test_gpu_matches_reference_on_still_content(g):
    _check(g)
