"""Clips and runs for the key frames that a stopped launch leaves in their slots (h264e_host.c clip_keep_collect / clip_plan_launch,
DESIGN.md 5), shared by tests/test_emu_key_keep.py and tests/test_gpu_key_keep.py.

A full output buffer stops a launch deterministically: the whole clip is uploaded, then taken in instalments through a buffer sized for
three frames, so every call ends with frames in flight behind the one that did not fit -- key frames among them at a short GOP -- and the
next call's first launch finds them."""
import functools
import os

import clips
import oracle_lib
import synth


@functools.lru_cache(maxsize=None)
def clip(name, w, h, n):
    c = synth.clip(w, h, n) if name == "synth_v1" else clips.make(name, w, h, n)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, w, h, n, **kw):
    """the oracle's (stream, frame sizes)"""
    return oracle_lib.encode_clip(clip(name, w, h, n), w, h, **kw)


def cap_for_three(sizes):
    """an output buffer that any three frames of the stream fit (64: the room the encoder wants for a key frame's parameter sets)"""
    return 3 * max(sizes) + 64


def with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return fn()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def encode(P, c, w, h, cap=None, keep=True, knobs=None, **kw):
    """clip `c` through a ClipEncoder, whole or (cap: bytes of the output buffer) in as many calls as the buffer asks for.  Returns
    (stream, sizes, totals), totals = dict of the calls' summed kept_key_frames / kept_key_rows / spin_relaunches / processed_mbs /
    reencoded_gops, and `calls`.  keep=False: H264E_KEEP_KEY_ROWS=0 while the clip is opened; knobs: H264E_TEST_* variables, set with
    H264E_TEST_KNOBS=1 while it is opened"""
    env = {"H264E_KEEP_KEY_ROWS": None if keep else "0", "H264E_TEST_KNOBS": "1" if knobs else None}
    env.update(knobs or {})
    ce = with_env(env, lambda: P.ClipEncoder(w, h, len(c), **kw))
    tot = dict(kept_key_frames=0, kept_key_rows=0, spin_relaunches=0, processed_mbs=0, reencoded_gops=0, calls=0)
    try:
        ce.upload(c)
        out, sizes = b"", []
        while len(sizes) < len(c):
            o, s, st = ce.encode(rewind=not sizes, cap=cap)
            assert s, "a call delivered no frame"
            out += o
            sizes += s
            tot["calls"] += 1
            for k in tot:
                if k != "calls":
                    tot[k] += getattr(st, k)
        return out, sizes, tot
    finally:
        ce.close()
