"""The configurations whose launch decisions tests/golden/launch_plan.json records (tests/golden/make_golden_launch_plan.py writes it,
tests/test_emu_launch_plan.py compares): the host side of the device boundary (h264e_pool.h) decides, launch by launch, the window
geometry, the kernel variant, the jobs, the workgroups and the dispatch order -- none of which changes a byte of the emulated stream.
The emulation's launch function writes them down when H264E_EMU_LAUNCH_LOG names a file (tests/emu/emu_backend.cpp log_launch)."""
import os
import tempfile

import clips
import geometry_switch_cases
import pkg

LOG_ENV = "H264E_EMU_LAUNCH_LOG"


def _clip(P, w, h, n, name="synth", **kw):
    e = P.ClipEncoder(w, h, n, lib=pkg.EMU_LIB, **kw)
    e.upload(clips.make(name, w, h, n))
    return e


def _one_clip(P, w, h, n, **kw):
    e = _clip(P, w, h, n, **kw)
    try:
        e.encode()
    finally:
        e.close()


def _rate_control(P):
    """tests/test_emu_parity.py _rate_controlled_clip_through_a_small_output_buffer: hedge leaves, QP misses, and an output buffer of one
    and a half frames, so that launches are stopped and repeated"""
    w, h, n = 96, 80, 12
    e = _clip(P, w, h, n, gop=5, kbps=60)
    try:
        _, sizes, _ = e.encode()
        cap, done, calls = max(sizes) * 3 // 2, 0, 0
        while done < n:
            _, s, _ = e.encode(rewind=not calls, cap=cap)
            done += len(s)
            calls += 1
    finally:
        e.close()


def _per_frame(P):
    w, h, n = 64, 48, 3
    c = clips.make("synth", w, h, n)
    e = P.Encoder(w, h, gop=30, qp=26, lib=pkg.EMU_LIB)
    try:
        for t in range(n):
            e.encode(c[t])
    finally:
        e.close()


def _group(P, w, h, specs, **kw):
    """clips of different length in one launch group: merged orders, members that leave, `parallel` by member count"""
    encs = [_clip(P, w, h, n, name=name, gop=gop, qp=26, **kw) for name, n, gop in specs]
    try:
        P.ClipEncoder.encode_multi(encs)
    finally:
        for e in encs:
            e.close()


def _adaptive(P, name):
    """tests/geometry_switch_cases.py: a stream that changes its window geometry on its own, twice there and once back"""
    kw, instalments = geometry_switch_cases.SOLO[name]
    geometry_switch_cases.encode(P, geometry_switch_cases.clip(), geometry_switch_cases.W, geometry_switch_cases.H, instalments, lib=pkg.EMU_LIB, **kw)


def _group_mixed_geometry(P):
    """members that disagree about the geometry, one of them wide for life: rounds of two launches, the wide one first"""
    saved = os.environ.get("H264E_WIDE_WINDOW")
    encs = []
    try:
        encs = geometry_switch_cases.open_group(P, os.environ.__setitem__, os.environ.pop, lib=pkg.EMU_LIB)
        P.ClipEncoder.encode_multi(encs)
    finally:
        for e in encs:
            e.close()
        if saved is not None:
            os.environ["H264E_WIDE_WINDOW"] = saved


# name -> (environment of the case, what runs).  Every kernel variant and both order paths (plain, XCD bands) are reached:
CASES = {
    "intra_64x48": ({}, lambda P: _one_clip(P, 64, 48, 4, gop=1, qp=26)),                               # variant 0
    "cqp_64x48": ({}, lambda P: _one_clip(P, 64, 48, 6, gop=30, qp=26)),                                # variant 3: the grid is resident as a whole
    "cqp_176x144": ({}, lambda P: _one_clip(P, 176, 144, 6, gop=30, qp=26)),                            # variant 3
    "tall_16x2048": ({}, lambda P: _one_clip(P, 16, 2048, 6, gop=30, qp=26)),                           # variant 2: 6 jobs of 129 workgroups
    "tall_16x2048_2_slices": ({}, lambda P: _one_clip(P, 16, 2048, 13, gop=30, qp=26, slices=2)),       # variant 4: 13 jobs x 128 rows >= 1536
    "pan_176x144_ring_of_2": ({}, lambda P: _one_clip(P, 176, 144, 9, name="pan", gop=3, qp=30, max_chains=2)),   # a bounded ring, re-encodes
    "kbps_96x80_small_buffer": ({}, _rate_control),                                                     # `tree`, relaunches
    "kbps_16x2048_2_slices": ({}, lambda P: _one_clip(P, 16, 2048, 13, gop=30, kbps=400, slices=2)),    # `tree` keeps a big sliced launch off variant 4
    "per_frame_64x48": ({}, _per_frame),
    "group_176x144": ({}, lambda P: _group(P, 176, 144, (("synth", 9, 3), ("pan", 7, 3), ("noise", 5, 2)), max_chains=3)),
    "group_16x2048": ({}, lambda P: _group(P, 16, 2048, (("synth", 8, 30), ("ramp", 6, 30)))),          # variant 4 because two streams are parallel work
    "bands_8_64x48": ({"H264E_XCD_BANDS": "8"}, lambda P: _one_clip(P, 64, 48, 6, gop=30, qp=26)),      # the banded order through submit
    "uhd_3840x2160": ({}, lambda P: _one_clip(P, 3840, 2160, 2, gop=30, qp=30)),                        # the default band policy
    "adaptive_96x80": ({}, lambda P: _adaptive(P, "cqp")),                                              # narrow, wide, narrow, wide within one stream
    "adaptive_kbps_96x80": ({}, lambda P: _adaptive(P, "kbps")),                                        # ... with hedge leaves under both
    "group_mixed_geometry_96x80": ({}, _group_mixed_geometry),                                          # one member opened under H264E_WIDE_WINDOW
}


def run(name):
    """the launch lines of one case, in launch order"""
    env, fn = CASES[name]
    P = pkg.load_pkg()
    fd, path = tempfile.mkstemp(suffix=".launches")
    os.close(fd)
    saved = {k: os.environ.get(k) for k in list(env) + [LOG_ENV]}
    try:
        os.environ.update(env)
        os.environ[LOG_ENV] = path
        fn(P)
        with open(path) as f:
            return f.read().splitlines()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        os.unlink(path)
