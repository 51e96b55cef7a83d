"""CPU emulation: the streaming clip encoder changes its window geometry in the middle of a stream (h264e_host.c clip_adapt: wide after 8
delivered frames whose far reads exceed frames * macroblocks / 8, narrow again after wide_hold frames, a spell that doubles when narrow fails
again), and a launch group whose members disagree issues one launch per geometry (h264e_pool.h group_launch_locked).  Every stream stays the
oracle's, byte for byte, and the H264E_DEBUG launch lines (tests/launch_lines.py) show that the switches happened: these are conditions on the
inputs of tests/geometry_switch_cases.py, re-checked here so that a change of the adaptation that stops reaching them is noticed.

The relaunch across a switch -- a frame stopped under one geometry and encoded again from the row of its first wrong macroblock under the
other, the rows above kept from the other kernel -- was searched for with a loop over 96x80 and 64x48, dy 40 / 24 / 56, four patterns of
motion and max_chains 4 / 2 / 3 / 6: the first 13 candidates gave both directions, the two cases below.

The far-read counter that drives the switch counts reference READS that left the valid window (several per macroblock), and a frame's count
is the sum over its own rows: frames that were stopped add nothing to the frames that are delivered, however many were in flight."""
import functools
import subprocess
import os

import pytest

import geometry_switch_cases as cases
import launch_lines
import launch_plan_cases
import oracle_lib
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N = cases.W, cases.H, cases.N


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def _with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return fn()
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _debug_encode(c, w, h, wide=False, instalments=0, **kw):
    """(stream, sizes, launches, {frame: far reads}) of one emulated encode with H264E_DEBUG; wide: H264E_WIDE_WINDOW=1 at create time"""
    def go():
        with launch_lines.captured_stderr() as err:
            out, sizes, _ = cases.encode(pkg.load_pkg(), c, w, h, instalments, lib=pkg.EMU_LIB, **kw)
        return out, sizes, launch_lines.parse(err[0]), launch_lines.frame_far_reads(err[0])
    return _with_env({"H264E_DEBUG": "1", "H264E_WIDE_WINDOW": "1" if wide else None}, go)


@functools.lru_cache(maxsize=None)
def solo(name):
    kw, instalments = cases.SOLO[name]
    return _debug_encode(cases.clip(), W, H, instalments=instalments, **kw)


@functools.lru_cache(maxsize=None)
def either_way(wide, max_chains):
    """the clip of the "cqp" case with the geometry forced wide or left to adapt, and 2, 4 or 8 frames in flight"""
    return _debug_encode(cases.clip(), W, H, wide=wide, gop=30, qp=30, max_chains=max_chains)


# ---- a. solo switch

@pytest.mark.parametrize("name", sorted(cases.SOLO))
def test_stream_switches_to_wide_back_to_narrow_and_to_wide_again(name):
    out, sizes, launches, _ = solo(name)
    want, want_sizes = cases.reference(name)
    assert sizes == want_sizes and out == want
    g = launch_lines.geometries(launches)
    back = cases.came_back(launches)
    assert back, g                                  # a narrow launch, later a wide one, later a narrow one again
    assert "w" in g[back[2]:], g                    # ... and wide again: the second spell is the doubled wide_hold
    assert sum(l.valid for l in launches) == N


def test_the_doubled_spell_is_longer():
    """the frames delivered in the first wide spell are wide_hold = 30 (and what the launch that crossed its end carried on); the second
    spell starts with 60 to go and ends with the clip"""
    launches = solo("cqp")[2]
    a, b, c = cases.came_back(launches)
    first = sum(l.valid for l in launches[b:c])
    assert 30 <= first < 30 + 4, first


def test_a_launch_starts_below_row_0_in_each_geometry():
    rows = {(l.geometry, l.first_row > 0) for name in cases.SOLO for l in solo(name)[2]}
    assert ("narrow", True) in rows and ("wide", True) in rows


def test_rate_control_has_hedge_leaves_in_a_wide_launch_and_takes_one():
    launches = solo("kbps")[2]
    assert any(l.hedged and l.geometry == "wide" for l in launches)
    assert any(l.geometry == "wide" and l.ended_by.startswith("QP miss covered by a hedge leaf") for l in launches)


@pytest.mark.parametrize("w,h,n", cases.SLIDING)
def test_window_that_slides_along_the_row_under_a_geometry_that_changed(w, h, n):
    c = cases.clip(w, h, n)
    out, sizes, launches, _ = _debug_encode(c, w, h, gop=30, qp=30, max_chains=4)
    assert cases.came_back(launches), launch_lines.geometries(launches)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=30)
    assert sizes == want_sizes and out == want


# ---- b. a relaunch across the switch

@pytest.mark.parametrize("moving,stopped_under", [(cases.two_spells, "narrow"), (cases.always, "wide")], ids=["narrow_to_wide", "wide_to_narrow"])
def test_frame_stopped_under_one_geometry_goes_again_from_a_lower_row_under_the_other(moving, stopped_under):
    c = cases.clip(W, H, N, cases.DY, moving)
    out, sizes, launches, _ = _debug_encode(c, W, H, gop=30, qp=30, max_chains=4)
    across = [(a, b) for a, b in zip(launches, launches[1:]) if a.geometry == stopped_under and b.geometry != a.geometry and b.first_row > 0]
    assert across, launch_lines.geometries(launches)
    assert all(a.ended_by == "mv_clusters mis-speculation" for a, _ in across)
    want, want_sizes = oracle_lib.encode_clip(c, W, H, gop=30, qp=30)
    assert sizes == want_sizes and out == want


# ---- c. same stream either way

def test_same_stream_forced_wide_or_adaptive_with_2_4_or_8_frames_in_flight():
    want, want_sizes = cases.reference("cqp")
    for wide in (False, True):
        for max_chains in (2, 4, 8):
            out, sizes, launches, _ = either_way(wide, max_chains)
            assert sizes == want_sizes and out == want, (wide, max_chains)
            g = launch_lines.geometries(launches)
            assert ("n" not in g) if wide else cases.came_back(launches), (wide, max_chains, g)


# ---- a frame's far reads are its own

def test_far_reads_of_the_delivered_frames_do_not_depend_on_the_frames_in_flight():
    """forced wide, so that every run reads through the same window: per frame the same count with 2, 4 and 8 frames in flight, although
    the launches stop at different frames and leave different numbers of stopped frames behind; a launch's figure is the sum over the frames
    it delivered, 0 when it delivered none"""
    _, _, launches2, frames2 = either_way(True, 2)
    assert sorted(frames2) == list(range(N)) and sum(frames2.values()) > N * (W // 16) * (H // 16)       # (the clip does far-read)
    assert any(l.valid == 0 for l in launches2) and any(l.valid < l.frames_in_flight for l in launches2)
    for max_chains in (2, 4, 8):
        _, _, launches, frames = either_way(True, max_chains)
        assert frames == frames2, max_chains
        assert sum(l.far_reads for l in launches) == sum(frames.values()), max_chains
        assert all(l.far_reads == 0 for l in launches if l.valid == 0), max_chains


def test_far_reads_of_a_frame_encoded_alone_are_the_same():
    """one frame in flight: there is never a frame behind it whose rows could be counted -- the figure every other ring size has to give.
    (The frame itself can still be stopped and go again from a lower row: the rows kept from its first encode count once.)"""
    _, _, launches, frames = _debug_encode(cases.clip(), W, H, wide=True, gop=30, qp=30, max_chains=1)
    assert all(l.frames_in_flight == 1 for l in launches) and any(l.first_row > 0 for l in launches)
    assert sorted(frames) == list(range(N)) and frames == either_way(True, 2)[3]


# ---- d. mixed-geometry launch group

def test_group_with_both_geometries_in_one_round(monkeypatch, tmp_path):
    P = pkg.load_pkg()
    log = tmp_path / "launches"
    GROUP = cases.GROUP
    encs = cases.open_group(P, monkeypatch.setenv, monkeypatch.delenv, lib=pkg.EMU_LIB)
    try:
        monkeypatch.setenv("H264E_DEBUG", "1")
        monkeypatch.setenv(launch_plan_cases.LOG_ENV, str(log))
        with launch_lines.captured_stderr() as err:
            got = P.ClipEncoder.encode_multi(encs)
        monkeypatch.delenv(launch_plan_cases.LOG_ENV)
        solo_launches = {}
        for (name, moving, par), e, (out, sizes, _) in zip(GROUP, encs, got):
            c = cases.clip(W, H, N, cases.DY, moving)
            want, want_sizes = oracle_lib.encode_clip(c, W, H, gop=par["gop"], qp=par["qp"])
            assert sizes == want_sizes and out == want, name
            with launch_lines.captured_stderr() as alone_err:
                alone, alone_sizes, _ = e.encode()              # (rewinds: the member keeps the geometry policy it was opened with)
            assert alone_sizes == sizes and alone == out, name
            solo_launches[name] = launch_lines.parse(alone_err[0])
        monkeypatch.delenv("H264E_DEBUG")
    finally:
        for e in encs:
            e.close()
    # A member's k-th launch is part of the group's k-th round (members that are done have left): per round, the frames in flight of the
    # members' debug lines, by geometry, are the jobs of the round's launches -- wide first -- in the emulation's launch log.
    geometry = {name: set(launch_lines.geometries(ls)) for name, ls in solo_launches.items()}
    assert geometry == {"forced_wide": {"w"}, "adaptive": {"n", "w"}, "adaptive_late": {"n", "w"}, "intra_only": {"n"}}
    forced = solo_launches["forced_wide"]
    launches = launch_lines.parse(err[0])
    logged = [dict(f.split("=") for f in ln.split()) for ln in log.read_text().splitlines()]
    both = 0
    for r in range(1, max(l.index for l in launches) + 1):
        jobs = {g: sum(l.frames_in_flight for l in launches if l.index == r and l.geometry == g) for g in ("wide", "narrow")}
        both += bool(jobs["wide"] and jobs["narrow"])
        # the member that is wide for life is in every round until it is done, from the first one, beside members that are narrow
        if r <= len(forced):
            assert jobs["wide"] >= forced[r - 1].frames_in_flight and (r > 1 or jobs == {"wide": forced[0].frames_in_flight, "narrow": 12}), (r, jobs)
        for g in ("wide", "narrow"):
            if jobs[g]:
                ln = logged.pop(0)
                assert (ln["narrow"], int(ln["njobs"]), int(ln["active"])) == ("01"[g == "narrow"], jobs[g], jobs[g]), (r, g, ln)
    assert not logged and both >= 1
