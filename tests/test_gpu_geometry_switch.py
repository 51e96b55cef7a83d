"""GPU: the window geometry changes in the middle of a stream (h264e_host.c clip_adapt) on the MI355X, where the frames of a launch overlap
in time -- the narrow kernel runs 4 steps behind the frame in front, the wide one 7, and both have to read the same reference samples
whichever of them wrote the rows above and the frame before.  The configurations of tests/test_emu_geometry_switch.py (which holds them
to their conditions on the emulation) through the real library, against the oracle byte for byte: the solo switches, a frame that goes
again from a lower row under the other geometry, forced wide against adaptive with 2, 4 and 8 frames in flight, pictures whose window
slides along the row, and a launch group whose rounds issue one launch per geometry.  From the H264E_DEBUG launch lines only what does not
depend on when a launch was stopped: both geometries ran, and narrow ran again after wide.  No dependency wait may have needed its bounded
spin to expire."""
import pytest

import geometry_switch_cases as cases
import launch_lines
import oracle_lib
import pkg

pytestmark = pytest.mark.gpu

W, H, N = cases.W, cases.H, cases.N


def switched_and_came_back(capfd):
    launches = launch_lines.parse(capfd.readouterr().err)
    g = launch_lines.geometries(launches)
    print(g)
    assert "n" in g and "w" in g and "n" in g[g.index("w"):], g


@pytest.mark.parametrize("name", sorted(cases.SOLO))
def test_stream_switches_geometry_and_matches_oracle(monkeypatch, capfd, name):
    monkeypatch.delenv("H264E_WIDE_WINDOW", raising=False)
    monkeypatch.setenv("H264E_DEBUG", "1")
    kw, instalments = cases.SOLO[name]
    want, want_sizes = cases.reference(name)
    out, sizes, spins = cases.encode(pkg.load_pkg(), cases.clip(), W, H, instalments, **kw)
    assert sizes == want_sizes and out == want
    assert spins == 0
    switched_and_came_back(capfd)


@pytest.mark.parametrize("max_chains", [2, 4, 8])
def test_adaptive_stream_with_2_4_or_8_frames_in_flight(monkeypatch, capfd, max_chains):
    monkeypatch.delenv("H264E_WIDE_WINDOW", raising=False)
    monkeypatch.setenv("H264E_DEBUG", "1")
    want, want_sizes = cases.reference("cqp")
    out, sizes, spins = cases.encode(pkg.load_pkg(), cases.clip(), W, H, gop=30, qp=30, max_chains=max_chains)
    assert sizes == want_sizes and out == want
    assert spins == 0
    switched_and_came_back(capfd)


def test_forced_wide_same_stream_and_same_far_reads_per_frame_with_2_4_or_8_frames_in_flight(monkeypatch, capfd):
    """the same clip wide for life: the oracle's stream again, and every delivered frame reports the far reads of its own rows -- the same
    figure however many frames were in flight, stopped and thrown away behind it (here the stopped frames really ran beside it)"""
    monkeypatch.setenv("H264E_WIDE_WINDOW", "1")
    monkeypatch.setenv("H264E_DEBUG", "1")
    want, want_sizes = cases.reference("cqp")
    far = {}
    for max_chains in (2, 4, 8):
        out, sizes, spins = cases.encode(pkg.load_pkg(), cases.clip(), W, H, gop=30, qp=30, max_chains=max_chains)
        assert sizes == want_sizes and out == want, max_chains
        assert spins == 0
        err = capfd.readouterr().err
        launches = launch_lines.parse(err)
        assert set(launch_lines.geometries(launches)) == {"w"}
        far[max_chains] = launch_lines.frame_far_reads(err)
        assert sum(l.far_reads for l in launches) == sum(far[max_chains].values())
    assert sorted(far[2]) == list(range(N)) and sum(far[2].values()) > 0
    assert far[4] == far[2] and far[8] == far[2]


def test_frame_goes_again_from_a_lower_row_after_wide_gave_way_to_narrow(monkeypatch, capfd):
    """motion that never stops: launches end in mis-speculations all the time, the one at the end of the wide spell too (on the emulation the
    next launch starts at a row > 0 under narrow; the other direction is part of the "cqp" case)"""
    monkeypatch.delenv("H264E_WIDE_WINDOW", raising=False)
    monkeypatch.setenv("H264E_DEBUG", "1")
    c = cases.clip(W, H, N, cases.DY, cases.always)
    want, want_sizes = oracle_lib.encode_clip(c, W, H, gop=30, qp=30)
    out, sizes, spins = cases.encode(pkg.load_pkg(), c, W, H, gop=30, qp=30, max_chains=4)
    assert sizes == want_sizes and out == want
    assert spins == 0
    switched_and_came_back(capfd)


@pytest.mark.parametrize("w,h,n", cases.SLIDING)
def test_window_that_slides_along_the_row_under_a_geometry_that_changed(monkeypatch, capfd, w, h, n):
    monkeypatch.delenv("H264E_WIDE_WINDOW", raising=False)
    monkeypatch.setenv("H264E_DEBUG", "1")
    c = cases.clip(w, h, n)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=30)
    out, sizes, spins = cases.encode(pkg.load_pkg(), c, w, h, gop=30, qp=30, max_chains=4)
    assert sizes == want_sizes and out == want
    assert spins == 0
    switched_and_came_back(capfd)


def test_group_with_both_geometries(monkeypatch, capfd):
    """one member wide for life (opened under H264E_WIDE_WINDOW, which the others are not), two adaptive ones that switch at different
    frames, one that never leaves narrow: rounds of two launches from the first round on"""
    P = pkg.load_pkg()
    encs = cases.open_group(P, monkeypatch.setenv, monkeypatch.delenv)
    monkeypatch.setenv("H264E_DEBUG", "1")
    try:
        got = P.ClipEncoder.encode_multi(encs)
        together = launch_lines.parse(capfd.readouterr().err)
        alone_geometry = {}
        for (name, moving, par), e, (out, sizes, st) in zip(cases.GROUP, encs, got):
            want, want_sizes = oracle_lib.encode_clip(cases.clip(W, H, N, cases.DY, moving), W, H, gop=par["gop"], qp=par["qp"])
            assert sizes == want_sizes and out == want, name
            assert st.spin_relaunches == 0, name
            alone, alone_sizes, _ = e.encode()
            assert alone_sizes == sizes and alone == out, name
            alone_geometry[name] = set(launch_lines.geometries(launch_lines.parse(capfd.readouterr().err)))
    finally:
        for e in encs:
            e.close()
    assert alone_geometry["forced_wide"] == {"w"} and alone_geometry["intra_only"] == {"n"}
    assert alone_geometry["adaptive"] == alone_geometry["adaptive_late"] == {"n", "w"}
    # a member's k-th launch belongs to the group's k-th round: the first round already holds the wide member beside three narrow ones
    assert sorted(l.geometry for l in together if l.index == 1) == ["narrow", "narrow", "narrow", "wide"]
