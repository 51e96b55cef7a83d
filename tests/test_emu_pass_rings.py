"""CPU: what the frame passes share (tests/pass_ring_cases.py) in the lane-loop emulation of the kernels (tests/emu), both lane orders
where kernels run: pass calls that wrap their rings, which frames the readers find on the device, inputs replaced behind the passes
through every producer, and the refusals with their texts."""
import os
import subprocess

import pytest

import pass_ring_cases as K
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def put_synth_range(ce, first, n):
    ce.generate_synth(first, n, t0=first)


def put_upload_range(ce, first, n):
    ce.upload(K.source()[first:first + n], first=first)


@pytest.mark.parametrize("lib", sorted(LIBS))
@pytest.mark.parametrize("name,resident,chunks", K.WRAPS, ids=K.WRAP_IDS)
def test_a_pass_call_that_wraps_its_ring(name, resident, chunks, lib):
    K.check_wrap(pkg.load_pkg(), LIBS[lib], name, resident, chunks)


@pytest.mark.parametrize("name,resident,chunks", K.WRAPS, ids=K.WRAP_IDS)
def test_readers_find_exactly_the_frames_on_the_device(name, resident, chunks):
    K.check_windows(pkg.load_pkg(), LIBS["fwd"], name, resident, chunks)


@pytest.mark.parametrize("lib", sorted(LIBS))
@pytest.mark.parametrize("producer", sorted(K.PRODUCERS))
def test_a_replaced_input_makes_every_pass_run_again(producer, lib):
    K.check_stale(pkg.load_pkg(), LIBS[lib], K.PRODUCERS[producer])


@pytest.mark.parametrize("producer", ["upload", "upload_device"])
def test_upload_behind_a_moved_ring_is_refused(producer):
    K.check_predecessor_has_left(pkg.load_pkg(), LIBS["fwd"], K.PRODUCERS[producer])


def test_generate_synth_behind_a_moved_ring_is_refused_like_an_upload():
    K.check_predecessor_has_left(pkg.load_pkg(), LIBS["fwd"], lambda ce, f, picture: ce.generate_synth(f, 1, t0=f))


def test_upload_into_a_full_ring_is_refused():
    K.check_ring_full(pkg.load_pkg(), LIBS["fwd"], put_upload_range)


def test_generate_synth_into_a_full_ring_is_refused_with_the_uploads_text():
    K.check_ring_full(pkg.load_pkg(), LIBS["fwd"], put_synth_range)


def test_more_frames_than_the_input_ring_holds():
    K.check_do_not_fit(pkg.load_pkg(), LIBS["fwd"])
