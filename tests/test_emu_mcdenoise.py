"""CPU: the motion-compensated temporal denoiser (H264E_clip_set_denoise_motion, enc_mcdenoise.h) in the lane-loop emulation of the
kernels (tests/emu): filtered planes and vector cells against the numpy model (tests/mcdenoise_model.py) through the device layer, streams
against a plain encoder fed the model's pictures, read-backs, and what is refused.  The cases are tests/mcdenoise_cases.py's."""
import os
import subprocess

import numpy as np
import pytest

import mcdenoise_cases as K
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = pkg.EMU_LIB


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", K.PLANES, ids=K.PLANE_IDS)
def test_planes_and_vectors_equal_the_model(case, mode):
    K.check_planes(LIB, case, mode)


def test_lane_order_does_not_matter():
    K.check_planes(pkg.EMU_REV_LIB, K.PLANES[3], 2)
    K.check_planes(pkg.EMU_REV_LIB, K.PLANES[4], 2)


def test_the_cases_take_the_paths_they_are_for():
    w, h, n, name, _, _ = K.PLANES[4]
    cells = K.model(name, w, h, n, 2)[2]
    odd = (np.abs(cells[4][0].astype(np.int64)) & 1).any(axis=-1)
    assert 2 * int(odd.sum()) >= odd.size, "the refinement is nonzero in at least half of frame 4's blocks (%d of %d)" % (odd.sum(), odd.size)
    w, h, n, name, _, _ = K.PLANES[5]
    fields = K.fields(name, w, h, n)
    assert any((f.astype(np.int64) & 1).any() for f in fields), "scene: odd chroma vectors"


def test_stream_is_the_plain_encoders_on_the_models_pictures():
    K.check_stream(pkg.load_pkg(), LIB)


def test_mode_1_stream_and_mode_change():
    K.check_mode_1_stream(pkg.load_pkg(), LIB)


def test_controller_plans_on_the_raw_input_and_codes_the_filtered_frames():
    K.check_controller(pkg.load_pkg(), LIB)


def test_ssd_compares_raw_input_with_reconstruction():
    K.check_ssd_is_against_the_raw_input(pkg.load_pkg(), LIB)


def test_refusals_change_nothing():
    K.check_refusals(pkg.load_pkg(), LIB)
