"""GPU: the motion-compensated temporal denoiser (h264e_mcdenoise_kernel, enc_mcdenoise.h) on the MI355X: filtered planes and vector
cells against the numpy model (tests/mcdenoise_model.py) through the device layer, streams against a plain encoder fed the model's
pictures, read-backs, and what is refused.  The cases are tests/mcdenoise_cases.py's, shared with the emulation test."""
import os

import pytest

import mcdenoise_cases as K
import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "h264-lab_amd", "lib", "libh264e_mi355x.so")


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", K.PLANES, ids=K.PLANE_IDS)
def test_kernel_planes_and_vectors_equal_the_model(P, case, mode):
    K.check_planes(LIB, case, mode)


def test_stream_is_the_plain_encoders_on_the_models_pictures(P):
    K.check_stream(P, None)


def test_mode_1_stream_and_mode_change(P):
    K.check_mode_1_stream(P, None)


def test_controller_plans_on_the_raw_input_and_codes_the_filtered_frames(P):
    K.check_controller(P, None)


def test_ssd_compares_raw_input_with_reconstruction(P):
    K.check_ssd_is_against_the_raw_input(P, None)


def test_refusals_change_nothing(P):
    K.check_refusals(P, None)
