"""CPU: H264E_encode with run parameters that change from frame to frame -- frame type, encode_speed, byte target, QP window,
run_param == NULL, H264E_set_vbv_state in front of a frame -- through the lane-loop emulation of the kernels (tests/emu), against what the
reference itself answered for the same scripts (tests/golden/run_params.json).  Exact bytes, frame by frame."""
import os
import subprocess

import pytest

import pkg
import run_param_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = R.load()
SMALL = sorted(n for n, c in CASES.items() if R.pixels(c) <= R.EMU_PIXEL_BUDGET)       # the rest runs on the GPU (tests/test_gpu_run_params.py)


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("name", SMALL)
def test_emulated_encoder_follows_per_frame_run_params(name):
    R.compare(CASES[name], R.replay_product(pkg.load_pkg(), CASES[name], lib=pkg.EMU_LIB), "emulation, " + name)
