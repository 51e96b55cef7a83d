"""GPU: H264E_encode on the MI355X with run parameters that change from frame to frame -- frame type, encode_speed, byte target, QP
window, run_param == NULL, H264E_set_vbv_state in front of a frame -- against what the reference itself answered for the same scripts
(tests/golden/run_params.json): every case, the two 1920x1080 ones included, and a handful again through H264E_encode_device, which
shares the per-frame path.  Exact bytes, frame by frame; no timing, no tolerance."""
import numpy as np
import pytest

import pkg
import run_param_cases as R

pytestmark = pytest.mark.gpu

CASES = R.load()
DEVICE_INPUT = ["overflow_on_key_frames_const_input", "cqp_changes_every_frame_cropped", "denoiser_mixed_speeds_const_input",
                "speed_changes_every_frame_3_slices", "rc_qp_window_narrows", "hd1080_key_speed_bitrate"]
# ... and the first seeded script with const_input_flag = 1 that holds a refused call and a NULL run_param
DEVICE_INPUT.append(next(n for n in sorted(CASES) if n.startswith("random_") and CASES[n]["create"][4]
                         and any(s < 0 for s in CASES[n]["sizes"]) and any(l[7] for l in CASES[n]["frames"])))


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("name", sorted(CASES))
def test_encoder_follows_per_frame_run_params(P, name):
    R.compare(CASES[name], R.replay_product(P, CASES[name]), "MI355X, " + name)


@pytest.mark.parametrize("name", DEVICE_INPUT)
def test_device_input_follows_per_frame_run_params(P, name):
    import torch
    assert torch.cuda.is_available()
    case = CASES[name]
    w, h = case["create"][:2]
    assert case["create"][4] == 1           # H264E_encode_device needs const_input_flag = 1

    def device(frame):
        return torch.from_numpy(np.ascontiguousarray(frame).reshape(h * 3 // 2, w)).cuda(), "i420"

    R.compare(case, R.replay_product(P, case, device=device), "MI355X device input, " + name)
