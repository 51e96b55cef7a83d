"""GPU: the partition search's chain step (enc_mb.h diamond_g) on the MI355X -- the cases of tests/test_emu_scan_step.py:
the recorded `diamond` searches of the stage fixtures and the full-sample cases where the 16-bit truncation of the cached costs shows
through h264e_stage_selftest_kernel, and the small streams of tests/scan_step_cases.py through the two-wave, 4-per-SIMD and four-wave
variants of the macroblock kernel (H264E_WAVES, as tests/test_gpu_handoffs.py forces them) against the oracle library: bytes, frame
sizes, decision trace, and no spin relaunch."""
import pytest

import handoff_cases
import pkg
import scan_step_cases as K
import test_stages as S
from test_emu_scan_step import diamond_fixture_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


def test_recorded_searches_of_the_reference(P):
    run, close = S._hook(None)
    try:
        assert diamond_fixture_cases(run) > 0
    finally:
        close()


def test_full_sample_searches_where_the_truncation_shows(P):
    run, close = S._hook(None)
    try:
        K.check_stage_cases(run)
    finally:
        close()


@pytest.mark.parametrize("waves", [2, 3, 4])
@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.CASE_IDS)
def test_small_streams_in_every_multi_wave_variant(P, i, waves):
    with handoff_cases.environment(H264E_WAVES=str(waves)):
        out, sizes, recs = K.encode(P, None, i)           # (asserts spin_relaunches == 0)
    K.check("H264E_WAVES=%d" % waves, i, out, sizes, recs)
