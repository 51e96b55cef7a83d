"""GPU: the cases of tests/handoff_cases.py -- small P frames in which intra 4x4 is close to the inter cost -- through the two-, three- and
four-wave variants of the macroblock kernel on the MI355X, against the oracle: stream, frame sizes and every macroblock's type and mv[0].
The order in which the search wave's bounds and decision reach the reconstruction wave is whatever the clock produces here, and nothing
tries to force it; tests/test_emu_handoffs.py runs the same cases with the order as an input."""
import pytest

import handoff_cases as K
import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("waves", [2, 3, 4])
@pytest.mark.parametrize("i", range(len(K.CASES)), ids=K.CASE_IDS)
def test_every_multi_wave_variant_gives_the_oracles_stream(P, i, waves):
    what = "H264E_WAVES=%d" % waves
    out, sizes, recs, _ = K.encode(P, None, i, dict(H264E_WAVES=str(waves)))
    K.check_stream(what, i, out, sizes, recs)
