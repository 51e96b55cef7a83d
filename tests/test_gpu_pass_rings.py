"""GPU: what the frame passes share (tests/pass_ring_cases.py) on the MI355X: pass calls that wrap their rings against a clip whose
rings never do, and inputs replaced behind the passes through every producer.  The cases are shared with the emulation test, which
also holds the refusals."""
import pytest

import pass_ring_cases as K
import pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.mark.parametrize("name,resident,chunks", K.WRAPS, ids=K.WRAP_IDS)
def test_a_pass_call_that_wraps_its_ring(P, name, resident, chunks):
    K.check_wrap(P, None, name, resident, chunks)


@pytest.mark.parametrize("producer", sorted(K.PRODUCERS))
def test_a_replaced_input_makes_every_pass_run_again(P, producer):
    K.check_stale(P, None, K.PRODUCERS[producer])
