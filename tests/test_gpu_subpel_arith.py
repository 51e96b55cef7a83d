"""GPU: the sub-sample stage of the partition search on sample pairs (enc_kernels.h halfpel3_rows: v_perm_b32, v_pk_add_u16, v_pk_mad_u16,
v_pk_ashrrev_i16, v_pk_max_i16 / v_pk_min_i16, v_dot2_i32_i16) and the packed byte average (wave.h avg4_u8: v_lerp_u8) on the MI355X --
the cases of tests/test_emu_subpel_arith.py through h264e_stage_selftest_kernel: stage hook 8 against the model of
tests/subpel_cases.py (whose reach the CPU test asserts), stage hook 16 over every pair of bytes against the carry-free formula."""
import pytest

import pkg
import subpel_cases as K
import test_stages as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


def test_sub_sample_cases(P):
    run, close = S._hook(None)
    try:
        assert K.check_cases(run) == 2 * (len(K.cases()) + 3 * 8)
    finally:
        close()


def test_avg4_every_pair_of_bytes(P):
    run, close = S._hook(None)
    try:
        K.avg4_all_pairs(run)
    finally:
        close()
