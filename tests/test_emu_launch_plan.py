"""CPU: the launch decisions of the host side of the device boundary (h264-lab_amd/csrc/h264e_pool.h) -- window geometry, kernel
variant, jobs and workgroups per launch, the dispatch order -- against the recorded plan tests/golden/launch_plan.json.  None of them
changes a byte of the emulated stream (the emulation runs the jobs one after the other whatever the order says), so no other CPU test
would notice if one of them moved; on the GPU they decide the speed (the variant table) and, for the order, whether a
launch makes progress at all."""
import json
import os
import subprocess

import pytest

import launch_plan_cases

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN = json.load(open(os.path.join(HERE, "golden", "launch_plan.json")))


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def test_the_recorded_plan_has_every_case_and_reaches_every_variant_and_both_order_paths():
    assert sorted(PLAN) == sorted(launch_plan_cases.CASES)
    lines = [ln for v in PLAN.values() for ln in v]
    assert {ln.split()[1] for ln in lines} == {"variant=0", "variant=2", "variant=3", "variant=4"}
    assert {ln.split()[0] for ln in lines} == {"narrow=0", "narrow=1"}
    # both geometries within one stream's own launches -- with and without rate control -- and within one launch group (that a ROUND of it
    # holds both: tests/test_emu_geometry_switch.py)
    for name in ("adaptive_96x80", "adaptive_kbps_96x80", "group_mixed_geometry_96x80"):
        assert {ln.split()[0] for ln in PLAN[name]} == {"narrow=0", "narrow=1"}, name
    # XCD bands pad the order: 8 queues of (ceil(nmby / 8) + 1) entries per job instead of nmby + 1 entries per job
    assert PLAN["bands_8_64x48"] != PLAN["cqp_64x48"] and "nblocks=96 " in PLAN["bands_8_64x48"][0] and "nblocks=24 " in PLAN["cqp_64x48"][0]
    assert "nblocks=288 " in PLAN["uhd_3840x2160"][0]              # the default policy bands a single-slice 4K launch: 2 x 8 x 18, not 2 x 136


@pytest.mark.parametrize("name", sorted(launch_plan_cases.CASES))
def test_launch_decisions_are_the_recorded_ones(name):
    """line for line and in launch order (a launch group's launches too: a round is launched by one thread, under the group's lock,
    when its last member has arrived, so neither the rounds nor what they hold depend on thread timing)"""
    got = launch_plan_cases.run(name)
    assert got == PLAN[name]
