"""A refused h264e_hip_submit leaves nothing behind.  tests/submit_refusals.c -- a C program against the headers' own structs, not a
ctypes mirror -- submits each class of bad task array to a 64x48 pool with 3 chains and then, without any h264e_hip_release, encodes
three frames with the clip encoder in the same process; see its head comment for what it checks.  Here against the emulation
library; the GPU twin links the same source against the product library and runs it once."""
import os
import subprocess

import pytest

import oracle_lib
import pkg
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
CASES = ["qp", "slot", "denoised", "mixed"]


def _build(tmp, libdir, libname):
    exe = os.path.join(str(tmp), "submit_refusals_" + libname)
    subprocess.check_call([os.environ.get("CC", "cc"), "-O1", "-g", "-Wall", "-Wextra", "-I", INC, "-o", exe, os.path.join(HERE, "submit_refusals.c"),
                           "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-lm", "-lpthread"])
    return exe


def _run(exe, case, tmp):
    """runs one case; the program's own alarm ends an encode that blocks, the timeout here is only a second line"""
    out = os.path.join(str(tmp), "%s_%s.264" % (os.path.basename(exe), case))
    r = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=120)
    print(r.stdout + r.stderr)
    assert r.returncode == 0 and "FAILED" not in r.stdout, r.stdout + r.stderr
    with open(out, "rb") as f:
        return r.stdout, f.read()


def _oracle_stream():
    return oracle_lib.encode_clip(synth.clip(64, 48, 3), 64, 48, gop=30, qp=26)[0]


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)
    tmp = tmp_path_factory.mktemp("refusals")
    exe = _build(tmp, os.path.dirname(pkg.EMU_LIB), "h264e_emu")
    return exe, tmp, _run(exe, "none", tmp)[1]


def test_the_encode_of_a_fresh_process_is_the_oracles(emu):
    assert emu[2] == _oracle_stream()


@pytest.mark.parametrize("case", CASES + ["all"])
def test_a_refused_submit_changes_nothing(emu, case):
    exe, tmp, fresh = emu
    log, stream = _run(exe, case, tmp)
    assert log.count("ok: ") == 3 * (len(CASES) if case == "all" else 1) + 1         # three checks per refusal, and the encode
    assert stream == fresh


@pytest.mark.gpu
def test_gpu_a_refused_submit_changes_nothing(tmp_path):
    """the same program against the product library, once: four refused submits (nothing is launched), then the ordinary encode"""
    libdir = os.path.join(ROOT, "h264-lab_amd", "lib")
    exe = _build(tmp_path, libdir, "h264e_mi355x")
    log, stream = _run(exe, "all", tmp_path)
    assert log.count("ok: ") == 3 * len(CASES) + 1
    assert stream == _oracle_stream()
