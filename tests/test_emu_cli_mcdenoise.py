"""CPU: encode_app --denoise-motion M (the product CLI against the emulation library): the binding's stream, and the refusals."""
import os
import subprocess

import pytest

import clips
import mcdenoise_model
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
W, H, N, GOP, WINDOW, KBPS, R = 176, 144, 12, 8, 4, 120, 8


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def clip():
    return mcdenoise_model.hash_noise(clips.pan(W, H, N, step=5))


def _app(tmp_path, c, args, name="o.264"):
    yuv = tmp_path / ("mc_%dx%d.yuv" % (W, H))
    c.tofile(yuv)
    out = tmp_path / name
    r = subprocess.run([APP, "--input", str(yuv), "--output", str(out), "--stats", "x"] + args, capture_output=True, text=True, timeout=600)
    return r, (out.read_bytes() if out.exists() else b"")


def _binding(c, mode):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(W, H, N, lib=pkg.EMU_LIB, gop=GOP, qp=26, abr_kbps=KBPS, lookahead=WINDOW, lookahead_search=R, denoise_motion=mode)
    ce.upload(c)
    out, _, _ = ce.encode()
    ce.close()
    return out


def test_cli_denoise_motion(tmp_path, clip):
    want = {m: _binding(clip, m) for m in (0, 1, 2)}
    assert len(set(want.values())) == 3, "the clip tells the modes apart"
    base = ["--gop", str(GOP), "--kbps", str(KBPS), "--lookahead", str(WINDOW), "--lookahead-search", str(R)]
    for m in (2, 1, 0):
        r, out = _app(tmp_path, clip, base + ["--denoise-motion", str(m)])
        assert r.returncode == 0, r.stdout + r.stderr
        assert out == want[m], "mode %d" % m
    r, out = _app(tmp_path, clip, base)
    assert r.returncode == 0 and out == want[0]


def test_cli_denoise_motion_refusals(tmp_path, clip):
    base = ["--gop", str(GOP), "--kbps", str(KBPS)]
    for args in (base + ["--denoise-motion", "2"], base + ["--lookahead", str(WINDOW), "--denoise-motion", "2"],
                 ["--gop", str(GOP), "--qp", "30", "--denoise-motion", "1"],
                 base + ["--lookahead", str(WINDOW), "--lookahead-search", str(R), "--denoise-motion", "3"],
                 base + ["--lookahead", str(WINDOW), "--lookahead-search", str(R), "--speed", "2", "--denoise-motion", "2"]):
        r, out = _app(tmp_path, clip, args, name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout and "denoise-motion" in r.stdout, (args, r.stdout)
    # the reference's own option stays refused, alone and next to the new one
    for args in (base + ["--denoise", "x"], base + ["--lookahead", str(WINDOW), "--lookahead-search", str(R), "--denoise-motion", "2", "--denoise", "x"]):
        r, out = _app(tmp_path, clip, args, name="refused.264")
        assert r.returncode == 1 and "--denoise is not supported" in r.stdout, (args, r.stdout)
