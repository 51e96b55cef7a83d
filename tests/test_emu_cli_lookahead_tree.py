"""CPU: encode_app --lookahead-tree S[,A] (the product CLI against the emulation library): the binding's stream, and the refusals."""
import os
import subprocess

import pytest

import clips
import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
W, H, N, GOP, WINDOW, KBPS, R, S, A = 176, 144, 12, 8, 4, 120, 8, 8, 2


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def _app(tmp_path, c, args, name="o.264"):
    yuv = tmp_path / ("lt_%dx%d.yuv" % (W, H))
    c.tofile(yuv)
    out = tmp_path / name
    r = subprocess.run([APP, "--input", str(yuv), "--output", str(out), "--stats", "x"] + args, capture_output=True, text=True, timeout=600)
    return r, (out.read_bytes() if out.exists() else b"")


def _binding(c, tree):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(W, H, N, lib=pkg.EMU_LIB, gop=GOP, qp=26, abr_kbps=KBPS, lookahead=WINDOW, lookahead_search=R, lookahead_tree=tree)
    ce.upload(c)
    out, sizes, _ = ce.encode()
    _, qp = ce.read_lookahead(costs=False)
    ce.close()
    return out, sizes, qp


def test_cli_lookahead_tree(tmp_path):
    c = clips.make("synth", W, H, N)
    want, sizes, qp = _binding(c, (S, A))
    plain, _, _ = _binding(c, 0)
    assert want != plain, "clip and target tell the tree from no tree"
    base = ["--gop", str(GOP), "--kbps", str(KBPS), "--lookahead", str(WINDOW), "--lookahead-search", str(R)]
    r, out = _app(tmp_path, c, base + ["--lookahead-tree", "%d,%d" % (S, A)])
    assert r.returncode == 0, r.stdout + r.stderr
    assert out == want
    line = "lookahead: window %d, QP %d..%d, %.1f kbps for a target of %d" % (WINDOW, qp.min(), qp.max(), sum(sizes) * 8.0 * 30.0 / N / 1000.0, KBPS)
    assert [l for l in r.stdout.splitlines() if l.startswith("lookahead")] == [line]
    # the whole clip is resident: the default looks min(W, N - W) = W frames ahead
    r, out = _app(tmp_path, c, base + ["--lookahead-tree", str(S)])
    assert r.returncode == 0 and out == _binding(c, (S, WINDOW))[0] == _binding(c, S)[0]
    r, out = _app(tmp_path, c, base + ["--lookahead-tree", "0"])
    assert r.returncode == 0 and out == plain
    r, out = _app(tmp_path, c, base)
    assert r.returncode == 0 and out == plain, "without the option nothing changes"


def test_cli_lookahead_tree_refusals(tmp_path):
    c = clips.make("synth", W, H, N)
    base = ["--gop", str(GOP), "--kbps", str(KBPS), "--lookahead", str(WINDOW)]
    for args in (base + ["--lookahead-tree", str(S)], ["--gop", str(GOP), "--qp", "30", "--lookahead-tree", str(S)],
                 base + ["--lookahead-search", str(R), "--lookahead-tree", "17"], base + ["--lookahead-search", str(R), "--lookahead-tree", "-1"],
                 base + ["--lookahead-search", str(R), "--lookahead-tree", "%d,256" % S]):
        r, out = _app(tmp_path, c, args, name="refused.264")
        assert r.returncode == 1 and "ERROR" in r.stdout and "lookahead-tree" in r.stdout, (args, r.stdout)
