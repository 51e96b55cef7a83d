"""GPU: HDR10 device input (H264E_set_tonemap) through the gfx950 kernel of enc_tonemap.h, with torch CUDA tensors as the source.  The
cases are tests/tonemap_cases.py's, the ones the emulation runs: the input slot holds exactly the model's picture (tests/tonemap_model.py
with the library's tables) and the stream is the stream of the model's R'G'B' picture fed as "rgbp".  Over-reads are the emulation's to
find: here only results are compared.  Every comparison is equality of bytes."""
import numpy as np
import pytest

import pkg
import tonemap_cases as TC
import tonemap_model as TM

pytestmark = pytest.mark.gpu


class Gpu:
    """the backend of tests/tonemap_cases.py over torch CUDA tensors"""
    lib = None

    def __init__(self, torch):
        self.torch = torch

    def array(self, a, signed=False):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint8:
            return self.torch.from_numpy(a).cuda()
        t = self.torch.from_numpy(a.view(np.int16).copy()).cuda()
        return t if signed else t.view(self.torch.uint16)

    def planes(self, planes, kind, signed=False):
        out = []
        for a in planes:
            h, w = a.shape
            if kind == "tight":
                out.append(self.array(a, signed))
            elif kind == "separate":                # an allocation of its own, not a piece of torch's pool
                t = self.array(a, signed)
                out.append(t.clone(memory_format=self.torch.contiguous_format))
            else:                                   # "padded": one word in, rows an odd number of words apart; "view": three words in, rows dwords apart
                pitch, off = (w + 1 + (w & 1), 1) if kind == "padded" else (w + 6 + (w & 1), 3)
                big = np.full((h, pitch), 0xA5A5, a.dtype)
                big[:, off:off + w] = a
                out.append(self.array(big, signed)[:, off:off + w])
        return out


@pytest.fixture(scope="module")
def B():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    import torch
    assert torch.cuda.is_available()
    return Gpu(torch)


@pytest.mark.parametrize("fmt,depth,w,h,kind,color,curve,signed", TC.at_size_cases())
def test_at_size_slot_and_stream(B, fmt, depth, w, h, kind, color, curve, signed):
    TC.case_at_size(B, fmt, depth, w, h, kind, color, curve, signed)


@pytest.mark.parametrize("curve", TM.CURVES)
def test_all_codes(B, curve):
    TC.case_all_codes(B, curve)


@pytest.mark.parametrize("name,fmt,depth,kind,color,curve", [
    ("2to1", "p010", 16, "tight", "bt709", "hable"), ("2to1", "i420_16", 10, "padded", None, "clip"),
    ("crop", "nv12_16", 10, "separate", None, "reinhard"), ("crop", "i420_16", 12, "view", "bt709", "hable"),
    ("pure_crop", "i420_16", 10, "tight", "bt709", "hable"), ("pure_crop", "p010", 16, "padded", None, "reinhard")])
def test_window_slot_and_stream(B, name, fmt, depth, kind, color, curve):
    TC.case_window(B, name, fmt, depth, kind, color, curve)


@pytest.mark.parametrize("fmt,depth", [("p010", 16), ("i420_16", 10)])
def test_frame_at_a_time(B, fmt, depth):
    TC.case_frame_at_a_time(B, fmt, depth)


def test_ladder_from_a_p010_source(B):
    TC.case_ladder(B)


def test_off_means_off(B):
    TC.case_off_means_off(B)


def test_refusals_name_the_value_move_nothing_and_leave_the_encoders_usable(B):
    TC.case_refusals(B)


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(B):
    """torch writes the P010 surface on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer and overwritten as soon as the call returns: the slots hold the first contents tone-mapped, at size and through the window"""
    torch = B.torch
    P = pkg.load_pkg()
    (sw, sh), (dw, dh), n, fmt = (64, 48), (32, 24), 2, "p010"
    tables = P.tonemap_tables("pq")
    frames = [TM.picture(sw, sh, 16, t) for t in range(n)]
    plain = np.stack([TM.slot(f, 16, tables) for f in frames])
    scaled = np.stack([TM.window_slot(f, 16, tables, dw, dh) for f in frames])
    staged = [TC.source(B, f, fmt, signed=True) for f in frames]
    y = torch.zeros((sh, sw), dtype=torch.int16, device="cuda")
    uv = torch.zeros((sh // 2, sw), dtype=torch.int16, device="cuda")
    busy = torch.ones((1024, 1024), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a = P.ClipEncoder(sw, sh, n, gop=TC.GOP, qp=TC.QP, tonemap="pq")
    b = P.ClipEncoder(dw, dh, n, gop=TC.GOP, qp=TC.QP, tonemap="pq")
    try:
        with torch.cuda.stream(s):
            assert torch.cuda.current_stream().cuda_stream != 0
            for i in range(n):
                for ce, kw in ((a, {}), (b, dict(src_size=(sw, sh)))):
                    for _ in range(10):
                        busy = busy @ busy * 1e-4           # queued work in front of the write
                    y.copy_(staged[i][0])                   # the producer, on stream s
                    uv.copy_(staged[i][1])
                    ce.upload_device([(y, uv)], fmt, first=i, **kw)         # torch's current stream is the producer
                    y.fill_(0x4000)
                    uv.fill_(0x4000)
            got_plain, got_scaled = a.download(), b.download()
        torch.cuda.synchronize()
    finally:
        a.close()
        b.close()
    assert np.array_equal(got_plain, plain), "the tone-map launch did not wait for the producer's stream, or read the frame after the call had returned"
    assert np.array_equal(got_scaled, scaled), "the window's launches did not wait for the producer's stream, or read the frame after the call had returned"
