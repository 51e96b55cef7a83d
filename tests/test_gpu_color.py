"""GPU: colour and frame rate (H264E_set_color / H264E_set_frame_rate and their clip forms) on the MI355X with torch CUDA tensors as the
source: the input slots of h264e_ingest_kernel and h264e_scale_rgb_kernel against the numpy model for each of the three new matrix rows
(tests/color_model.py), the streams against the oracle's with nothing but the SPS changed, the rate-control invariant with the longer
parameter sets, and the refusals, which come before any launch.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import clips
import color_model as CM
import oracle_lib
import pkg
import rgbp_model
from test_gpu_rgbp_input import source

pytestmark = pytest.mark.gpu

WINDOWS = {"2to1": ((128, 96), None, (64, 48)), "16to1": ((32, 32), None, (2, 2)), "crop_and_scale": ((200, 120), (14, 6, 180, 108), (68, 36))}


@pytest.fixture(scope="module")
def P():
    p = pkg.load_pkg()
    assert p.load().h264e_hip_device_count() > 0, "no HIP device visible"
    return p


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def frames_for(w, h):
    """two noise frames and the eight corner colours"""
    return np.concatenate([rgbp_model.noisy_clip(w, h, 2), CM.corner_frame(w, h)[None]])


def rgb_tensor(torch, chw, pb, pad):
    """the planar frame as an (h, w, pb) view of interleaved pixels whose rows are w * pb + pad bytes apart"""
    _, h, w = chw.shape
    hwc = np.full((h, w, pb), 0x5A, np.uint8)
    hwc[:, :, :3] = chw.transpose(1, 2, 0)
    buf = torch.full(((h - 1) * (w * pb + pad) + w * pb,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (h, w, pb), (w * pb + pad, pb, 1))
    view.copy_(torch.from_numpy(hwc))
    return view


def slots(P, w, h, n, feed, **kw):
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26, **kw)
    try:
        feed(ce)
        return ce.download()
    finally:
        ce.close()


@pytest.mark.parametrize("w,h", [(2, 2), (64, 48), (202, 122)])
@pytest.mark.parametrize("matrix,full", CM.NEW_ROWS)
def test_plain_slots_hold_the_models_bytes(P, torch, matrix, full, w, h):
    frames = frames_for(w, h)
    want = np.stack([CM.to_i420(f, matrix, full) for f in frames])
    for kind, arg in (("rgb", (3, 1)), ("rgb", (4, 0)), ("rgbp", "padded"), ("rgbp", "chw_slice"), ("rgbp", "chw_rows")):
        srcs = [rgb_tensor(torch, f, *arg) if kind == "rgb" else source(torch, f, arg) for f in frames]
        got = slots(P, w, h, len(frames), lambda ce: ce.upload_device(srcs, kind), color=(matrix, full))
        assert np.array_equal(got, want), "slot contents differ from the model (%s %r)" % (kind, arg)


@pytest.mark.parametrize("geom", sorted(WINDOWS))
@pytest.mark.parametrize("matrix,full", CM.NEW_ROWS)
def test_windowed_slots_hold_the_models_bytes(P, torch, matrix, full, geom):
    src, crop, (w, h) = WINDOWS[geom]
    frames = frames_for(*src)
    want = np.stack([CM.scale_to_i420(f, w, h, crop, matrix, full) for f in frames])
    for layout in ("padded", "chw_rows"):
        srcs = [source(torch, f, layout) for f in frames]
        got = slots(P, w, h, len(frames), lambda ce: ce.upload_device(srcs, "rgbp", src_size=src, crop=crop), color=(matrix, full))
        assert np.array_equal(got, want), "slot contents differ from the model (%s)" % layout


@pytest.mark.parametrize("src", [None, (3840, 2160)])
def test_1080p_bt709_full(P, torch, src):
    """one frame at the flagship size: at the picture's size, and a 4K source reduced to it"""
    w, h = 1920, 1080
    sw, sh = src or (w, h)
    frame = rgbp_model.noisy_clip(sw, sh, 1)[0]
    t = torch.from_numpy(frame).cuda()
    if src:
        want = CM.scale_to_i420(frame, w, h, None, 1, 1)
        got = slots(P, w, h, 1, lambda ce: ce.upload_device([t], "rgbp", src_size=src), color="bt709-full")
    else:
        want = CM.to_i420(frame, 1, 1)
        got = slots(P, w, h, 1, lambda ce: ce.upload_device([t], "rgbp"), color="bt709-full")
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("color,fps", [("bt709", None), (None, 25), ("bt709", (30, 1)), ("bt709-full", (30000, 1001)), ("bt601-full", None)])
def test_streams_differ_from_the_oracles_in_the_sps_alone(P, torch, color, fps):
    w, h, n = 64, 48, 4
    matrix, full = CM.NAMES[color] if color else (0, 0)
    fp = None if fps is None else (fps, 1) if isinstance(fps, int) else fps
    chw = rgbp_model.clip(w, h, n)
    model = np.stack([CM.to_i420(f, matrix, full) for f in chw])
    want, _ = oracle_lib.encode_clip(model, w, h, gop=2, qp=26)
    i420 = clips.make("synth", w, h, n)
    want_yuv, _ = oracle_lib.encode_clip(i420, w, h, gop=2, qp=26)
    kw = dict(gop=2, qp=26, color=color, fps=fps)
    ce = P.ClipEncoder(w, h, n, **kw)
    e = P.Encoder(w, h, **kw)
    try:
        ce.upload_device([source(torch, f, "chw") for f in chw], "rgbp")
        got, sizes, _ = ce.encode()
        parts = [e.encode_device(rgb_tensor(torch, f, 3, 0), "rgb") for f in chw]
    finally:
        ce.close()
        e.close()
    ce = P.ClipEncoder(w, h, n, **kw)
    e = P.Encoder(w, h, **kw)
    try:
        ce.upload_device([torch.from_numpy(f.reshape(h * 3 // 2, w)).cuda() for f in i420], "i420")
        assert np.array_equal(ce.download(), i420)          # signalling only: the samples are not touched
        got_yuv, _, _ = ce.encode()
        parts_yuv = [e.encode(f) for f in i420]
    finally:
        ce.close()
        e.close()
    assert b"".join(parts) == got and [len(p) for p in parts] == sizes and b"".join(parts_yuv) == got_yuv
    for a, b in ((got, want), (got_yuv, want_yuv)):
        spss = CM.compare_streams(a, b, matrix, full, fp)
        assert len(spss) == 2 and spss[0] == spss[1]


def test_rate_control_clip_equals_per_frame_with_longer_parameter_sets(P):
    w, h, n = 176, 144, 8
    c = clips.make("synth", w, h, n)
    kw = dict(gop=4, kbps=300, color="bt709", fps=(30000, 1001))
    e = P.Encoder(w, h, **kw)
    ce = P.ClipEncoder(w, h, n, **kw)
    try:
        parts = [e.encode(f) for f in c]
        ce.upload(c)
        out, sizes, _ = ce.encode()
    finally:
        e.close()
        ce.close()
    assert out == b"".join(parts) and sizes == [len(p) for p in parts]
    spss = [x for x in CM.split_annexb(out) if CM.is_sps(x)]
    assert len(spss) == 2 and all(CM.parse_sps(x)["vui"] == CM.vui_fields(1, 0, (30000, 1001)) for x in spss)


def test_refusals_come_before_any_launch(P, torch):
    """a refused call leaves slots, position and settings as they were: the slots still hold what the accepted setting made of the frames"""
    w, h, n = 64, 48, 4
    chw = rgbp_model.clip(w, h, n)
    model = np.stack([CM.to_i420(f, 1, 0) for f in chw])
    plain, _ = oracle_lib.encode_clip(model, w, h, gop=2, qp=26)
    srcs = [source(torch, f, "chw") for f in chw]
    ce = P.ClipEncoder(w, h, n, gop=2, qp=26, color="bt709", fps=30)
    e = P.Encoder(w, h, gop=2, qp=26, color="bt709", fps=30)
    try:
        ce.upload_device(srcs[:2], "rgbp")
        for enc in (ce, e):
            for bad in ((2, 0), (5, 0), (9, 0), (-1, 0), (0, 1), (1, 2)):
                with pytest.raises(P.H264EError, match="matrix|full_range"):
                    enc.set_color(bad)
            for bad in ((0, 1), (1, 0), (-1, 1), ((1 << 30) + 1, 1)):
                with pytest.raises(P.H264EError, match="numerator|denominator"):
                    enc.set_frame_rate(bad)
        assert np.array_equal(ce.download(0, 2), model[:2])
        first, _, _ = ce.encode()
        nxt = C.c_int()
        ce.L.H264E_clip_position(ce.c, C.byref(nxt), None)
        assert nxt.value == 2
        parts = [e.encode_device(srcs[0], "rgbp")]
        for enc in (ce, e):
            with pytest.raises(P.H264EError, match="frame"):
                enc.set_color("bt601-full")
            with pytest.raises(P.H264EError, match="frame"):
                enc.set_frame_rate(25)
        ce.upload_device(srcs[2:], "rgbp", first=2)
        assert np.array_equal(ce.download(), model)
        rest, _, _ = ce.encode(rewind=False)
        parts += [e.encode_device(s, "rgbp") for s in srcs[1:]]
    finally:
        ce.close()
        e.close()
    assert first + rest == b"".join(parts)
    CM.compare_streams(first + rest, plain, 1, 0, (30, 1))
