"""GPU: decoder surfaces as device input -- 16-bit samples (H264E_DEV_DEPTH: torch.uint16 / torch.int16 tensors) and 4:4:4 chroma
(H264E_DEV_CHROMA_444) -- through the gfx950 kernels of enc_hbd.h.  For every case the input slot holds exactly the model's picture
(tests/hbd_model.py) and the clip's stream is the stream of that 8-bit picture through the existing upload; the ladder, the producer's
stream and the quality metrics see the same.  Over-reads are the emulation's to find (tests/test_emu_hbd_input.py): here only results
are compared.  Every comparison is equality of bytes."""
import numpy as np
import pytest

import hbd_model as HM
import pkg

pytestmark = pytest.mark.gpu
GOP, QP = 30, 26
SIZES = [(2, 2), (6, 4), (1030, 4), (64, 48)]


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


def tensor(torch, a, signed=False):
    """a numpy plane (uint8 or uint16) as a CUDA tensor: torch.uint8, torch.uint16, or torch.int16 holding the same bits"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return torch.from_numpy(a).cuda()
    t = torch.from_numpy(a.view(np.int16).copy()).cuda()
    return t if signed else t.view(torch.uint16)


def strided(torch, a, signed=False):
    """the plane as a view that starts one sample into a buffer whose rows are an odd number of samples apart: pointer and stride are
    2 mod 4 bytes for 16-bit samples, odd for 8-bit"""
    h, w = a.shape
    pitch = w + 3 if (w + 3) & 1 else w + 4
    big = np.full((h, pitch), 0xA5A5 & (0xffff if a.dtype.itemsize == 2 else 0xff), a.dtype)
    big[:, 1:1 + w] = a
    t = tensor(torch, big, signed)[:, 1:1 + w]
    assert t.data_ptr() % 4 == a.dtype.itemsize and (t.stride(0) * a.dtype.itemsize) % 4 == (2 if a.dtype.itemsize == 2 else pitch % 4)
    return t


def source(torch, planes, fmt, odd=False, signed=False):
    """the frame (y, u, v) as upload_device(..., fmt) takes it: one packed / (3, h, w) tensor or (y, uv), or strided views per plane"""
    y, u, v = planes
    parts = [y, HM.interleave(u, v)] if fmt.startswith("nv12") or fmt in ("p010", "p016") else [y, u, v]
    if odd:
        return [strided(torch, p, signed) for p in parts]
    if len(parts) == 2:
        return [tensor(torch, p, signed) for p in parts]
    if HM.is_444(fmt):
        return tensor(torch, np.stack(parts), signed)
    return tensor(torch, np.concatenate([p.reshape(-1) for p in parts]).reshape(y.shape[0] * 3 // 2, y.shape[1]), signed)


def run_clip(P, w, h, n, put, **kw):
    ce = P.ClipEncoder(w, h, n, **dict(dict(gop=GOP, qp=QP), **kw))
    try:
        put(ce)
        slots = ce.download()
        out, sizes, _ = ce.encode()
        return slots, out, sizes
    finally:
        ce.close()


def check(P, torch, fmt, depth, frames, dw, dh, src_size=None, crop=None, odd=False, signed=False):
    n = len(frames)
    kw = dict(depth=depth) if HM.is_16(fmt) else {}
    win = dict(src_size=src_size, crop=crop) if src_size else {}
    model = np.stack([HM.slot(f, fmt, depth, dw, dh, crop) if src_size else HM.slot(f, fmt, depth) for f in frames])
    src = [source(torch, f, fmt, odd, signed) for f in frames]
    slots, got, sizes = run_clip(P, dw, dh, n, lambda ce: ce.upload_device(src, fmt, **win, **kw))
    assert np.array_equal(slots, model), "%s depth %s: the slot differs from the model" % (fmt, depth)
    _, want, want_sizes = run_clip(P, dw, dh, n, lambda ce: ce.upload(model))
    assert got == want and sizes == want_sizes, "%s depth %s: the stream differs from that of the 8-bit picture" % (fmt, depth)
    return src, slots, got


def cases_at_size():
    out = []
    for i, fmt in enumerate(HM.FORMATS):
        for j, (w, h) in enumerate(SIZES):
            for k, d in enumerate((10, 12, 16) if HM.is_16(fmt) else (8,)):
                out.append(pytest.param(fmt, w, h, d, (i + j + k) & 1, id="%s-%dx%d-d%d" % (fmt, w, h, d)))
    return out


@pytest.mark.parametrize("fmt,w,h,depth,flip", cases_at_size())
def test_at_size_slot_and_stream(P, torch, fmt, w, h, depth, flip):
    """2 x 2: a lone partial group; 6 x 4: a whole and a partial group; 1030 x 4: more than one block of lanes, an odd chroma width;
    64 x 48: a picture.  Every 16-bit layout meets the depths 10, 12 and 16; half of the cases are strided views at 2 (mod 4) addresses"""
    frames = [HM.picture(w, h, fmt, depth, t) for t in range(2)]
    src, slots, got = check(P, torch, fmt, depth, frames, w, h, odd=bool(flip), signed=bool(flip))
    if fmt in ("i420_16", "nv12_16"):               # ... and the existing 8-bit device path fed with torch's quantiser, the two steps this replaces
        r, s = 1 << (depth - 9), depth - 8
        q = [[((p.view(torch.int16).int() & 0xffff) + r >> s).clamp(max=255).to(torch.uint8) for p in (f if isinstance(f, list) else [f])] for f in src]
        q = [f if len(f) > 1 else f[0] for f in q]
        slots8, got8, _ = run_clip(P, w, h, len(frames), lambda ce: ce.upload_device(q, fmt[:4]))
        assert np.array_equal(slots8, slots) and got8 == got


@pytest.mark.parametrize("fmt", HM.FORMATS)
@pytest.mark.parametrize("odd", [False, True], ids=["tight", "2mod4"])
def test_addressing(P, torch, fmt, odd):
    check(P, torch, fmt, 10, [HM.picture(22, 6, fmt, 10, 3)], 22, 6, odd=odd)


@pytest.mark.parametrize("depth", list(HM.DEPTHS))
def test_all_words(P, torch, depth):
    """every 16-bit word at every depth: luma holds each twice, U the lower half, V the upper"""
    check(P, torch, "i420_16", depth, [HM.all_patterns_picture()], 512, 256, signed=bool(depth & 1))


def window_cases():
    out = []
    for i, fmt in enumerate(HM.FORMATS):
        for j, name in enumerate(HM.windows_of(fmt)):
            out.append(pytest.param(fmt, name, (10, 12, 16)[(i + j) % 3], (i + j) & 1, id="%s-%s" % (fmt, name)))
    return out


@pytest.mark.parametrize("fmt,name,depth,flip", window_cases())
def test_window_slot_and_stream(P, torch, fmt, name, depth, flip):
    (sw, sh), (dw, dh), crop = HM.WINDOWS[name]
    frames = [HM.picture(sw, sh, fmt, depth, t) for t in range(1 if sw > 256 else 2)]
    check(P, torch, fmt, depth, frames, dw, dh, (sw, sh), crop, odd=bool(flip))


@pytest.mark.parametrize("fmt", HM.FORMATS + ("p010",))
def test_frame_at_a_time(P, torch, fmt):
    depth = 16 if fmt == "p010" else 12
    model_fmt = "nv12_16" if fmt == "p010" else fmt
    kw = dict(depth=depth) if HM.is_16(fmt) and fmt != "p010" else {}
    for (sw, sh), (dw, dh), crop in (((64, 48), (64, 48), None), ((100, 76), (64, 48), (2, 4, 96, 72))):
        scaled = (sw, sh) != (dw, dh)
        frames = [HM.picture(sw, sh, model_fmt, depth, t) for t in range(2)]
        win = dict(src_size=(sw, sh), crop=crop) if scaled else {}
        model = np.stack([HM.slot(f, model_fmt, depth, dw, dh, crop) if scaled else HM.slot(f, model_fmt, depth) for f in frames])
        _, want, want_sizes = run_clip(P, dw, dh, len(frames), lambda ce: ce.upload(model))
        e = P.Encoder(dw, dh, gop=GOP, qp=QP)
        parts = [e.encode_device(source(torch, f, fmt, odd=scaled), fmt, **win, **kw) for f in frames]
        e.close()
        assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """torch writes the P010 surface on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer and overwritten as soon as the call returns: the slots hold the first contents, at size and through the window"""
    (sw, sh), (dw, dh), n, fmt = (256, 128), (128, 64), 2, "p010"
    frames = [HM.picture(sw, sh, "nv12_16", 16, t) for t in range(n)]
    plain = np.stack([HM.slot(f, "nv12_16", 16) for f in frames])
    scaled = np.stack([HM.slot(f, "nv12_16", 16, dw, dh) for f in frames])
    staged = [source(torch, f, fmt, signed=True) for f in frames]
    y = torch.zeros((sh, sw), dtype=torch.int16, device="cuda")
    uv = torch.zeros((sh // 2, sw), dtype=torch.int16, device="cuda")
    busy = torch.ones((1024, 1024), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a = P.ClipEncoder(sw, sh, n, gop=GOP, qp=QP)
    b = P.ClipEncoder(dw, dh, n, gop=GOP, qp=QP)
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
    a.close()
    b.close()
    assert np.array_equal(got_plain, plain), "the ingest did not wait for the producer's stream, or read the frame after the call had returned"
    assert np.array_equal(got_scaled, scaled), "the scaler did not wait for the producer's stream, or read the frame after the call had returned"


def test_ladder_from_a_p010_source(P, torch):
    """two rungs from one P010 source: each rung's stream is the stream from the quantised NV12 source"""
    sw, sh, n = 128, 96, 2
    frames = [HM.picture(sw, sh, "nv12_16", 16, t) for t in range(n)]
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26))]
    got = P.encode_ladder([source(torch, f, "p010") for f in frames], "p010", (sw, sh), rungs, gop=GOP)
    nv12 = [source(torch, HM.eight_bit(f, "nv12_16", 16), "nv12") for f in frames]
    want = P.encode_ladder(nv12, "nv12", (sw, sh), rungs, gop=GOP)
    for (out, sizes, _), (out8, sizes8, _) in zip(got, want):
        assert out == out8 and sizes == sizes8 and len(out) > 0


def test_quality_sees_the_slot(P, torch):
    """read_quality() after a 16-bit upload: the values after the quantised 8-bit upload"""
    w, h, n, fmt, depth = 64, 48, 2, "i420_16", 10
    frames = [HM.picture(w, h, fmt, depth, t) for t in range(n)]
    res = []
    for put in (lambda ce: ce.upload_device([source(torch, f, fmt) for f in frames], fmt, depth=depth),
                lambda ce: ce.upload_device([source(torch, HM.eight_bit(f, fmt, depth), "i420") for f in frames], "i420")):
        ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, quality=True)
        put(ce)
        out = ce.encode()[0]
        ssd, ssim = ce.read_quality()
        ce.close()
        res.append((out, ssd, ssim))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
    assert res[0][1].shape == (n, 3) and res[0][1].any()
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    e.encode_device(source(torch, frames[0], fmt), fmt, depth=depth)
    q16 = e.read_quality()
    e.close()
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    e.encode_device(source(torch, HM.eight_bit(frames[0], fmt, depth), "i420"), "i420")
    q8 = e.read_quality()
    e.close()
    assert np.array_equal(q16[0], q8[0]) and np.array_equal(q16[1], q8[1])


def test_plane_extents_count_sample_bytes_and_chroma_geometry(P, torch):
    """what the emulation cannot check: a plane must lie inside ONE device allocation from its first to its last byte -- a 16-bit plane
    one sample short, a 4:4:4 chroma plane of 4:2:0 size, and a window whose last row leaves the plane are refused without a launch;
    the exact sizes are taken"""
    (sw, sh), (dw, dh) = (128, 96), (64, 48)
    L = P.load()
    owned = []

    def dev(nbytes):
        p = L.H264E_dev_malloc(0, nbytes)
        assert p
        owned.append(p)
        return p

    ce = P.ClipEncoder(dw, dh, 1, gop=GOP, qp=QP)
    try:
        y16, c16, y8 = dev(dw * dh * 2), dev(dw * dh // 2), dev(dw * dh)
        short16, half8 = dev(dw * dh * 2 - 2), dev(dw * dh // 4)
        ce.upload_device([[(y16, dw * 2), (c16, dw), (c16, dw)]], "i420_16", depth=10)
        ce.upload_device([[(y16, dw * 2), (y16, dw * 2)]], "p010")                   # (dh/2 rows of the luma plane serve as its U,V pairs)
        ce.upload_device([[(y8, dw), (y8, dw), (y8, dw)]], "i444")
        ce.upload_device([[(y16, dw * 2), (y16, dw * 2), (y16, dw * 2)]], "i444_16", depth=12)
        for planes, fmt, kw, k in (([(short16, dw * 2), (c16, dw), (c16, dw)], "i420_16", dict(depth=10), 0),
                                   ([(y16, dw * 2), (c16, dw), (y8, dw)], "i420_16", dict(depth=10), None),       # y8 holds more than a chroma plane: taken
                                   ([(y16, dw * 2), (c16, dw * 2)], "p010", {}, 1),                           # a quarter of the U,V pairs
                                   ([(y8, dw), (half8, dw), (y8, dw)], "i444", {}, 1),
                                   ([(y16, dw * 2), (y16, dw * 2), (c16, dw * 2)], "i444_16", dict(depth=12), 2)):
            if k is None:
                ce.upload_device([planes], fmt, **kw)
                continue
            with pytest.raises(P.H264EError, match="plane %d .*not memory of device|plane %d .*not inside one allocation" % (k, k)):
                ce.upload_device([planes], fmt, **kw)
        Y16, Y8 = dev(sw * sh * 2), dev(sw * sh)
        ce.upload_device([[(Y16, sw * 2), (Y16, sw * 2), (Y16, sw * 2)]], "i444_16", src_size=(sw, sh))
        ce.upload_device([[(Y8, sw), (Y8, sw), (Y8, sw)]], "i444", src_size=(sw, sh), crop=(64, 48, 64, 48))
        with pytest.raises(P.H264EError, match="plane 2 .*not inside one allocation|plane 2 .*not memory of device"):
            ce.upload_device([[(Y16, sw * 2), (Y16, sw * 2), (Y8, sw * 2)]], "i444_16", src_size=(sw, sh))      # half the bytes
        with pytest.raises(P.H264EError, match="plane 1 .*not inside one allocation|plane 1 .*not memory of device"):
            ce.upload_device([[(Y8, sw), (Y8 + sw, sw), (Y8, sw)]], "i444", src_size=(sw, sh), crop=(64, 48, 64, 48))     # one row down: the last row leaves
    finally:
        ce.close()
        for p in owned:
            L.H264E_dev_free(p)
