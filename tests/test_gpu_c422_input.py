"""GPU: 4:2:2 device input -- I422, NV16 and packed YUYV / UYVY, 8-bit samples or 16-bit words in torch.uint16 / torch.int16 tensors
(H264E_DEV_CHROMA_422, H264E_DEV_PACK_*) -- through the gfx950 kernels of enc_422.h.  For every case the input slot holds exactly the
model's picture (tests/c422_model.py) and the clip's stream is the stream of that 8-bit picture through the existing upload; the
frame-at-a-time calls, the producer's stream and the ladder see the same.  Over-reads are the emulation's to find
(tests/test_emu_c422_input.py): here only results are compared.  Every comparison is equality of bytes."""
import numpy as np
import pytest

import c422_model as CM
import hbd_model as HM
from test_gpu_hbd_input import GOP, QP, P, run_clip, strided, tensor, torch  # noqa: F401  (P and torch are the module's fixtures)

pytestmark = pytest.mark.gpu
SIZES = [(2, 2), (6, 4), (1030, 4), (64, 48)]
ALIASES_16 = ("p210", "p216", "y210", "y216")


def source(torch, planes, fmt, odd=False, signed=False):
    """the 4:2:2 frame (y, u, v) as upload_device(..., fmt) takes it.  odd: strided views at 2 (mod 4) or odd addresses, one per array;
    else one (2h, w) tensor in ffmpeg's order for "i422", (y, uv) for "nv16", one (h, w, 2) tensor for the packed orders"""
    arrays = CM.layout(planes, fmt)
    h, w = planes[0].shape
    if odd:
        out = [strided(torch, a, signed) for a in arrays]
        return out if len(out) > 1 else out[0]
    if len(arrays) == 1:
        return tensor(torch, arrays[0], signed).view(h, w, 2)
    if len(arrays) == 2:
        return [tensor(torch, a, signed) for a in arrays]
    return tensor(torch, np.concatenate([a.reshape(-1) for a in arrays]).reshape(2 * h, w), signed)


def depth_kw(fmt, depth):
    return dict(depth=depth) if CM.is_16(fmt) and fmt not in ALIASES_16 else {}


def check(P, torch, fmt, depth, frames, dw, dh, src_size=None, crop=None, odd=False, signed=False):
    n = len(frames)
    win = dict(src_size=src_size, crop=crop) if src_size else {}
    model = np.stack([CM.slot(f, fmt, depth, dw, dh, crop) if src_size else CM.slot(f, fmt, depth) for f in frames])
    src = [source(torch, f, fmt, odd, signed) for f in frames]
    slots, got, sizes = run_clip(P, dw, dh, n, lambda ce: ce.upload_device(src, fmt, **win, **depth_kw(fmt, depth)))
    assert np.array_equal(slots, model), "%s depth %s: the slot differs from the model" % (fmt, depth)
    _, want, want_sizes = run_clip(P, dw, dh, n, lambda ce: ce.upload(model))
    assert got == want and sizes == want_sizes, "%s depth %s: the stream differs from that of the 8-bit picture" % (fmt, depth)
    return src, slots, got


def two_step(torch, src, fmt, depth):
    """what a caller writes today in front of "i420": de-interleave, quantise (the 8-bit samples are the definition's), take the rounded
    mean of the row pairs -- (y, u, v) uint8 tensors"""
    parts = list(src) if isinstance(src, (list, tuple)) else [src]
    if CM.is_16(fmt):
        r, s = 1 << (depth - 9), depth - 8
        parts = [((p.view(torch.int16).int() & 0xffff) + r >> s).clamp(max=255).to(torch.uint8) for p in parts]
    fam = CM.family(fmt)
    if fam == "i422":
        if len(parts) == 1:                          # ffmpeg's buffer: (2h, w)
            h2, w = parts[0].shape
            h = h2 // 2
            flat = parts[0].reshape(-1)
            parts = [flat[:w * h].view(h, w), flat[w * h:w * h * 3 // 2].view(h, w // 2), flat[w * h * 3 // 2:].view(h, w // 2)]
        y, u, v = parts
    else:
        y, uv = parts
        u, v = uv[:, 0::2], uv[:, 1::2]
    mean = lambda c: ((c[0::2].int() + c[1::2].int() + 1) >> 1).to(torch.uint8).contiguous()       # noqa: E731
    return [y.contiguous(), mean(u), mean(v)]


def cases_at_size():
    out = []
    for i, fmt in enumerate(CM.FORMATS):
        for j, (w, h) in enumerate(SIZES):
            for k, d in enumerate((10, 12, 16) if CM.is_16(fmt) else (8,)):
                out.append(pytest.param(fmt, w, h, d, (i + j + k) & 1, id="%s-%dx%d-d%d" % (fmt, w, h, d)))
    return out


@pytest.mark.parametrize("fmt,w,h,depth,flip", cases_at_size())
def test_at_size_slot_and_stream(P, torch, fmt, w, h, depth, flip):
    """2 x 2: a lone partial group, one chroma row from two; 6 x 4: a whole and a partial group; 1030 x 4: more than one block of lanes,
    an odd chroma width; 64 x 48: a picture.  Every 16-bit layout meets the depths 10, 12 and 16; half of the cases are strided views
    (and int16 for the 16-bit names)"""
    frames = [CM.picture(w, h, fmt, depth, t) for t in range(2)]
    src, slots, got = check(P, torch, fmt, depth, frames, w, h, odd=bool(flip), signed=bool(flip))
    if fmt in ("i422", "nv16_16"):                  # ... and the existing "i420" device path fed by torch, the two steps this replaces
        q = [two_step(torch, f, fmt, depth) for f in src]
        slots8, got8, _ = run_clip(P, w, h, len(frames), lambda ce: ce.upload_device(q, "i420"))
        assert np.array_equal(slots8, slots) and got8 == got


def window_cases():
    out = []
    for i, fmt in enumerate(CM.FORMATS):
        for j, name in enumerate(CM.WINDOWS):
            out.append(pytest.param(fmt, name, (10, 12, 16)[(i + j) % 3], (i + j) & 1, id="%s-%s" % (fmt, name)))
    return out


@pytest.mark.parametrize("fmt,name,depth,flip", window_cases())
def test_window_slot_and_stream(P, torch, fmt, name, depth, flip):
    """2:1; a fraction with a crop; the vertical limit (luma 8:1, chroma 16:1); 16:1 in width; a pure crop, which is the ingest of the
    cropped region"""
    (sw, sh), (dw, dh), crop = CM.WINDOWS[name]
    frames = [CM.picture(sw, sh, fmt, depth, t) for t in range(1 if sw > 256 else 2)]
    _, slots, _ = check(P, torch, fmt, depth, frames, dw, dh, (sw, sh), crop, odd=bool(flip), signed=bool(flip))
    if name == "pure_crop":
        cx, cy, cw, ch = crop
        cut = [tuple(np.ascontiguousarray(p[cy:cy + ch, (cx if k == 0 else cx // 2):(cx + cw if k == 0 else (cx + cw) // 2)]) for k, p in enumerate(f)) for f in frames]
        assert np.array_equal(check(P, torch, fmt, depth, cut, dw, dh)[1], slots)


@pytest.mark.parametrize("fmt", CM.FORMATS)
def test_window_beyond_the_vertical_limit_is_refused(P, torch, fmt):
    """(64, 386) to (64, 48): the chroma planes would be reduced by more than 16:1"""
    frame = source(torch, CM.picture(64, 386, fmt, 10, 0), fmt)
    ce = P.ClipEncoder(64, 48, 1, gop=GOP, qp=QP)
    try:
        with pytest.raises(P.H264EError, match="4:2:2 window height 386 is more than 8 times the picture's 48"):
            ce.upload_device([frame], fmt, src_size=(64, 386), **depth_kw(fmt, 10))
    finally:
        ce.close()


@pytest.mark.parametrize("fmt", ["i422", "nv16_16", "uyvy", "p210"])
def test_frame_at_a_time(P, torch, fmt):
    """Encoder.encode_device at size and scaled: a planar, a semi-planar and a packed format, and "p210" """
    depth = 16 if fmt in ALIASES_16 else 12
    for (sw, sh), (dw, dh), crop in (((64, 48), (64, 48), None), ((100, 76), (64, 48), (2, 4, 96, 72))):
        scaled = (sw, sh) != (dw, dh)
        frames = [CM.picture(sw, sh, fmt, depth, t) for t in range(2)]
        win = dict(src_size=(sw, sh), crop=crop) if scaled else {}
        model = np.stack([CM.slot(f, fmt, depth, dw, dh, crop) if scaled else CM.slot(f, fmt, depth) for f in frames])
        _, want, want_sizes = run_clip(P, dw, dh, len(frames), lambda ce: ce.upload(model))
        e = P.Encoder(dw, dh, gop=GOP, qp=QP)
        parts = [e.encode_device(source(torch, f, fmt, odd=scaled), fmt, **win, **depth_kw(fmt, depth)) for f in frames]
        e.close()
        assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """torch writes the UYVY surface on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer and overwritten as soon as the call returns: the slots hold the first contents, at size and through the window"""
    (sw, sh), (dw, dh), n, fmt = (128, 96), (64, 48), 2, "uyvy"
    frames = [CM.picture(sw, sh, fmt, 8, t) for t in range(n)]
    plain = np.stack([CM.slot(f, fmt, 8) for f in frames])
    scaled = np.stack([CM.slot(f, fmt, 8, dw, dh) for f in frames])
    staged = [tensor(torch, CM.layout(f, fmt)[0]) for f in frames]
    surface = torch.zeros((sh, 2 * sw), dtype=torch.uint8, device="cuda")
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
                surface.copy_(staged[i])                # the producer, on stream s
                ce.upload_device([surface], fmt, first=i, **kw)         # torch's current stream is the producer
                surface.fill_(0x40)
        got_plain, got_scaled = a.download(), b.download()
    torch.cuda.synchronize()
    a.close()
    b.close()
    assert np.array_equal(got_plain, plain), "the ingest did not wait for the producer's stream, or read the frame after the call had returned"
    assert np.array_equal(got_scaled, scaled), "the scaler did not wait for the producer's stream, or read the frame after the call had returned"


def test_ladder_from_a_y210_source(P, torch):
    """two rungs from one Y210 source.  Every rung's stream is the stream of the model's picture; and where every chroma row of the source
    comes twice -- a 4:2:0 picture carried as 4:2:2, the case in which reducing the row pairs first and the window second is the same
    arithmetic (tests/test_c422_model.py) -- each rung's stream is the stream from the quantised "nv12" source"""
    sw, sh, n = 128, 96, 2
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26))]
    frames = [CM.picture(sw, sh, "y210", 16, t) for t in range(n)]
    got = P.encode_ladder([source(torch, f, "y210") for f in frames], "y210", (sw, sh), rungs, gop=GOP)
    for (out, sizes, _), (dw, dh, kw) in zip(got, rungs):
        model = np.stack([CM.slot(f, "y210", 16, dw, dh) if (dw, dh) != (sw, sh) else CM.slot(f, "y210", 16) for f in frames])
        _, want, want_sizes = run_clip(P, dw, dh, n, lambda ce: ce.upload(model), **kw)
        assert out == want and sizes == want_sizes and len(out) > 0
    twice = [CM.from_420(y, u[0::2], v[0::2]) for y, u, v in frames]
    got = P.encode_ladder([source(torch, f, "y210") for f in twice], "y210", (sw, sh), rungs, gop=GOP)
    nv12 = [[tensor(torch, HM.quantise(y, 16)), tensor(torch, HM.interleave(HM.quantise(u[0::2], 16), HM.quantise(v[0::2], 16)))] for y, u, v in twice]
    want = P.encode_ladder(nv12, "nv12", (sw, sh), rungs, gop=GOP)
    for (out, sizes, _), (out8, sizes8, _) in zip(got, want):
        assert out == out8 and sizes == sizes8 and len(out) > 0


def test_plane_extents_count_the_422_geometry(P, torch):
    """what the emulation cannot check: a plane must lie inside ONE device allocation from its first to its last byte -- a 4:2:2 chroma
    plane of 4:2:0 size, a packed plane one sample short and a window whose last chroma row leaves its plane are refused without a launch;
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
        y8, c8, c8_420, pk8, pk8_short = dev(dw * dh), dev(dw // 2 * dh), dev(dw // 2 * dh // 2), dev(2 * dw * dh), dev(2 * dw * dh - 1)
        y16, pk16, pk16_short = dev(2 * dw * dh), dev(4 * dw * dh), dev(4 * dw * dh - 2)
        ce.upload_device([[(y8, dw), (c8, dw // 2), (c8, dw // 2)]], "i422")
        ce.upload_device([[(y8, dw), (y8, dw)]], "nv16")                            # (a luma plane has the bytes of the U,V pairs)
        ce.upload_device([(pk8, 2 * dw)], "yuyv")
        ce.upload_device([(pk8, 2 * dw)], "uyvy")
        ce.upload_device([[(y16, 2 * dw), (y8, dw), (y8, dw)]], "i422_16", depth=10)
        ce.upload_device([[(y16, 2 * dw), (y16, 2 * dw)]], "p210")
        ce.upload_device([(pk16, 4 * dw)], "y210")
        for planes, fmt, kw, k in (([(y8, dw), (c8_420, dw // 2), (c8, dw // 2)], "i422", {}, 1),              # a chroma plane of 4:2:0 size
                                   ([(y8, dw), (c8, dw // 2), (c8_420, dw // 2)], "i422", {}, 2),
                                   ([(y16, 2 * dw), (c8, dw), (y8, dw)], "i422_16", dict(depth=10), 1),         # half the bytes of 16-bit 4:2:2 chroma
                                   ([(y8, dw), (c8, dw)], "nv16", {}, 1),                                        # the U,V pairs of 4:2:0
                                   ([(y16, 2 * dw), (y8, 2 * dw)], "p210", {}, 1),
                                   ((pk8_short, 2 * dw), "yuyv", {}, 0),                                         # one sample short
                                   ((pk8_short, 2 * dw), "uyvy", {}, 0),
                                   ((pk16_short, 4 * dw), "y210", {}, 0),
                                   ((pk8, 4 * dw), "uyvy_16", dict(depth=12), 0)):                               # 8-bit bytes for 16-bit words
            with pytest.raises(P.H264EError, match="plane %d .*not memory of device|plane %d .*not inside one allocation" % (k, k)):
                ce.upload_device([planes], fmt, **kw)
        Y8, C8, PK8 = dev(sw * sh), dev(sw // 2 * sh), dev(2 * sw * sh)
        corner = dict(src_size=(sw, sh), crop=(64, 48, 64, 48))                     # the window ends with the source's last sample
        ce.upload_device([[(Y8, sw), (C8, sw // 2), (C8, sw // 2)]], "i422", src_size=(sw, sh))
        ce.upload_device([[(Y8, sw), (C8, sw // 2), (C8, sw // 2)]], "i422", **corner)
        ce.upload_device([[(Y8, sw), (Y8, sw)]], "nv16", **corner)
        ce.upload_device([(PK8, 2 * sw)], "yuyv", **corner)
        with pytest.raises(P.H264EError, match="plane 1 .*not inside one allocation|plane 1 .*not memory of device"):
            ce.upload_device([[(Y8, sw), (C8 + sw // 2, sw // 2), (C8, sw // 2)]], "i422", **corner)           # one row down: the last chroma row leaves
        with pytest.raises(P.H264EError, match="plane 2 .*not inside one allocation|plane 2 .*not memory of device"):
            ce.upload_device([[(Y8, sw), (C8, sw // 2), (dev(sw // 2 * sh // 2), sw // 2)]], "i422", src_size=(sw, sh))   # a chroma plane of 4:2:0 size
        with pytest.raises(P.H264EError, match="plane 1 .*not inside one allocation|plane 1 .*not memory of device"):
            ce.upload_device([[(Y8, sw), (C8, sw)]], "nv16", **corner)
        with pytest.raises(P.H264EError, match="plane 0 .*not inside one allocation|plane 0 .*not memory of device"):
            ce.upload_device([(PK8 + 2 * sw, 2 * sw)], "uyvy", **corner)
    finally:
        ce.close()
        for p in owned:
            L.H264E_dev_free(p)
