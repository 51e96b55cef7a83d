"""The HDR10 device input's cases, once for both places they run: the lane-loop emulation (tests/test_emu_tonemap_input.py) and the MI355X
(tests/test_gpu_tonemap_input.py).  Each of the two hands over a backend B that puts numpy arrays into its device memory:

    B.lib                       the library to load (None: the product)
    B.planes(planes, kind, signed)   2-D arrays -> one device array per plane.  kind "tight": contiguous; "padded": rows an odd number of
                                words apart, the first sample one word into the buffer; "view": every plane a row-strided view of a wider
                                array; "separate": every plane an allocation of its own that ends with the plane's last sample
    B.array(a)                  one contiguous array of any shape
    signed                      16-bit words as int16 instead of uint16 (the same bits)

Every comparison is equality of bytes: the slot with the model's slot (tests/tonemap_model.py, with the LIBRARY's tables), the stream with
the stream of the model's R'G'B' picture fed as "rgbp" to an encoder with the same colour."""
import ctypes as C
import re

import numpy as np
import pytest

import color_model as CM
import hbd_model as HM
import pkg
import tonemap_model as TM

GOP, QP = 30, 26
SIZES = [(16, 16), (18, 16), (34, 18), (66, 34), (64, 48)]          # 34 and 66: row tails of the 2-, 4- and 8-sample lanes
FORMATS = [("i420_16", 10), ("i420_16", 12), ("p010", 16), ("nv12_16", 10)]
KINDS = ["tight", "padded", "view", "separate"]
COLORS = [None, "bt709"]


def color_pair(color):
    return CM.NAMES[color] if color else (0, 0)


def source(B, frame, fmt, kind="tight", signed=False):
    """the frame (y, u, v) as upload_device(..., fmt) takes it"""
    y, u, v = frame
    if fmt in ("p010", "p016", "nv12_16"):
        return B.planes([y, TM.interleave(u, v)], kind, signed)
    if kind == "tight":                             # packed I420: one array
        return B.planes([np.concatenate([p.reshape(-1) for p in frame]).reshape(y.shape[0] * 3 // 2, y.shape[1])], kind, signed)[0]
    return B.planes([y, u, v], kind, signed)


def depth_kw(fmt, depth):
    return {} if fmt in ("p010", "p016") else dict(depth=depth)


def run_clip(B, w, h, n, put, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, n, **dict(dict(gop=GOP, qp=QP, lib=B.lib), **kw))
    try:
        put(ce)
        slots = ce.download()
        out, sizes, _ = ce.encode()
        return slots, out, sizes
    finally:
        ce.close()


def opts(color, tonemap=None):
    kw = {}
    if color:
        kw["color"] = color
    if tonemap is not None:
        kw["tonemap"] = tonemap
    return kw


def check_at_size(B, fmt, depth, frames, kind="tight", color=None, curve="hable", signed=False, stats=None):
    """slots and stream of the frames at the picture's size; returns (slots, stream)"""
    P = pkg.load_pkg()
    tm = {"transfer": "pq", "curve": curve}
    tables = P.tonemap_tables(tm, lib=B.lib)
    h, w = frames[0][0].shape
    model = np.stack([TM.slot(f, depth, tables, color_pair(color), stats) for f in frames])
    slots, got, sizes = run_clip(B, w, h, len(frames), lambda ce: ce.upload_device([source(B, f, fmt, kind, signed) for f in frames], fmt, **depth_kw(fmt, depth)),
                                 **opts(color, tm))
    assert np.array_equal(slots, model), "%s depth %d %s %s: the slot differs from the model" % (fmt, depth, kind, curve)
    rgb = [B.array(TM.rgb8(f, depth, tables)) for f in frames]
    slots8, want, want_sizes = run_clip(B, w, h, len(frames), lambda ce: ce.upload_device(rgb, "rgbp"), **opts(color))
    assert np.array_equal(slots8, model)
    assert got == want and sizes == want_sizes, "%s depth %d: the stream differs from that of the model's R'G'B' picture" % (fmt, depth)
    return slots, got


def check_window(B, fmt, depth, frames, dw, dh, crop=None, kind="tight", color=None, curve="hable"):
    """through a window: the model's tone-mapped crop through the I420 scale model, and through the existing "i420" path with src_size="""
    P = pkg.load_pkg()
    tm = {"transfer": "pq", "curve": curve}
    tables = P.tonemap_tables(tm, lib=B.lib)
    sh, sw = frames[0][0].shape
    n = len(frames)
    model = np.stack([TM.window_slot(f, depth, tables, dw, dh, crop, color_pair(color)) for f in frames])
    slots, got, sizes = run_clip(B, dw, dh, n, lambda ce: ce.upload_device([source(B, f, fmt, kind) for f in frames], fmt, src_size=(sw, sh), crop=crop,
                                                                           **depth_kw(fmt, depth)), **opts(color, tm))
    assert np.array_equal(slots, model), "%s depth %d window %r: the slot differs from the model" % (fmt, depth, crop)
    cuts = [TM.crop_frame(f, crop) for f in frames]
    ch, cw = cuts[0][0].shape
    mapped = [B.array(TM.slot(c, depth, tables, color_pair(color)).reshape(ch * 3 // 2, cw)) for c in cuts]
    slots8, want, want_sizes = run_clip(B, dw, dh, n, lambda ce: ce.upload_device(mapped, "i420", src_size=(cw, ch)), **opts(color))
    assert np.array_equal(slots8, slots) and got == want and sizes == want_sizes, "window %r: differs from the tone-mapped crop fed as i420" % (crop,)
    return slots, got


def at_size_cases():
    """every size with every format; the addressing, the colour, the curve and the sample type rotate through them"""
    out = []
    for i, (w, h) in enumerate(SIZES):
        for j, (fmt, depth) in enumerate(FORMATS):
            k = i * len(FORMATS) + j
            kind, color, curve = KINDS[(i + j) % 4], COLORS[(i + j // 2) % 2], TM.CURVES[k % 3]
            out.append(pytest.param(fmt, depth, w, h, kind, color, curve, bool(k & 1), id="%s-d%d-%dx%d-%s-%s-%s" % (fmt, depth, w, h, kind, color or "bt601", curve)))
    return out


def case_at_size(B, fmt, depth, w, h, kind, color, curve, signed):
    check_at_size(B, fmt, depth, [TM.picture(w, h, depth, t) for t in range(2)], kind, color, curve, signed)


def case_all_codes(B, curve):
    """all 1024 luma codes under chroma at the corners and the centre: every m, both clamps of step 2, both ends of the threshold search"""
    stats = {}
    check_at_size(B, "i420_16", 10, TM.all_codes_pictures(), "tight", "bt709" if curve != "clip" else None, curve, stats=stats)
    assert stats["m"] == set(range(1024)) and stats["below"] > 0 and stats["above"] > 0 and {0, 255} <= stats["out"]


WINDOWS = {"2to1": ((64, 48), (32, 24), None), "crop": ((64, 48), (16, 16), (2, 2, 36, 20)), "pure_crop": ((64, 48), (32, 24), (4, 6, 32, 24))}


def case_window(B, name, fmt, depth, kind, color, curve):
    (sw, sh), (dw, dh), crop = WINDOWS[name]
    frames = [TM.picture(sw, sh, depth, t) for t in range(2)]
    slots, got = check_window(B, fmt, depth, frames, dw, dh, crop, kind, color, curve)
    if name == "pure_crop":                         # ... which is the at-size result of the cropped planes
        cut = [tuple(np.ascontiguousarray(p) for p in TM.crop_frame(f, crop)) for f in frames]
        slots0, got0 = check_at_size(B, fmt, depth, cut, "tight", color, curve)
        assert np.array_equal(slots0, slots) and got0 == got


def case_frame_at_a_time(B, fmt, depth):
    """H264E_encode_device and H264E_encode_device_scaled against the clip encoder: the same bytes"""
    P = pkg.load_pkg()
    tm = {"transfer": "pq", "curve": "reinhard", "peak": 4000, "ref_white": 100}
    for (sw, sh), (dw, dh), crop in (((64, 48), (64, 48), None), ((64, 48), (32, 24), None), ((64, 48), (16, 16), (2, 2, 36, 20))):
        scaled = (sw, sh) != (dw, dh)
        win = dict(src_size=(sw, sh), crop=crop) if scaled else {}
        frames = [TM.picture(sw, sh, depth, t) for t in range(2)]
        _, want, want_sizes = run_clip(B, dw, dh, 2, lambda ce: ce.upload_device([source(B, f, fmt) for f in frames], fmt, **win, **depth_kw(fmt, depth)),
                                       tonemap=tm, color="bt709")
        e = P.Encoder(dw, dh, gop=GOP, qp=QP, lib=B.lib, color="bt709", tonemap=tm)
        try:
            parts = [e.encode_device(source(B, f, fmt, "padded" if scaled else "separate"), fmt, **win, **depth_kw(fmt, depth)) for f in frames]
            state = e.tonemap_state()
        finally:
            e.close()
        assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes
        surface = ((crop[2] * crop[3] if crop else sw * sh) * 3 // 2) if scaled else 0       # the window's size, only where a window was used
        assert state == (1, 4 * 2304, surface)


def case_ladder(B):
    """encode_ladder with tonemap="pq": two rungs of different size from one P010 source = the ladder of the tone-mapped 8-bit source"""
    P = pkg.load_pkg()
    sw, sh = 64, 48
    frames = [TM.picture(sw, sh, 16, t) for t in range(2)]
    tables = P.tonemap_tables("pq", lib=B.lib)
    rungs = [(64, 48, dict(qp=30)), (32, 24, dict(qp=26, tonemap={"curve": "hable"}))]
    got = P.encode_ladder([source(B, f, "p010") for f in frames], "p010", (sw, sh), rungs, gop=GOP, lib=B.lib, tonemap="pq", color="bt709")
    mapped = [B.array(TM.slot(f, 16, tables, CM.NAMES["bt709"]).reshape(sh * 3 // 2, sw)) for f in frames]
    want = P.encode_ladder(mapped, "i420", (sw, sh), [(w, h, dict(qp=o["qp"])) for w, h, o in rungs], gop=GOP, lib=B.lib, color="bt709")
    for (out, sizes, _), (out8, sizes8, _) in zip(got, want):
        assert out == out8 and sizes == sizes8 and len(out) > 0


def case_off_means_off(B):
    """an encoder that never switched it on and one that passed H264E_TONEMAP_OFF give the bytes of the "p010" path; nothing is allocated"""
    P = pkg.load_pkg()
    w, h = 64, 48
    frames = [TM.picture(w, h, 16, t) for t in range(2)]
    model = np.stack([HM.slot(f, "nv12_16", 16) for f in frames])
    _, want, want_sizes = run_clip(B, w, h, 2, lambda ce: ce.upload(model))
    for tm in (None, "off", {"transfer": "off", "curve": "clip", "peak": 4000}):
        ce = P.ClipEncoder(w, h, 2, gop=GOP, qp=QP, lib=B.lib, **opts(None, tm))
        try:
            ce.upload_device([source(B, f, "p010") for f in frames], "p010")
            assert np.array_equal(ce.download(), model)
            out, sizes, _ = ce.encode()
            assert out == want and sizes == want_sizes
            assert ce.tonemap_state() == (0, 0, 0)
            ce.upload_device([source(B, f, "p010") for f in frames], "p010", src_size=(w, h), crop=(0, 0, w, h))      # ... through the window path too
            assert np.array_equal(ce.download(), np.stack([HM.slot(f, "nv12_16", 16, w, h, (0, 0, w, h)) for f in frames])) and ce.tonemap_state() == (0, 0, 0)
        finally:
            ce.close()
        e = P.Encoder(w, h, gop=GOP, qp=QP, lib=B.lib, **opts(None, tm))
        try:
            parts = [e.encode_device(source(B, f, "p010"), "p010") for f in frames]
            assert b"".join(parts) == want and e.tonemap_state() == (0, 0, 0)
        finally:
            e.close()
    # on, then off again before the first frame: the p010 bytes; the table buffer stays, unused
    ce = P.ClipEncoder(w, h, 2, gop=GOP, qp=QP, lib=B.lib, tonemap="pq")
    try:
        ce.set_tonemap("off")
        ce.upload_device([source(B, f, "p010") for f in frames], "p010")
        assert np.array_equal(ce.download(), model) and ce.encode()[0] == want and ce.tonemap_state() == (0, 4 * 2304, 0)
    finally:
        ce.close()


BAD_PARAMETERS = [
    ((2, 0, 0.0, 0.0), "transfer 2"), ((-1, 0, 0.0, 0.0), "transfer -1"), ((1, 3, 0.0, 0.0), "curve 3"), ((1, -1, 0.0, 0.0), "curve -1"),
    ((1, 0, 100.0, 203.0), "peak_nits 100 "), ((1, 0, 10001.0, 0.0), "peak_nits 10001 "), ((1, 0, 150.0, 0.0), "peak_nits 150 "),
    ((1, 0, 0.0, 49.0), "ref_white_nits 49 "), ((1, 0, 0.0, 1001.0), "ref_white_nits 1001 "), ((1, 0, 0.0, 1500.0), "ref_white_nits 1500 "),
    ((1, 0, float("nan"), 0.0), "peak_nits -?nan is not finite"), ((1, 0, float("inf"), 0.0), "peak_nits inf is not finite"),
    ((1, 0, 0.0, float("nan")), "ref_white_nits -?nan is not finite"), ((1, 0, 0.0, float("-inf")), "ref_white_nits -inf is not finite"),
    ((0, 5, 0.0, 0.0), "curve 5"),
]


def case_refusals(B):
    """bad parameters, a call after the first frame and every frame that is not HDR10 while it is on: each with its text, with position
    and settings unchanged and nothing launched; the setting survives a rewind"""
    P = pkg.load_pkg()
    w, h, n = 32, 16, 2
    tm = {"transfer": "pq", "curve": "clip"}
    tables = P.tonemap_tables(tm, lib=B.lib)
    frames = [TM.picture(w, h, 10, t) for t in range(n)]
    big = [TM.picture(2 * w, 2 * h, 10, t) for t in range(n)]
    model = np.stack([TM.slot(f, 10, tables) for f in frames])
    L = P.load(B.lib)
    ycc, e1, e2, e3 = np.zeros(8, np.int32), np.zeros(1024, np.float32), np.zeros(1024, np.float32), np.zeros(256, np.float32)
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, lib=B.lib, tonemap=tm)
    e = P.Encoder(w, h, gop=GOP, qp=QP, lib=B.lib, tonemap=tm)
    try:
        state = ce.tonemap_state()
        assert state == (1, 4 * 2304, 0) and e.tonemap_state() == state
        for args, msg in BAD_PARAMETERS:
            assert L.H264E_clip_set_tonemap(ce.c, *args) == -1
            assert re.search("clip_set_tonemap: " + msg, L.H264E_last_error().decode()), (msg, L.H264E_last_error().decode())
            assert L.H264E_set_tonemap(e.persist, *args) == P.STATUS_BAD_PARAMETER
            assert re.search("^set_tonemap: " + msg, L.H264E_last_error().decode()), (msg, L.H264E_last_error().decode())
            assert L.H264E_tonemap_tables(*args, ycc.ctypes.data, e1.ctypes.data, e2.ctypes.data, e3.ctypes.data) == -1
            assert re.search("tonemap_tables: " + msg, L.H264E_last_error().decode())
            assert ce.tonemap_state() == state and e.tonemap_state() == state
        for bad in ("hlg", {"curve": "aces"}, {"transfer": "pq", "knee": 1}, 7):
            with pytest.raises(P.H264EError, match="tonemap"):
                ce.set_tonemap(bad)
        # every frame that is not HDR10 is refused by name while it is on; the slots keep what they held
        marker = np.arange(n * w * h * 3 // 2, dtype=np.uint32).astype(np.uint8).reshape(n, -1)
        ce.upload(marker)
        buf = B.array(np.zeros((3 * h, 2 * w), np.uint16))
        ptr = P.dev_frame(buf, "i420_16", 2 * w, 2 * h, depth=10)[0].plane[0]
        I420, NV12, D = P.DEV_FORMAT_I420, P.DEV_FORMAT_NV12, P.DEV_DEPTH
        cases = [(I420, "8-bit I420"), (NV12, "8-bit NV12"), (P.DEV_FORMAT_RGB, "RGB"), (P.DEV_FORMAT_RGBP, "RGBP"), (P.DEV_FORMAT_RGBP_F16, "RGBP of f16"),
                 (P.DEV_FORMAT_I422 | D(10), "4:2:2 I420"), (P.DEV_FORMAT_NV16 | D(16), "4:2:2 NV12"), (P.DEV_FORMAT_YUYV, "4:2:2 packed YUYV"),
                 (P.DEV_FORMAT_I444, "4:4:4 I420"), (P.DEV_FORMAT_I444 | D(10), "4:4:4 I420"), (I420 | D(9), "I420 of depth 9"), (NV12 | D(9), "NV12 of depth 9")]
        for code, name in cases:
            d = P.DevFrame(format=code, pixel_bytes=3)
            for k in range(3):
                d.plane[k], d.stride[k] = ptr, 8 * w
            data, size = C.c_void_p(), C.c_int()
            msg = "format %d is %s, but tone mapping is on" % (code, re.escape(name))
            for win in (None, P.dev_window((2 * w, 2 * h), None, w, h)[0]):
                if win is None:
                    assert L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) != 0
                    text = L.H264E_last_error().decode()
                    assert L.H264E_encode_device(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(data), C.byref(size)) != 0
                else:
                    assert L.H264E_clip_upload_device_scaled(ce.c, 0, 1, C.byref(d), C.byref(win)) != 0
                    text = L.H264E_last_error().decode()
                    assert L.H264E_encode_device_scaled(e.persist, e.scratch, C.byref(e.rp), C.byref(d), C.byref(win), C.byref(data), C.byref(size)) != 0
                assert re.search(msg, text), (msg, text)
                assert re.search(msg, L.H264E_last_error().decode()), (msg, L.H264E_last_error().decode())
                assert np.array_equal(ce.download(), marker), "a refused call wrote the slot: " + name
                assert ce.tonemap_state() == state and e.tonemap_state() == state
        nxt, up = C.c_int(-1), C.c_int(-1)
        L.H264E_clip_position(ce.c, C.byref(nxt), C.byref(up))
        assert nxt.value == 0
        # ... and both encoders go on: the frames are taken and tone-mapped
        ce.upload_device([source(B, f, "i420_16", "padded") for f in frames], "i420_16", depth=10)
        assert np.array_equal(ce.download(), model)
        want = ce.encode()[0]
        parts = [e.encode_device(source(B, f, "i420_16"), "i420_16", depth=10) for f in frames]
        assert b"".join(parts) == want
        # after the first frame the call is refused, and the setting stays
        assert L.H264E_clip_set_tonemap(ce.c, 0, 0, 0.0, 0.0) == -1
        assert re.search("clip_set_tonemap: only at frame 0 .*not at frame %d" % n, L.H264E_last_error().decode())
        assert L.H264E_set_tonemap(e.persist, 0, 0, 0.0, 0.0) == P.STATUS_BAD_PARAMETER
        assert re.search("set_tonemap: only before the first frame .%d encoded" % n, L.H264E_last_error().decode())
        assert ce.tonemap_state() == state and e.tonemap_state() == state
        # a rewind keeps it: the same frames through a window give the window's bytes, and the call is accepted again
        L.H264E_clip_rewind(ce.c)
        assert ce.tonemap_state() == state
        ce.upload_device([source(B, f, "i420_16") for f in big], "i420_16", depth=10, src_size=(2 * w, 2 * h))
        assert np.array_equal(ce.download(), np.stack([TM.window_slot(f, 10, tables, w, h) for f in big]))
        assert ce.tonemap_state() == (1, 4 * 2304, 2 * w * 2 * h * 3 // 2)
        ce.set_tonemap({"curve": "hable"})
        ce.upload_device([source(B, f, "i420_16") for f in frames], "i420_16", depth=10)
        assert np.array_equal(ce.download(), np.stack([TM.slot(f, 10, P.tonemap_tables("pq", lib=B.lib)) for f in frames]))
    finally:
        ce.close()
        e.close()
