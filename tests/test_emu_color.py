"""CPU: colour and frame rate (H264E_set_color / H264E_set_frame_rate and their clip forms) in the lane-loop emulation of the kernels
(tests/emu), both lane orders.  tests/color_model.py is the definition: the matrix rows, and the VUI an SPS must carry.

  - with nothing set, or set back to (0, 0) and 0/0, slots and streams are today's;
  - the input slots hold exactly the model's bytes for each of the three new rows: interleaved RGB of 3 and 4 bytes and planar RGB, at the
    picture's size and (planar) through a window, noise frames and the eight corner colours;
  - a signalled stream is the oracle's stream for the model's frames with nothing but the SPSs changed, and every SPS parses to the
    oracle's fields plus exactly the VUI asked for: clip encoder, per-frame encoder, and I420 input (where the call only signals);
  - with rate control the clip encoder's stream is still the concatenation of the per-frame encoder's frames;
  - what is refused is refused with a message that names the value, changes nothing, and the encoder goes on to the right stream.

Every comparison is byte equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clips
import color_model as CM
import ingest_model
import oracle_lib
import pkg
import rgbp_model
from test_emu_rgbp_input import DevMem, source

HERE = os.path.dirname(os.path.abspath(__file__))
LIBS = {"fwd": pkg.EMU_LIB, "rev": pkg.EMU_REV_LIB}
APP = os.path.join(HERE, "emu", "build", "encode_app_emu")
WINDOWS = [((128, 96), None, (64, 48)), ((32, 32), None, (2, 2)), ((200, 120), (14, 6, 180, 108), (68, 36))]


@pytest.fixture(scope="module", autouse=True)
def _emu():
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu")], stdout=subprocess.DEVNULL)


def frames_for(w, h):
    """(3, 3, h, w): two noise frames and the eight corner colours"""
    return np.concatenate([rgbp_model.noisy_clip(w, h, 2), CM.corner_frame(w, h)[None]])


def put_rgb(mem, chw, pb, pad, offset):
    """the planar frame as interleaved pixels of pb bytes in device memory (a fourth byte holds 0x5A and must be ignored)"""
    _, h, w = chw.shape
    hwc = np.full((h, w, pb), 0x5A, np.uint8)
    hwc[:, :, :3] = chw.transpose(1, 2, 0)
    ptr, stride = mem.put(hwc.reshape(h, w * pb), w * pb + pad, offset)
    return type("Dev", (), {"__cuda_array_interface__": dict(shape=(h, w, pb), strides=(stride, pb, 1), typestr="|u1", data=(ptr, False), version=3)})()


def slots_of(lib, w, h, frames, feed, **kw):
    P = pkg.load_pkg()
    ce = P.ClipEncoder(w, h, len(frames), gop=30, qp=26, lib=lib, **kw)
    try:
        feed(ce)
        return ce.download()
    finally:
        ce.close()


# ---------------------------------------------------------------- the default


@pytest.mark.parametrize("how", ["no call", "zeros", "set and cleared"])
def test_default_slots_and_streams_are_todays(how):
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    chw = rgbp_model.clip(w, h, n)
    model = np.stack([rgbp_model.to_i420(f) for f in chw])
    want, want_sizes = oracle_lib.encode_clip(model, w, h, gop=2, qp=26)

    def prepare(e):
        if how == "zeros":
            e.set_color((0, 0))
            e.set_frame_rate((0, 0))
        if how == "set and cleared":
            e.set_color("bt709-full")
            e.set_frame_rate((30000, 1001))
            e.set_color((0, 0))
            e.set_frame_rate((0, 0))

    mem = DevMem(pkg.EMU_LIB)
    try:
        for kind in ("rgb", "rgbp", "i420"):
            ce = P.ClipEncoder(w, h, n, gop=2, qp=26, lib=pkg.EMU_LIB)
            e = P.Encoder(w, h, gop=2, qp=26, lib=pkg.EMU_LIB)
            try:
                prepare(ce)
                prepare(e)
                if kind == "rgb":
                    srcs = [put_rgb(mem, f, 3, 1, 1) for f in chw]
                    ce.upload_device(srcs, "rgb")
                    parts = [e.encode_device(s, "rgb") for s in srcs]
                elif kind == "rgbp":
                    srcs = [source(mem, f, "chw_padded") for f in chw]
                    ce.upload_device(srcs, "rgbp")
                    parts = [e.encode_device(s, "rgbp") for s in srcs]
                else:
                    ce.upload(model)
                    parts = [e.encode(f) for f in model]
                assert np.array_equal(ce.download(), model)
                out, sizes, _ = ce.encode()
            finally:
                ce.close()
                e.close()
            assert out == want and sizes == want_sizes and b"".join(parts) == want, kind
    finally:
        mem.close()


# ---------------------------------------------------------------- slot bytes against the model


@pytest.mark.parametrize("w,h", [(2, 2), (64, 48), (202, 122)])
@pytest.mark.parametrize("matrix,full", CM.NEW_ROWS)
def test_plain_slots_hold_the_models_bytes(matrix, full, w, h):
    frames = frames_for(w, h)
    want = np.stack([CM.to_i420(f, matrix, full) for f in frames])
    assert not np.array_equal(want, np.stack([CM.to_i420(f) for f in frames]))
    for lib, kind, arg in (("fwd", "rgb", (3, 1, 1)), ("rev", "rgb", (4, 4, 2)), ("rev", "rgb", (3, 0, 0)), ("fwd", "rgbp", "padded"), ("rev", "rgbp", "chw_padded"),
                           ("fwd", "rgbp", "separate")):
        mem = DevMem(LIBS[lib])
        try:
            srcs = [put_rgb(mem, f, *arg) if kind == "rgb" else source(mem, f, arg) for f in frames]
            got = slots_of(LIBS[lib], w, h, frames, lambda ce: ce.upload_device(srcs, kind), color=(matrix, full))
        finally:
            mem.close()
        assert np.array_equal(got, want), "slot contents differ from the model (%s %r, %s)" % (kind, arg, lib)


@pytest.mark.parametrize("src,crop,dst", WINDOWS)
@pytest.mark.parametrize("matrix,full", CM.NEW_ROWS)
def test_windowed_slots_hold_the_models_bytes(matrix, full, src, crop, dst):
    (sw, sh), (w, h) = src, dst
    frames = frames_for(sw, sh)
    want = np.stack([CM.scale_to_i420(f, w, h, crop, matrix, full) for f in frames])
    assert not np.array_equal(want, np.stack([CM.scale_to_i420(f, w, h, crop) for f in frames]))
    for lib, layout in (("fwd", "padded"), ("rev", "chw"), ("fwd", "chw_padded")):
        mem = DevMem(LIBS[lib])
        try:
            srcs = [source(mem, f, layout) for f in frames]
            got = slots_of(LIBS[lib], w, h, frames, lambda ce: ce.upload_device(srcs, "rgbp", src_size=src, crop=crop), color=(matrix, full))
        finally:
            mem.close()
        assert np.array_equal(got, want), "slot contents differ from the model (%s, %s)" % (layout, lib)


# ---------------------------------------------------------------- streams

STREAM_CASES = [("bt709", None), ("bt601-full", None), ("bt709-full", None), (None, 25), (None, (30000, 1001)), ("bt709", (30, 1)), ("bt709-full", (30000, 1001))]


def fps_of(fps):
    return None if fps is None else (fps, 1) if isinstance(fps, int) else tuple(fps)


@pytest.mark.parametrize("lib", ["fwd", "rev"])
@pytest.mark.parametrize("color,fps", STREAM_CASES)
def test_streams_differ_from_the_oracles_in_the_sps_alone(color, fps, lib):
    P = pkg.load_pkg()
    w, h, n = 64, 48, 4
    matrix, full = CM.NAMES[color] if color else (0, 0)
    chw = rgbp_model.clip(w, h, n)
    model = np.stack([CM.to_i420(f, matrix, full) for f in chw])
    want, _ = oracle_lib.encode_clip(model, w, h, gop=2, qp=26)
    i420 = clips.make("synth", w, h, n)
    want_yuv, _ = oracle_lib.encode_clip(i420, w, h, gop=2, qp=26)
    kw = dict(gop=2, qp=26, lib=LIBS[lib], color=color, fps=fps)
    mem = DevMem(LIBS[lib])
    try:
        # the clip encoder, planar RGB
        ce = P.ClipEncoder(w, h, n, **kw)
        try:
            ce.upload_device([source(mem, f, "chw") for f in chw], "rgbp")
            assert np.array_equal(ce.download(), model)
            got_clip, sizes, _ = ce.encode()
        finally:
            ce.close()
        # the per-frame encoder, interleaved RGB
        e = P.Encoder(w, h, **kw)
        try:
            parts = [e.encode_device(put_rgb(mem, f, 3, 0, 0), "rgb") for f in chw]
        finally:
            e.close()
        # I420 input, host and device: the call only signals
        ce = P.ClipEncoder(w, h, n, **kw)
        e = P.Encoder(w, h, **kw)
        try:
            ce.upload(i420)
            assert np.array_equal(ce.download(), i420)
            got_yuv, _, _ = ce.encode()
            y = [mem.put(f[: w * h].reshape(h, w)) for f in i420]
            u = [mem.put(f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2)) for f in i420]
            v = [mem.put(f[w * h * 5 // 4:].reshape(h // 2, w // 2)) for f in i420]
            ce.upload_device(list(zip(y, u, v)), "i420")
            assert np.array_equal(ce.download(), i420)
            parts_yuv = [e.encode(f) for f in i420]
        finally:
            ce.close()
            e.close()
    finally:
        mem.close()
    assert b"".join(parts) == got_clip and sum(sizes) == len(got_clip) and [len(p) for p in parts] == sizes
    assert b"".join(parts_yuv) == got_yuv
    for got, ref in ((got_clip, want), (got_yuv, want_yuv)):
        spss = CM.compare_streams(got, ref, matrix, full, fps_of(fps))
        assert len(spss) == 2 and spss[0] == spss[1]
    if fps_of(fps) == (30, 1):
        # num_units_in_tick = 1 is 00 00 00 01 inside the payload: it must come out escaped, and the escaped SPS still holds no start code
        assert b"\x00\x00\x03" in spss[0] and b"\x00\x00\x01" not in spss[0] and b"\x00\x00\x00" not in spss[0]


def test_rate_control_clip_equals_per_frame_with_longer_parameter_sets():
    """the standing invariant: H264E_clip_encode == the concatenation of H264E_encode, the bytes rate control counts now including the VUI"""
    P = pkg.load_pkg()
    w, h, n = 176, 144, 8
    c = clips.make("synth", w, h, n)
    kw = dict(gop=4, kbps=300, lib=pkg.EMU_LIB, color="bt709", fps=(30000, 1001))
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
    plain, _ = oracle_lib.encode_clip(c, w, h, gop=4, kbps=300)
    assert CM.split_annexb(out)[2] == CM.split_annexb(plain)[2]        # the first key frame is coded before any byte has been counted


def test_nalu_callback_receives_the_sps_of_the_stream():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 3
    c = clips.make("synth", w, h, n)
    seen = []
    cb = P.binding.NALU_CB(lambda data, size, token: seen.append(C.string_at(data, size)))
    e = P.Encoder(w, h, gop=2, qp=26, lib=pkg.EMU_LIB, color="bt601-full", fps=(30, 1))
    try:
        e.rp.nalu_callback = cb
        out = b"".join(e.encode(f) for f in c)
    finally:
        e.close()
    assert seen == CM.split_annexb(out)
    spss = [x for x in seen if CM.is_sps(x)]
    assert len(spss) == 2 and CM.parse_sps(spss[0])["vui"] == CM.vui_fields(6, 1, (30, 1))


# ---------------------------------------------------------------- refusals, rewind, several clips

BAD_COLORS = [((2, 0), "matrix 2"), ((5, 0), "matrix 5"), ((9, 1), "matrix 9"), ((-1, 0), "matrix -1"), ((0, 1), "full_range 1"), ((1, 2), "full_range 2")]
BAD_FPS = [((0, 1), "numerator 0"), ((1, 0), "denominator 0"), ((-1, 1), "numerator -1"), (((1 << 30) + 1, 1), "numerator %d" % ((1 << 30) + 1))]


def test_refusals_change_nothing():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 4
    chw = rgbp_model.clip(w, h, n)
    model = np.stack([CM.to_i420(f, 1, 0) for f in chw])
    plain, _ = oracle_lib.encode_clip(model, w, h, gop=2, qp=26)
    mem = DevMem(pkg.EMU_LIB)
    ce = P.ClipEncoder(w, h, n, gop=2, qp=26, lib=pkg.EMU_LIB, color="bt709", fps=(1 << 30, 0x7fffffff))
    e = P.Encoder(w, h, gop=2, qp=26, lib=pkg.EMU_LIB, color="bt709", fps=(1 << 30, 0x7fffffff))
    try:
        srcs = [source(mem, f, "chw") for f in chw]
        for enc, status in ((ce, -1), (e, P.STATUS_BAD_PARAMETER)):
            clip = enc is ce
            for (bad, text) in BAD_COLORS:
                with pytest.raises(P.H264EError, match=text):
                    enc.set_color(bad)
                call = enc.L.H264E_clip_set_color if clip else enc.L.H264E_set_color
                assert call(enc.c if clip else enc.persist, *bad) == status
            for (bad, text) in BAD_FPS:
                with pytest.raises(P.H264EError, match=text):
                    enc.set_frame_rate(bad)
                call = enc.L.H264E_clip_set_frame_rate if clip else enc.L.H264E_set_frame_rate
                assert call(enc.c if clip else enc.persist, *bad) == status
        for bad in ("bt2020", 7, None):
            with pytest.raises(P.H264EError):
                ce.set_color(bad)
        for bad in (29.97, "30", (30, 1, 1)):
            with pytest.raises(P.H264EError):
                ce.set_frame_rate(bad)
        # after the first frame: refused, position and settings as they were
        ce.upload_device(srcs[:2], "rgbp")
        first, _, _ = ce.encode()
        parts = [e.encode_device(srcs[0], "rgbp")]
        nxt = C.c_int()
        for enc in (ce, e):
            with pytest.raises(P.H264EError, match="frame"):
                enc.set_color("bt601")
            with pytest.raises(P.H264EError, match="frame"):
                enc.set_frame_rate(25)
            with pytest.raises(P.H264EError, match="frame"):
                enc.set_color((0, 0))
        ce.L.H264E_clip_position(ce.c, C.byref(nxt), None)
        assert nxt.value == 2
        ce.upload_device(srcs[2:], "rgbp", first=2)
        assert np.array_equal(ce.download(), model)
        rest, _, _ = ce.encode(rewind=False)
        parts += [e.encode_device(s, "rgbp") for s in srcs[1:]]
    finally:
        ce.close()
        e.close()
        mem.close()
    assert first + rest == b"".join(parts)
    CM.compare_streams(first + rest, plain, 1, 0, (1 << 30, 0x7fffffff))


def test_rewind_keeps_the_setting_and_every_clip_has_its_own():
    P = pkg.load_pkg()
    w, h, n = 64, 48, 4
    chw = rgbp_model.clip(w, h, n)
    mem = DevMem(pkg.EMU_LIB)
    a = P.ClipEncoder(w, h, n, gop=2, qp=26, lib=pkg.EMU_LIB, color="bt709", fps=30)
    b = P.ClipEncoder(w, h, n, gop=2, qp=26, lib=pkg.EMU_LIB, color="bt601-full")
    try:
        srcs = [source(mem, f, "chw") for f in chw]
        a.upload_device(srcs, "rgbp")
        b.upload_device(srcs, "rgbp")
        one, _, _ = a.encode()
        again, _, _ = a.encode()                        # rewinds
        a.L.H264E_clip_rewind(a.c)
        a.set_frame_rate((0, 0))                        # at frame 0 again: allowed
        no_fps, _, _ = a.encode(rewind=False)
        a.L.H264E_clip_rewind(a.c)
        a.set_frame_rate(30)
        ra, rb = P.ClipEncoder.encode_multi([a, b])
        alone, _, _ = b.encode()
    finally:
        a.close()
        b.close()
        mem.close()
    want_a, _ = oracle_lib.encode_clip(np.stack([CM.to_i420(f, 1, 0) for f in chw]), w, h, gop=2, qp=26)
    want_b, _ = oracle_lib.encode_clip(np.stack([CM.to_i420(f, 6, 1) for f in chw]), w, h, gop=2, qp=26)
    assert one == again == ra[0] and rb[0] == alone
    CM.compare_streams(one, want_a, 1, 0, (30, 1))
    CM.compare_streams(no_fps, want_a, 1, 0, None)
    CM.compare_streams(alone, want_b, 6, 1, None)


# ---------------------------------------------------------------- the CLI


@pytest.mark.parametrize("gop", [1, 30])
def test_cli_signals_on_both_paths(tmp_path, gop):
    """--colour / --fps on a YUV file: the reference's recorded stream with only the SPS replaced"""
    w, h, n = 64, 48, 4
    c = clips.make("synth", w, h, n)
    yuv = tmp_path / ("app_%dx%d.yuv" % (w, h))
    c.tofile(yuv)
    golden = open(os.path.join(HERE, "golden", "synth_64x48_qp_26_gop_%d.264" % gop), "rb").read()
    for extra in (["--clip", "0"], ["--clip", "1"]):
        out = tmp_path / "o.264"
        r = subprocess.run([APP, "--input", str(yuv), "--output", str(out), "--qp", "26", "--gop", str(gop), "--colour", "bt709", "--fps", "30000/1001"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        spss = CM.compare_streams(out.read_bytes(), golden, 1, 0, (30000, 1001))
        assert len(spss) == (n if gop == 1 else 1)
    for bad in (["--colour", "bt2020"], ["--fps", "30/0"], ["--fps", "x"]):
        r = subprocess.run([APP, "--input", str(yuv), "--output", str(tmp_path / "bad.264")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "ERROR" in r.stdout
