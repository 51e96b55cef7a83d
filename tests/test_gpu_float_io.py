"""GPU: float planar RGB device frames on the MI355X (H264E_DEV_FORMAT_RGBP | H264E_DEV_SAMPLE_F16 / _BF16 / _F32:
h264e_ingest_float_kernel, h264e_scale_rgb_float_kernel and h264e_egress_float_kernel) with torch CUDA tensors of the three dtypes.

  - way in: the input slots against the numpy model of the quantised frame (tests/float_model.py, tests/rgbp_model.py), against the
    two-step path a caller writes today (torch quantise, then "rgbp"), and the streams against the oracle -- tiny and ragged pictures, a
    row that crosses the 256-lane block, windows, all 65536 bit patterns of the 16-bit types, the float32 edge set, views;
  - way out: bit for bit (read_recon_device("rgbp").float() / 255).to(dtype), strided and sliced out=, and out=None.  The expression is
    evaluated by torch on the HOST (reference() below): there float32 division is IEEE, the definition.  Evaluated on the device, this
    torch build divides by a constant without correct rounding and is one ulp off for some float32 values (float16 and bfloat16 hide
    it), which is exactly what the definition rules out;
  - ordering against a producer's stream; the refusals (host memory, a plane a gigabyte past its allocation, misaligned planes) before
    any launch; encode_ladder from a float source.

Every comparison is equality of bytes."""
import ctypes as C
import re

import numpy as np
import pytest

import clips
import float_model as FM
import oracle_lib
import pkg
import rgbp_model as M

pytestmark = pytest.mark.gpu
GOP, QP = 30, 26


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


def dtype_of(torch, kind):
    return {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[kind]


def tensor(torch, bits, kind):
    """the bit patterns (numpy, any shape) as a CUDA tensor of the kind's dtype"""
    signed = np.ascontiguousarray(bits, FM.BITS[kind]).view(np.int16 if FM.BYTES[kind] == 2 else np.int32)
    return torch.from_numpy(signed.copy()).cuda().view(dtype_of(torch, kind))


def bits_of(torch, t, kind):
    """the bit patterns of a tensor (numpy)"""
    return t.contiguous().view(torch.int16 if FM.BYTES[kind] == 2 else torch.int32).cpu().numpy().view(FM.BITS[kind])


def source(torch, bits, kind, layout):
    """what upload_device(..., "rgbp_<kind>" | "rgbpf") takes for one (3, h, w) frame of bit patterns"""
    _, h, w = bits.shape
    t = tensor(torch, bits, kind)
    if layout == "chw":
        return t
    if layout == "separate":                # three tensors
        return [t[c].clone() for c in range(3)]
    if layout == "chw_slice":               # channels 1..3 of a [4, h, w] tensor
        big = torch.full((4, h, w), 0.25, dtype=t.dtype, device="cuda")
        big[1:].copy_(t)
        return big[1:]
    if layout == "chw_rows":                # every other row and a column window that starts at an odd sample: rows at 2 (mod 4) byte addresses for 16-bit samples
        big = torch.full((3, 2 * h, w + 7), 0.25, dtype=t.dtype, device="cuda")
        v = big[:, 1::2, 3:3 + w]
        v.copy_(t)
        assert not v.is_contiguous() and v.stride() == (2 * h * (w + 7), 2 * (w + 7), 1)
        return v
    raise ValueError(layout)


def reference(torch, u8, kind):
    """(u8.float() / 255).to(dtype) with the IEEE division of the host, back on the device"""
    return (u8.cpu().float() / 255).to(dtype_of(torch, kind)).cuda()


def two_step(torch, t):
    """what a caller writes today in front of "rgbp" """
    return torch.nan_to_num((t.float() * 255).round().clamp(0, 255), nan=0).to(torch.uint8)


def slots(P, frames, fmt, dw, dh, src_size=None, crop=None):
    ce = P.ClipEncoder(dw, dh, len(frames), gop=GOP, qp=QP)
    try:
        ce.upload_device(frames, fmt, src_size=src_size, crop=crop)
        return ce.download()
    finally:
        ce.close()


def check_way_in(P, torch, kind, frames, layout, dw, dh, src_size=None, crop=None, stream=True):
    quantised = [FM.quantise(f, kind) for f in frames]
    model = np.stack([M.to_i420(q) if src_size is None else M.scale_to_i420(q, dw, dh, crop) for q in quantised])
    src = [source(torch, f, kind, layout) for f in frames]
    got = slots(P, src, FM.FORMAT[kind], dw, dh, src_size, crop)
    assert np.array_equal(got, model), "%s %s: slot contents differ from the model of the quantised frame" % (kind, layout)
    assert np.array_equal(slots(P, src, "rgbpf", dw, dh, src_size, crop), model), "%s %s: fmt 'rgbpf' differs" % (kind, layout)
    # the two-step path: torch quantises, "rgbp" takes the bytes
    u8 = [two_step(torch, s) if layout != "separate" else [two_step(torch, p) for p in s] for s in src]
    for q, t in zip(quantised, u8):
        assert np.array_equal(q, (t if layout != "separate" else torch.stack(t)).cpu().numpy()), "%s: torch's quantiser is not the model's" % kind
    assert np.array_equal(slots(P, u8, "rgbp", dw, dh, src_size, crop), got), "%s %s: the float path and torch quantise + 'rgbp' differ" % (kind, layout)
    if not stream:
        return
    want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=GOP, qp=QP)
    ce = P.ClipEncoder(dw, dh, len(frames), gop=GOP, qp=QP)
    ce.upload_device(src, FM.FORMAT[kind], src_size=src_size, crop=crop)
    out, sizes, _ = ce.encode()
    ce.close()
    assert (out, sizes) == (want, want_sizes), "%s %s: the clip stream differs from the oracle's for the quantised frames" % (kind, layout)
    e = P.Encoder(dw, dh, gop=GOP, qp=QP)
    parts = [e.encode_device(s, "rgbpf", src_size=src_size, crop=crop) for s in src]
    e.close()
    assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes, "%s %s: the frame-at-a-time stream differs" % (kind, layout)


# ---------------------------------------------------------------- way in

LAYOUTS = ["chw", "chw_rows", "separate", "chw_slice"]


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("w,h", [(2, 2), (6, 4), (1030, 4), (64, 48)])
def test_plain_slot_and_streams(P, torch, w, h, kind):
    i = FM.KINDS.index(kind) + [2, 6, 1030, 64].index(w)
    check_way_in(P, torch, kind, [FM.ramp_picture(w, h, kind, t) for t in range(2)], LAYOUTS[i % 4], w, h)


WINDOWS = {"2to1": ((128, 96), (64, 48), None), "crop_and_scale": ((200, 120), (66, 50), (2, 4, 198, 116)), "pure_crop": ((128, 96), (64, 48), (64, 48, 64, 48))}


@pytest.mark.parametrize("kind", FM.KINDS)
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_window_slot_and_streams(P, torch, name, kind):
    (sw, sh), (dw, dh), crop = WINDOWS[name]
    i = FM.KINDS.index(kind) + sorted(WINDOWS).index(name)
    check_way_in(P, torch, kind, [FM.ramp_picture(sw, sh, kind, t) for t in range(2)], LAYOUTS[(i + 1) % 4], dw, dh, (sw, sh), crop)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_all_16_bit_patterns(P, torch, kind):
    """NaNs, infinities, denormals and negative values among them; also through a 1:1 window (the scaler's loads)"""
    pic = FM.all_patterns_picture()
    check_way_in(P, torch, kind, [pic], "chw", 256, 256, stream=False)
    check_way_in(P, torch, kind, [pic], "chw_rows", 256, 256, (256, 256), (0, 0, 256, 256), stream=False)


def test_f32_edge_set(P, torch):
    pic = FM.f32_edge_picture()
    h, w = pic.shape[1:]
    check_way_in(P, torch, "f32", [pic], "chw_rows", w, h, stream=False)
    check_way_in(P, torch, "f32", [pic], "chw", w, h, (w, h), (0, 0, w, h), stream=False)


# ---------------------------------------------------------------- way out


@pytest.fixture(scope="module")
def encoded(P, torch):
    """one clip at a low QP over the whole byte range, full-range colour: its 8-bit planar RGB holds every value"""
    w, h, n = 70, 36, 2
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=4, color="bt601-full")
    ce.upload(clips.noise(w, h, n))
    ce.encode()
    yield ce, w, h, n
    ce.close()


@pytest.mark.parametrize("kind", FM.KINDS)
def test_way_out_is_the_torch_expression_bit_for_bit(P, torch, encoded, kind):
    ce, w, h, n = encoded
    dt = dtype_of(torch, kind)
    seen = np.zeros(256, bool)
    for f in range(n):
        u8 = ce.read_recon_device(f, "rgbp")
        seen[np.unique(u8.cpu().numpy())] = True
        want = reference(torch, u8, kind)
        assert np.array_equal(bits_of(torch, want, kind), FM.dequantise(u8.cpu().numpy(), kind)), "torch's expression is not the model's"
        # out=None: a fresh (3, h, w) tensor of the dtype
        got = ce.read_recon_device(f, FM.FORMAT[kind])
        assert got.dtype == dt and tuple(got.shape) == (3, h, w) and got.is_contiguous()
        assert np.array_equal(bits_of(torch, got, kind), bits_of(torch, want, kind))
        # a strided view: every other row and a column window at an odd sample of a sentinel-filled tensor
        big = tensor(torch, np.full((3, 2 * h, w + 7), 0x5A5A5A5A if kind == "f32" else 0x5A5A, FM.BITS[kind]), kind)
        view = big[:, 1::2, 3:3 + w]
        assert ce.read_recon_device(f, "rgbpf", out=view) is view
        assert np.array_equal(bits_of(torch, view, kind), bits_of(torch, want, kind))
        rest = bits_of(torch, big, kind).copy()
        rest[:, 1::2, 3:3 + w] = rest[0, 0, 0]
        assert (rest == rest[0, 0, 0]).all(), "samples outside the rows were written"
        # a channel slice, and three separate planes
        four = torch.zeros((4, h, w), dtype=dt, device="cuda")
        ce.read_recon_device(f, FM.FORMAT[kind], out=four[1:])
        assert np.array_equal(bits_of(torch, four[1:], kind), bits_of(torch, want, kind)) and (four[0] == 0).all()
        planes = [torch.zeros((h, w), dtype=dt, device="cuda") for _ in range(3)]
        ce.read_recon_device(f, "rgbpf", out=planes)
        assert np.array_equal(bits_of(torch, torch.stack(planes), kind), bits_of(torch, want, kind))
    assert seen.all(), "the 8-bit planes miss the values %s" % np.flatnonzero(~seen)


def test_way_out_defaults_and_frame_at_a_time(P, torch):
    w, h = 64, 48
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    e.encode(clips.noise(w, h, 1)[0])
    u8 = e.read_recon_device("rgbp")
    got = e.read_recon_device("rgbpf")                                  # out=None: float32
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, h, w)
    assert torch.equal(got, reference(torch, u8, "f32"))
    for kind in ("f16", "bf16"):
        assert torch.equal(e.read_recon_device(FM.FORMAT[kind]), reference(torch, u8, kind))
    with pytest.raises(P.H264EError, match="float16, bfloat16 or float32 samples.*uint8"):
        e.read_recon_device("rgbpf", out=u8)
    with pytest.raises(P.H264EError, match="takes float16 samples, not torch.float32"):
        e.read_recon_device("rgbp_f16", out=got)
    e.close()


# ---------------------------------------------------------------- ordering


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """torch writes the float source on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer and trashed as soon as the call returns; the reconstruction is read into a tensor that the side stream still fills"""
    (sw, sh), (dw, dh), n, kind = (256, 128), (128, 64), 2, "f16"
    frames = [FM.ramp_picture(sw, sh, kind, t) for t in range(n)]
    plain = np.stack([M.to_i420(FM.quantise(f, kind)) for f in frames])
    scaled = np.stack([M.scale_to_i420(FM.quantise(f, kind), dw, dh) for f in frames])
    staged = [tensor(torch, f, kind) for f in frames]
    frame = torch.zeros((3, sh, sw), dtype=torch.float16, device="cuda")
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
                frame.copy_(staged[i])                  # the producer, on stream s
                ce.upload_device([frame], "rgbpf", first=i, **kw)       # torch's current stream is the producer
                frame.fill_(0.5)
        got_plain, got_scaled = a.download(), b.download()
        a.encode()
        out = torch.empty((3, sh, sw), dtype=torch.float16, device="cuda")
        for _ in range(10):
            busy = busy @ busy * 1e-4
        out.fill_(2.0)                                  # still queued when the reconstruction is asked for
        a.read_recon_device(n - 1, "rgbpf", out=out)
        want = reference(torch, a.read_recon_device(n - 1, "rgbp"), "f16")
    torch.cuda.synchronize()
    a.close()
    b.close()
    assert np.array_equal(got_plain, plain), "the ingest did not wait for the producer's stream, or read the frame after the call had returned"
    assert np.array_equal(got_scaled, scaled), "the scaler did not wait for the producer's stream, or read the frame after the call had returned"
    assert torch.equal(out, want), "the egress did not wait for the stream that still wrote its destination"


# ---------------------------------------------------------------- refusals


def test_refusals_before_any_launch(P, torch):
    """host memory, a plane a gigabyte past its allocation, misaligned pointers and strides, short strides, a sample type on another
    layout: refused by both entry points and both directions without a launch; then the encoders go on working"""
    (sw, sh), (dw, dh), n, kind = (128, 96), (64, 48), 2, "f32"
    big, small = [FM.ramp_picture(sw, sh, kind, t) for t in range(n)], [FM.ramp_picture(dw, dh, kind, t) for t in range(n)]
    want_plain = oracle_lib.encode_clip(np.stack([M.to_i420(FM.quantise(f, kind)) for f in small]), dw, dh, gop=GOP, qp=QP)[0]
    want_scaled = oracle_lib.encode_clip(np.stack([M.scale_to_i420(FM.quantise(f, kind), dw, dh) for f in big]), dw, dh, gop=GOP, qp=QP)[0]
    good_big, good_small = source(torch, big[0], kind, "separate"), source(torch, small[0], kind, "separate")
    host_big, host_small = np.ascontiguousarray(big[0]), np.ascontiguousarray(small[0])
    torch.cuda.synchronize()
    far = 1 << 30                                                       # rows a gigabyte apart leave any segment of torch's allocator
    ce = P.ClipEncoder(dw, dh, n, gop=GOP, qp=QP)
    e = P.Encoder(dw, dh, gop=GOP, qp=QP)
    ce.upload(clips.noise(dw, dh, n))
    ce.encode()                                                         # a picture for the way out to refuse
    e.encode(clips.noise(dw, dh, 1)[0])
    e.close()
    e = P.Encoder(dw, dh, gop=GOP, qp=QP)
    L, owned = ce.L, []
    for good, host, w, kw in ((good_small, host_small, dw, {}), (good_big, host_big, sw, dict(src_size=(sw, sh)))):
        ok = [(t.data_ptr(), t.stride(0) * 4) for t in good]
        cases = [([(host[c].ctypes.data, w * 4) for c in range(3)], "not memory of device|not inside one allocation")]
        for k in range(3):
            planes = list(ok)
            planes[k] = (host[k].ctypes.data, w * 4)                    # one host plane among device planes
            cases.append((planes, "not memory of device|not inside one allocation"))
            planes = list(ok)
            planes[k] = (ok[k][0], far)                                 # a plane that runs past its allocation
            cases.append((planes, "not memory of device|not inside one allocation"))
            planes = list(ok)
            planes[k] = (ok[k][0] + 2, ok[k][1])
            cases.append((planes, "plane %d .* is not a multiple of the 4 bytes of a f32 sample" % k))
            planes = list(ok)
            planes[k] = (ok[k][0], ok[k][1] + 2)
            cases.append((planes, "stride %d of plane %d is not a multiple of the 4 bytes" % (ok[k][1] + 2, k)))
            planes = list(ok)
            planes[k] = (ok[k][0], w * 4 - 4)
            cases.append((planes, "stride %d of plane %d is below" % (w * 4 - 4, k)))
        # the extent counts the sample's bytes: an allocation one sample short of the last row's end (the library's own allocator: torch
        # carves tensors out of larger blocks)
        rows = sh if kw else dh
        short = L.H264E_dev_malloc(0, rows * w * 4 - 4)
        assert short
        owned.append(short)
        cases.append(([ok[0], (short, w * 4), ok[2]], "plane 1 .*not inside one allocation"))
        for planes, msg in cases:
            with pytest.raises(P.H264EError, match=msg):
                ce.upload_device([planes], "rgbp_f32", **kw)
            with pytest.raises(P.H264EError, match=msg):
                e.encode_device(planes, "rgbp_f32", **kw)
            if not kw:
                with pytest.raises(P.H264EError, match=msg):
                    ce.read_recon_device(0, "rgbp_f32", out=planes)
    y = torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")
    pair = (y.data_ptr(), dw)
    for code, msg in ((P.DEV_FORMAT_I420 | P.DEV_SAMPLE_F16, "asks for f16 samples .* of I420"), (P.DEV_FORMAT_NV12 | P.DEV_SAMPLE_F32, "asks for f32 samples .* of NV12"),
                      (P.DEV_FORMAT_RGB | P.DEV_SAMPLE_BF16, "asks for bf16 samples .* of RGB"), (0x43, "unknown format 67")):
        d = P.DevFrame(format=code, pixel_bytes=3)
        for k in range(3):
            d.plane[k], d.stride[k] = pair
        assert ce.L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) != 0
        assert re.search(msg, ce.L.H264E_last_error().decode())
        assert ce.L.H264E_clip_read_recon_device(ce.c, 0, C.byref(d)) != 0
        assert re.search(msg, ce.L.H264E_last_error().decode())
    ce.upload_device([source(torch, f, kind, "chw") for f in small], "rgbpf")
    assert ce.encode()[0] == want_plain
    ce.upload_device([source(torch, f, kind, "chw_rows") for f in big], "rgbp_f32", src_size=(sw, sh))
    assert ce.encode()[0] == want_scaled
    assert b"".join(e.encode_device(source(torch, f, kind, "chw"), "rgbpf", src_size=(sw, sh)) for f in big) == want_scaled
    ce.close()
    e.close()
    for p in owned:
        L.H264E_dev_free(p)


# ---------------------------------------------------------------- ladder


@pytest.mark.parametrize("kind", ["bf16", "f32"])
def test_ladder_from_a_float_source(P, torch, kind):
    sw, sh, n = 128, 96, 2
    frames = [FM.ramp_picture(sw, sh, kind, t) for t in range(n)]
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26)), (64, 48, dict(qp=34))]
    got = P.encode_ladder([source(torch, f, kind, "chw_slice") for f in frames], "rgbpf", (sw, sh), rungs, gop=GOP)
    for (w, h, opts), (out, sizes, _) in zip(rungs, got):
        model = np.stack([M.scale_to_i420(FM.quantise(f, kind), w, h) for f in frames])
        assert (out, sizes) == oracle_lib.encode_clip(model, w, h, **dict(dict(gop=GOP), **opts))
