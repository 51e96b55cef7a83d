"""GPU: device input of another size on the MI355X (h264e_scale_kernel, H264E_clip_upload_device_scaled / H264E_encode_device_scaled) with
torch CUDA tensors as the source: the input slots against the numpy model (tests/scale_model.py), the streams against the oracle and
upload() of the model's frames, ordering against the producer's stream, the refusal of host pointers and of planes that reach past their
allocation BY THE SOURCE'S SIZE, and the ladder.  Everything that is refused here is refused by the host's checks, before any launch.

The issue's geometry "34x50 -> 2x2" is beyond the 16:1 cap the same issue sets (see tests/test_emu_scaled_input.py): the far 32 x 32
corner of a 34 x 50 source stands in for it."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import pkg
import scale_model as M

pytestmark = pytest.mark.gpu

GEOMETRIES = {
    "2to1": ((128, 96), (64, 48), None),
    "3to2": ((96, 72), (64, 48), None),
    "5to3": ((100, 60), (60, 36), None),
    "ragged": ((100, 52), (36, 20), None),
    "one_axis": ((128, 48), (64, 48), None),
    "crop_far_corner": ((100, 80), (64, 48), (36, 32, 64, 48)),
    "16to1": ((256, 64), (16, 4), None),
    "corner_of_34x50_to_2x2": ((34, 50), (2, 2), (2, 18, 32, 32)),
    "crop_and_scale": ((200, 120), (68, 36), (14, 6, 180, 108)),
    "two_tiles_wide": ((300, 160), (150, 80), None),
    "4k_to_1080p": ((3840, 2160), (1920, 1080), None),
    "1080p_to_360p": ((1920, 1080), (640, 360), None),
}
CASES = [("2to1", "packed"), ("2to1", "nv12_padded"), ("3to2", "padded"), ("3to2", "nv12"), ("5to3", "oddbase"), ("5to3", "separate"),
         ("ragged", "oddbase"), ("ragged", "nv12_padded"), ("ragged", "packed"), ("one_axis", "separate"), ("one_axis", "padded"),
         ("crop_far_corner", "packed"), ("crop_far_corner", "oddbase"), ("crop_far_corner", "nv12"), ("crop_far_corner", "separate"),
         ("16to1", "padded"), ("16to1", "nv12"), ("corner_of_34x50_to_2x2", "oddbase"), ("corner_of_34x50_to_2x2", "nv12_padded"),
         ("corner_of_34x50_to_2x2", "packed"), ("crop_and_scale", "oddbase"), ("crop_and_scale", "nv12_padded"),
         ("two_tiles_wide", "padded"), ("two_tiles_wide", "nv12"), ("4k_to_1080p", "packed"), ("1080p_to_360p", "nv12_padded")]


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


def dev(torch, arr, stride=None, offset=0):
    """the 2-D `arr` as a CUDA tensor; with `stride` / `offset`: a view into a 0xA5-filled buffer whose rows are `stride` bytes apart,
    which starts `offset` bytes into its tensor and ends with the last row's last byte"""
    arr = np.ascontiguousarray(arr, np.uint8)
    t = torch.from_numpy(arr).cuda()
    if stride is None and not offset:
        return t
    rows, rb = arr.shape
    stride = stride or rb
    buf = torch.full((offset + (rows - 1) * stride + rb,), 0xA5, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (rows, rb), (stride, 1), offset)
    view.copy_(t)
    return view


def source(torch, frame, w, h, layout):
    y, u, v = M.split(frame, w, h)
    if layout == "packed":
        return dev(torch, np.asarray(frame).reshape(h * 3 // 2, w)), "i420"
    if layout == "padded":
        return [dev(torch, y, w + 13), dev(torch, u, w // 2 + 7), dev(torch, v, w // 2 + 1)], "i420"
    if layout == "oddbase":
        return [dev(torch, y, w + 3, 1), dev(torch, u, w // 2 + 2, 3), dev(torch, v, w // 2 + 5, 1)], "i420"
    if layout == "separate":
        return [dev(torch, y), dev(torch, u), dev(torch, v)], "i420"
    yy, uv = M.nv12_planes(frame, w, h)
    if layout == "nv12":
        return (dev(torch, yy), dev(torch, uv)), "nv12"
    if layout == "nv12_padded":
        return (dev(torch, yy, w + 5, 3), dev(torch, uv, w + 9, 1)), "nv12"
    raise ValueError(layout)


def feed(torch, ce, frames, sw, sh, layout, crop, first=0):
    srcs = [source(torch, f, sw, sh, layout) for f in frames]
    ce.upload_device([s[0] for s in srcs], srcs[0][1], first=first, src_size=(sw, sh), crop=crop)


def model_frames(frames, sw, sh, dw, dh, crop):
    return np.stack([M.scale_frame(f, sw, sh, dw, dh, crop) for f in frames])


def clip_stream(P, w, h, n, put, **kw):
    ce = P.ClipEncoder(w, h, n, **kw)
    try:
        put(ce)
        out, sizes, _ = ce.encode()
        return out, sizes
    finally:
        ce.close()


# ---------------------------------------------------------------- slot bytes


@pytest.mark.parametrize("geom,layout", CASES)
def test_slot_holds_the_models_bytes(P, torch, geom, layout):
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    n = 2 if sw * sh <= 1 << 20 else 1
    frames = M.source_clip(sw, sh, n)
    want = model_frames(frames, sw, sh, dw, dh, crop)
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26)
    try:
        feed(torch, ce, frames, sw, sh, layout, crop)
        got = ce.download()
    finally:
        ce.close()
    assert np.array_equal(got, want), "slot contents differ from the model"


@pytest.mark.parametrize("kind", ["all255", "random"])
def test_4096_square_to_256_square_stays_inside_32_bits(P, torch, kind):
    s, d = 4096, 256
    rng = np.random.default_rng(5)
    y = np.full((s, s), 255, np.uint8) if kind == "all255" else rng.integers(0, 256, (s, s), dtype=np.uint8)
    if kind == "random":
        y[: s // 2] |= 0xF0
    u = np.full((s // 2, s // 2), 255, np.uint8) if kind == "all255" else rng.integers(0, 256, (s // 2, s // 2), dtype=np.uint8)
    v = u[::-1].copy()
    want = M.scale_i420(y, u, v, d, d)
    ce = P.ClipEncoder(d, d, 1, gop=30, qp=26)
    try:
        ce.upload_device([[dev(torch, y), dev(torch, u), dev(torch, v)]], "i420", src_size=(s, s))
        got = ce.download()[0]
    finally:
        ce.close()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------- streams


@pytest.mark.parametrize("geom,n,layout", [("2to1", 4, "padded"), ("5to3", 3, "nv12_padded"), ("crop_far_corner", 3, "oddbase")])
def test_streams_match_the_oracle_for_the_models_frames(P, torch, geom, n, layout):
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, crop)
    want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)
    got, sizes = clip_stream(P, dw, dh, n, lambda ce: feed(torch, ce, frames, sw, sh, layout, crop), gop=30, qp=26)
    up, up_sizes = clip_stream(P, dw, dh, n, lambda ce: ce.upload(model), gop=30, qp=26)
    e = P.Encoder(dw, dh, gop=30, qp=26)
    parts = []
    for f in frames:
        s, fmt = source(torch, f, sw, sh, layout)
        parts.append(e.encode_device(s, fmt, src_size=(sw, sh), crop=crop))
    e.close()
    assert got == up and sizes == up_sizes, "scaled device input and upload() of the model's frames give different streams"
    assert got == want and sizes == want_sizes, "scaled device input differs from the oracle"
    assert b"".join(parts) == want


# ---------------------------------------------------------------- ordering


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """torch writes the 1080p source on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer, and trashed as soon as the call returns: the slot must hold the model's 720p picture of the finished frame"""
    (sw, sh), (dw, dh) = (1920, 1080), (1280, 720)
    n = 2
    frames = M.source_clip(sw, sh, n)
    model = model_frames(frames, sw, sh, dw, dh, None)
    staged = torch.from_numpy(frames).cuda().view(n, sh * 3 // 2, sw)
    frame = torch.zeros((sh * 3 // 2, sw), dtype=torch.uint8, device="cuda")
    busy = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26)
    e = P.Encoder(dw, dh, gop=30, qp=26)
    parts = []
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        for i in range(n):
            for _ in range(20):
                busy = busy @ busy * 1e-4               # queued work in front of the write
            frame.copy_(staged[i])                      # the producer, on stream s
            ce.upload_device([frame], "i420", first=i, src_size=(sw, sh), stream=s.cuda_stream)
            frame.fill_(0x55)
            for _ in range(20):
                busy = busy @ busy * 1e-4
            frame.copy_(staged[i])
            parts.append(e.encode_device(frame, "i420", src_size=(sw, sh), stream=s.cuda_stream))
            frame.fill_(0xAA)
    slots = ce.download()
    out, _, _ = ce.encode()
    ce.close()
    e.close()
    torch.cuda.synchronize()
    assert np.array_equal(slots, model), "the scaler did not wait for the producer's stream, or read the frame after the call had returned"
    assert b"".join(parts) == out


# ---------------------------------------------------------------- refusals


def test_host_pointers_and_planes_beyond_their_allocation_are_refused(P, torch):
    """extents come from the SOURCE's size and window: a plane that holds the picture but not the source is refused, by both entry
    points, without a launch; so is host memory"""
    (sw, sh), (dw, dh) = (128, 96), (64, 48)
    frames = M.source_clip(sw, sh, 2)
    model = model_frames(frames, sw, sh, dw, dh, None)
    want = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)[0]
    good, _ = source(torch, frames[0], sw, sh, "separate")
    small = torch.zeros((dh, dw), dtype=torch.uint8, device="cuda")                # an allocation of its own that holds 64 x 48 samples only
    # (torch hands out parts of larger segments: only an extent beyond the SEGMENT is sure to be refused, so the rows are far apart)
    host = np.ascontiguousarray(frames[0])
    torch.cuda.synchronize()
    ok = [(t.data_ptr(), t.stride(0)) for t in good]
    far = 1 << 30
    ce = P.ClipEncoder(dw, dh, 2, gop=30, qp=26)
    e = P.Encoder(dw, dh, gop=30, qp=26)
    base = host.ctypes.data
    bad = [[(base, sw), (base + sw * sh, sw // 2), (base + sw * sh * 5 // 4, sw // 2)],       # host memory
           [ok[0], (base + sw * sh, sw // 2), ok[2]]]
    for k in range(3):                                                              # rows a gigabyte apart: 95 (47) of them leave any segment
        planes = list(ok)
        planes[k] = (ok[k][0], far)
        bad.append(planes)
    bad.append([(small.data_ptr(), far), ok[1], ok[2]])
    for planes in bad:
        with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
            ce.upload_device([planes], "i420", src_size=(sw, sh))
        with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
            e.encode_device(planes, "i420", src_size=(sw, sh))
    # the extent is the window's, by the source's stride: the last rows of a far window leave the allocation, the first rows do not
    with pytest.raises(P.H264EError, match="leave the source"):
        ce.upload_device([ok], "i420", src_size=(sw, sh), crop=(0, 50, 64, 48))
    pos, up = C.c_int(), C.c_int()
    ce.L.H264E_clip_position(ce.c, C.byref(pos), C.byref(up))
    assert (pos.value, up.value) == (0, 0)
    feed(torch, ce, frames, sw, sh, "separate", None)
    assert ce.encode()[0] == want
    assert b"".join(e.encode_device(source(torch, f, sw, sh, "packed")[0], "i420", src_size=(sw, sh)) for f in frames) == want
    ce.close()
    e.close()


# ---------------------------------------------------------------- ladder


def test_ladder_gives_each_rung_the_stream_of_a_standalone_encoder(P, torch):
    sw, sh, n = 128, 96, 4
    frames = M.source_clip(sw, sh, n)
    rungs = [(64, 48, dict(qp=26)), (64, 48, dict(qp=34)), (32, 24, dict(qp=28, gop=2))]
    srcs = [source(torch, f, sw, sh, "padded")[0] for f in frames]
    got = P.encode_ladder(srcs, "i420", (sw, sh), rungs, gop=30)
    assert len(got) == len(rungs)
    for (w, h, opts), (out, sizes, _) in zip(rungs, got):
        model = model_frames(frames, sw, sh, w, h, None)
        want, want_sizes = oracle_lib.encode_clip(model, w, h, **dict(dict(gop=30), **opts))
        assert (out, sizes) == (want, want_sizes)
