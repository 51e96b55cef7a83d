"""GPU: planar RGB device input on the MI355X (H264E_DEV_FORMAT_RGBP: h264e_ingest_kernel at the picture's size, h264e_scale_rgb_kernel
with a window) with torch CUDA tensors as the source: the input slots against the numpy model (tests/rgbp_model.py), CHW tensors that are
non-contiguous views, the streams against the oracle, ordering against the producer's stream, and the refusal of host pointers and of
planes that reach past their allocation, before any launch.  Everything is integer arithmetic: every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import ingest_model
import oracle_lib
import pkg
import rgbp_model as M

pytestmark = pytest.mark.gpu


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


def source(torch, chw, layout):
    """what upload_device(..., "rgbp") takes for one (3, h, w) frame"""
    _, h, w = chw.shape
    if layout == "separate":                # three tensors
        return [dev(torch, chw[c]) for c in range(3)]
    if layout == "padded":                  # odd strides and odd start addresses per plane
        return [dev(torch, chw[0], w + 13, 1), dev(torch, chw[1], w + 7, 3), dev(torch, chw[2], w + 1, 2)]
    if layout == "chw":                     # one contiguous CHW tensor
        return torch.from_numpy(np.ascontiguousarray(chw)).cuda()
    if layout == "chw_slice":               # channels 1..3 of a [4, h, w] tensor: a view that starts h*w bytes into its storage
        t = torch.full((4, h, w), 0xA5, dtype=torch.uint8, device="cuda")
        t[1:].copy_(torch.from_numpy(np.ascontiguousarray(chw)))
        return t[1:]
    if layout == "chw_rows":                # every other row and a column window of a [3, 2h, w + 6] tensor: row and channel strides of a view
        t = torch.full((3, 2 * h, w + 6), 0xA5, dtype=torch.uint8, device="cuda")
        v = t[:, 1::2, 3:3 + w]
        v.copy_(torch.from_numpy(np.ascontiguousarray(chw)))
        assert not v.is_contiguous() and v.stride() == (2 * h * (w + 6), 2 * (w + 6), 1)
        return v
    raise ValueError(layout)


def feed(torch, ce, frames, layout, src_size=None, crop=None, first=0):
    ce.upload_device([source(torch, f, layout) for f in frames], "rgbp", first=first, src_size=src_size, crop=crop)


def slots(P, torch, frames, layout, dw, dh, src_size=None, crop=None):
    ce = P.ClipEncoder(dw, dh, len(frames), gop=30, qp=26)
    try:
        feed(torch, ce, frames, layout, src_size, crop)
        return ce.download()
    finally:
        ce.close()


# ---------------------------------------------------------------- slot bytes, at the picture's size


@pytest.mark.parametrize("w,h,layout", [(2, 2, "separate"), (2, 2, "chw_rows"), (202, 122, "separate"), (202, 122, "padded"), (64, 48, "padded"),
                                        (64, 48, "chw"), (64, 48, "chw_slice"), (64, 48, "chw_rows"), (1920, 1080, "chw"), (1282, 722, "chw_slice")])
def test_plain_slot_holds_the_models_bytes(P, torch, w, h, layout):
    n = 3 if w * h <= 1 << 16 else 1
    frames = M.clip(w, h, n)
    want = np.stack([M.to_i420(f) for f in frames])
    assert np.array_equal(slots(P, torch, frames, layout, w, h), want), "slot contents differ from the model"


def test_planar_equals_packed_rgb_of_the_same_image(P, torch):
    w, h, n = 202, 122, 2
    hwc = ingest_model.rgb_clip(w, h, n, 3)
    a = slots(P, torch, M.clip(w, h, n), "chw", w, h)
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26)
    ce.upload_device([torch.from_numpy(f).cuda() for f in hwc], "rgb")
    b = ce.download()
    ce.close()
    assert np.array_equal(a, b)


# ---------------------------------------------------------------- slot bytes, through a window

GEOMETRIES = {
    "2to1": ((128, 96), (64, 48), None),
    "5to3": ((160, 80), (96, 48), None),
    "crop_far_corner": ((128, 96), (64, 48), (64, 48, 64, 48)),
    "16to1": ((32, 32), (2, 2), None),
    "partial_tiles": ((200, 102), (80, 34), None),
    "crop_and_scale": ((200, 120), (68, 36), (14, 6, 180, 108)),
    "4k_to_1080p": ((3840, 2160), (1920, 1080), None),
}
SCALED = [("2to1", "separate"), ("2to1", "chw"), ("5to3", "padded"), ("5to3", "chw_rows"), ("crop_far_corner", "separate"), ("crop_far_corner", "chw_slice"),
          ("16to1", "padded"), ("16to1", "separate"), ("partial_tiles", "separate"), ("partial_tiles", "padded"), ("crop_and_scale", "padded"),
          ("crop_and_scale", "chw_rows"), ("4k_to_1080p", "chw")]


@pytest.mark.parametrize("geom,layout", SCALED)
def test_scaled_slot_holds_the_models_bytes(P, torch, geom, layout):
    (sw, sh), (dw, dh), crop = GEOMETRIES[geom]
    frames = M.noisy_clip(sw, sh, 2 if sw * sh <= 1 << 20 else 1)
    want = np.stack([M.scale_to_i420(f, dw, dh, crop) for f in frames])
    assert np.array_equal(slots(P, torch, frames, layout, dw, dh, (sw, sh), crop), want), "slot contents differ from the model"


@pytest.mark.parametrize("kind", ["all255", "random"])
def test_4096_square_to_256_square_stays_inside_32_bits(P, torch, kind):
    """16:1 from the largest window: 255 * 2^24 + 2^23 is the largest numerator, in every channel"""
    s, d = 4096, 256
    if kind == "all255":
        chw = np.full((3, s, s), 255, np.uint8)
    else:
        chw = np.random.default_rng(5).integers(0, 256, (3, s, s), dtype=np.uint8)
        chw[:, : s // 2] |= 0xF0            # bright half: sums close to the bound next to sums that are not
    want = M.scale_to_i420(chw, d, d)
    if kind == "all255":
        assert (want[: d * d] == 235).all() and (want[d * d:] == 128).all()
    assert np.array_equal(slots(P, torch, [chw], "chw", d, d, (s, s))[0], want)


# ---------------------------------------------------------------- streams


@pytest.mark.parametrize("name", ["plain", "scaled"])
def test_streams_match_the_oracle_for_the_models_frames(P, torch, name):
    (sw, sh), (dw, dh), n = ((64, 48) if name == "plain" else (128, 96)), (64, 48), 4
    src_size = None if name == "plain" else (sw, sh)
    frames = M.noisy_clip(sw, sh, n)
    model = np.stack([M.to_i420(f) if name == "plain" else M.scale_to_i420(f, dw, dh) for f in frames])
    want, want_sizes = oracle_lib.encode_clip(model, dw, dh, gop=30, qp=26)
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26)
    feed(torch, ce, frames, "chw_slice", src_size)
    got, sizes, _ = ce.encode()
    ce.close()
    e = P.Encoder(dw, dh, gop=30, qp=26)
    parts = [e.encode_device(source(torch, f, "padded"), "rgbp", src_size=src_size) for f in frames]
    e.close()
    assert got == want and sizes == want_sizes, "planar RGB device input differs from the oracle"
    assert b"".join(parts) == want


def test_ladder_from_chw_tensors(P, torch):
    sw, sh, n = 128, 96, 3
    frames = M.noisy_clip(sw, sh, n)
    rungs = [(128, 96, dict(qp=30)), (64, 48, dict(qp=26)), (64, 48, dict(qp=34))]
    got = P.encode_ladder([source(torch, f, "chw") for f in frames], "rgbp", (sw, sh), rungs, gop=30)
    for (w, h, opts), (out, sizes, _) in zip(rungs, got):
        model = np.stack([M.scale_to_i420(f, w, h) for f in frames])
        assert (out, sizes) == oracle_lib.encode_clip(model, w, h, **dict(dict(gop=30), **opts))


# ---------------------------------------------------------------- ordering


def test_source_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """torch writes the 1080p CHW source on a side stream behind a queue of other work; it is handed over at once with that stream as the
    producer, and trashed as soon as the call returns: the slots must hold the model's pictures of the finished frames, at the picture's
    size and at 720p"""
    (sw, sh), (dw, dh), n = (1920, 1080), (1280, 720), 2
    frames = M.noisy_clip(sw, sh, n)
    plain = np.stack([M.to_i420(f) for f in frames])
    scaled = np.stack([M.scale_to_i420(f, dw, dh) for f in frames])
    staged = torch.from_numpy(frames).cuda()
    frame = torch.zeros((3, sh, sw), dtype=torch.uint8, device="cuda")
    busy = torch.ones((2048, 2048), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    a = P.ClipEncoder(sw, sh, n, gop=30, qp=26)
    b = P.ClipEncoder(dw, dh, n, gop=30, qp=26)
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        for i in range(n):
            for ce, kw in ((a, {}), (b, dict(src_size=(sw, sh)))):
                for _ in range(20):
                    busy = busy @ busy * 1e-4           # queued work in front of the write
                frame.copy_(staged[i])                  # the producer, on stream s
                ce.upload_device([frame], "rgbp", first=i, stream=s.cuda_stream, **kw)
                frame.fill_(0x55)
    got_plain, got_scaled = a.download(), b.download()
    a.close()
    b.close()
    torch.cuda.synchronize()
    assert np.array_equal(got_plain, plain), "the ingest did not wait for the producer's stream, or read the frame after the call had returned"
    assert np.array_equal(got_scaled, scaled), "the scaler did not wait for the producer's stream, or read the frame after the call had returned"


# ---------------------------------------------------------------- refusals


def test_host_pointers_planes_beyond_their_allocation_and_other_types_are_refused(P, torch):
    """refused by both entry points, at the picture's size and through a window, without a launch; then the encoders go on working"""
    (sw, sh), (dw, dh), n = (128, 96), (64, 48), 2
    big, small = M.noisy_clip(sw, sh, n), M.noisy_clip(dw, dh, n)
    want_scaled = oracle_lib.encode_clip(np.stack([M.scale_to_i420(f, dw, dh) for f in big]), dw, dh, gop=30, qp=26)[0]
    want_plain = oracle_lib.encode_clip(np.stack([M.to_i420(f) for f in small]), dw, dh, gop=30, qp=26)[0]
    good_big, good_small = source(torch, big[0], "separate"), source(torch, small[0], "separate")
    host_big, host_small = np.ascontiguousarray(big[0]), np.ascontiguousarray(small[0])
    torch.cuda.synchronize()
    far = 1 << 30                                                       # rows a gigabyte apart leave any segment of torch's allocator
    ce = P.ClipEncoder(dw, dh, n, gop=30, qp=26)
    e = P.Encoder(dw, dh, gop=30, qp=26)
    for good, host, w, kw in ((good_small, host_small, dw, {}), (good_big, host_big, sw, dict(src_size=(sw, sh)))):
        ok = [(t.data_ptr(), t.stride(0)) for t in good]
        bad = [[(host[c].ctypes.data, w) for c in range(3)]]           # host memory
        for k in range(3):
            planes = list(ok)
            planes[k] = (host[k].ctypes.data, w)                        # one host plane among device planes
            bad.append(planes)
            planes = list(ok)
            planes[k] = (ok[k][0], far)                                 # a plane that runs past its allocation
            bad.append(planes)
        for planes in bad:
            with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
                ce.upload_device([planes], "rgbp", **kw)
            with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
                e.encode_device(planes, "rgbp", **kw)
    for t in (torch.zeros((3, dh, dw), dtype=torch.float32, device="cuda"), torch.zeros((3, dh, dw), dtype=torch.int8, device="cuda"),
              torch.zeros((3, dh, dw), dtype=torch.float16, device="cuda")):
        with pytest.raises(P.H264EError, match="uint8 samples, not torch"):
            ce.upload_device([t], "rgbp")
        with pytest.raises(P.H264EError, match="uint8 samples, not torch"):
            e.encode_device(t, "rgbp")
    pos, up = C.c_int(), C.c_int()
    ce.L.H264E_clip_position(ce.c, C.byref(pos), C.byref(up))
    assert (pos.value, up.value) == (0, 0)
    feed(torch, ce, small, "chw")
    assert ce.encode()[0] == want_plain
    feed(torch, ce, big, "chw_rows", (sw, sh))
    assert ce.encode()[0] == want_scaled
    assert b"".join(e.encode_device(source(torch, f, "chw"), "rgbp", src_size=(sw, sh)) for f in big) == want_scaled
    ce.close()
    e.close()
