"""GPU: device-resident output on the MI355X (H264E_clip_read_recon_device / H264E_read_recon_device: h264e_egress_kernel) with torch CUDA
tensors as the destination: the bytes against the numpy model (tests/egress_model.py) applied to read_recon(frame) -- I420, NV12, RGB of
3 and 4 bytes, planar RGB, every colour setting, plain, cropped and tiny pictures and a P-frame clip; destinations that are views (a CHW
slice, every other row of a larger tensor, odd addresses and strides) inside sentinel-filled buffers whose other bytes must stay;
ordering against a stream that still writes the destination; the tensors out=None returns; and the refusal of host pointers, of planes
that reach past their allocation and of another device's memory, before any launch.  Everything is integer arithmetic: every comparison
is byte equality."""
import numpy as np
import pytest

import clips
import egress_model as EM
import pkg

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 16
COLORS = [None, "bt709", "bt601-full", "bt709-full"]
KINDS = [("i420", 0), ("nv12", 0), ("rgb", 3), ("rgb", 4), ("rgbp", 0)]
RGB_KINDS = [k for k in KINDS if k[0] in ("rgb", "rgbp")]
LAYOUTS = {"i420": ["one", "separate", "odd"], "nv12": ["separate", "odd"], "rgb": ["one", "odd"], "rgbp": ["one", "slice", "rows", "separate", "odd"]}
# width, height, frames: the first has coded size = picture size, the next four are cropped (202 x 2: 101-byte chroma rows), the last has P frames of some size
PICTURES = [(64, 48, 3), (18, 18, 2), (2, 160, 2), (202, 2, 2), (2, 2, 2), (144, 96, 4)]
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


def coded(v):
    return (v + 15) // 16 * 16


def clip_frames(w, h, n):
    return clips.ramp(w, h, n) if w * h < 64 * 48 or (w, h) == (202, 2) else clips.make("scene", w, h, n)


_recons = {}


def recons(P, w, h, n, color=None):
    """(frames, [read_recon(f)]) of the clip of that size, encoded once per colour (the colour changes the SPS, not the pictures)"""
    key = (w, h, n, color)
    if key not in _recons:
        frames = clip_frames(w, h, n)
        ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, color=color)
        try:
            ce.upload(frames)
            ce.encode()
            _recons[key] = (frames, [ce.read_recon(f) for f in range(n)])
        finally:
            ce.close()
    return _recons[key]


class Dest:
    """a destination made of views into sentinel-filled CUDA buffers: `out` is what read_recon_device takes; result() reads the buffers
    back, returns the views' bytes in the model's shape and asserts that every other byte still holds the sentinel"""

    def __init__(self, torch, fmt, pb, w, h, layout):
        self.torch, self.fmt = torch, fmt
        sizes = {"i420": [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "nv12": [(h, w), (h // 2, w)], "rgb": [(h, w * pb)], "rgbp": [(h, w)] * 3}[fmt]
        self.items = []                             # (buffer, offset, shape, strides) of every view
        if fmt == "rgb":
            stride = w * pb if layout == "one" else (w * pb + 12) | 1
            self._view(GUARD + (0 if layout == "one" else 3), (h, w, pb), (stride, pb, 1))
        elif fmt == "rgbp" and layout == "one":
            self._view(GUARD, (3, h, w), (h * w, w, 1))
        elif fmt == "rgbp" and layout == "slice":   # channels 1..3 of a (4, h, w) tensor
            self._view(GUARD + h * w, (3, h, w), (h * w, w, 1))
        elif fmt == "rgbp" and layout == "rows":    # every other row and a column window of a (3, 2h, w + 6) tensor
            self._view(GUARD + (w + 6) + 3, (3, h, w), (2 * h * (w + 6), 2 * (w + 6), 1))
        elif fmt == "i420" and layout == "one":     # one packed (h*3/2, w) tensor
            self._view(GUARD, (h * 3 // 2, w), (w, 1))
        else:
            for k, (rows, rb) in enumerate(sizes):
                offset, stride = (GUARD + (1, 3, 2)[k], (rb + 12) | 1) if layout == "odd" else (GUARD, rb)
                self._view(offset, (rows, rb), (stride, 1))
        views = [torch.as_strided(b, s, st, o) for b, o, s, st in self.items]
        self.out = views[0] if len(views) == 1 else views

    def _view(self, offset, shape, strides):
        n = offset + sum((d - 1) * s for d, s in zip(shape, strides)) + 1 + GUARD
        self.items.append((self.torch.full((n,), SENTINEL, dtype=self.torch.uint8, device="cuda"), offset, shape, strides))

    def result(self):
        got = []
        for buf, offset, shape, strides in self.items:
            host = buf.cpu().numpy().copy()
            view = np.lib.stride_tricks.as_strided(host[offset:], shape, strides)
            got.append(view.copy())
            view[...] = SENTINEL
            bad = np.flatnonzero(host != SENTINEL)
            assert bad.size == 0, "%s: %d bytes outside the rows were written, the first at offset %d" % (self.fmt, bad.size, bad[0])
        if self.fmt == "i420":
            return np.concatenate([g.reshape(-1) for g in got])
        if self.fmt == "nv12":
            return tuple(got)
        return got[0] if len(got) == 1 else np.stack(got)

    def untouched(self):
        return all(bool((buf == SENTINEL).all()) for buf, _, _, _ in self.items)


def same(got, want):
    if isinstance(want, tuple):
        return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    return np.array_equal(got, want)


def check_all(torch, read, packed, w, h, color, kinds=KINDS, what=""):
    for fmt, pb in kinds:
        want = EM.recon_to(fmt, packed, coded(w), coded(h), w, h, color, pb or 3)
        for layout in LAYOUTS[fmt]:
            d = Dest(torch, fmt, pb, w, h, layout)
            read(fmt, d.out)
            assert same(d.result(), want), "%s %dx%d %s/%d %s colour %s: the destination differs from the model" % (what, w, h, fmt, pb, layout, color)


# ---------------------------------------------------------------- bytes


@pytest.mark.parametrize("color", COLORS, ids=lambda c: c or "default")
@pytest.mark.parametrize("w,h,n", PICTURES)
def test_clip_destination_holds_the_models_bytes(P, torch, w, h, n, color):
    frames = clip_frames(w, h, n)
    kinds = KINDS if color is None else RGB_KINDS           # colour only matters for the RGB formats
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP, color=color)
    try:
        ce.upload(frames)
        ce.encode()
        packed = [ce.read_recon(f) for f in range(n)]
        if n > 3:
            assert all(not np.array_equal(packed[f], packed[f + 1]) for f in range(n - 1))      # P frames, each its own picture
        for f in range(n):
            check_all(torch, lambda fmt, out: ce.read_recon_device(f, fmt, out=out), packed[f], w, h, color, kinds, "frame %d" % f)
    finally:
        ce.close()


@pytest.mark.parametrize("w,h,n,color", [(64, 48, 3, None), (18, 18, 2, "bt709-full"), (202, 2, 2, "bt709"), (144, 96, 4, "bt601-full")])
def test_per_frame_encoder_after_encode_and_after_encode_device(P, torch, w, h, n, color):
    frames, packed = recons(P, w, h, n)
    a = P.Encoder(w, h, gop=GOP, qp=QP, color=color)
    b = P.Encoder(w, h, gop=GOP, qp=QP, color=color)
    try:
        for f in range(n):
            a.encode(frames[f])
            check_all(torch, lambda fmt, out: a.read_recon_device(fmt, out=out), packed[f], w, h, color, what="encode, frame %d" % f)
            b.encode_device(torch.from_numpy(frames[f].reshape(h * 3 // 2, w)).cuda(), "i420")
            check_all(torch, lambda fmt, out: b.read_recon_device(fmt, out=out), packed[f], w, h, color, RGB_KINDS, "encode_device, frame %d" % f)
    finally:
        a.close()
        b.close()


def test_per_frame_i420_equals_what_const_input_0_writes_back(P, torch):
    w, h, n = 64, 48, 3
    frames = clip_frames(w, h, n)
    e = P.Encoder(w, h, gop=GOP, qp=QP, const_input=0)
    try:
        for f in range(n):
            y, u, v = (p.copy() for p in EM.planes(frames[f], w, h, w, h))
            e.encode_planes(y, u, v)
            back = np.concatenate([y.reshape(-1), u.reshape(-1), v.reshape(-1)])
            assert not np.array_equal(back, frames[f])
            d = Dest(torch, "i420", 0, w, h, "odd")
            e.read_recon_device("i420", out=d.out)
            assert np.array_equal(d.result(), back), "frame %d" % f
    finally:
        e.close()


# ---------------------------------------------------------------- ordering


def test_destination_still_being_filled_on_another_stream_is_waited_for(P, torch):
    """a fill of the destination is queued on a side stream behind other work, and the destination is handed over at once with that
    stream as the producer: the result must be the reconstruction, not the fill (the launch waited), on both entry points"""
    w, h, n = 640, 360, 2
    frames, packed = recons(P, w, h, n)
    want = EM.recon_to("rgbp", packed[1], coded(w), coded(h), w, h)
    busy = torch.ones((2048, 2048), device="cuda")
    out = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP)
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    try:
        ce.upload(frames)
        ce.encode()
        for f in frames:
            e.encode(f)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        for read in (lambda: ce.read_recon_device(1, "rgbp", out=out, stream=s.cuda_stream), lambda: e.read_recon_device("rgbp", out=out, stream=s.cuda_stream)):
            with torch.cuda.stream(s):
                assert torch.cuda.current_stream().cuda_stream != 0
                for _ in range(20):
                    busy = busy @ busy * 1e-4           # queued work in front of the fill
                out.fill_(0x55)
                read()
            s.synchronize()
            assert np.array_equal(out.cpu().numpy(), want), "the egress did not wait for the stream that was still filling the destination"
    finally:
        ce.close()
        e.close()


# ---------------------------------------------------------------- out=None


def test_out_none_returns_tensors_of_the_documented_shapes(P, torch):
    w, h, n = 18, 18, 2
    frames, packed = recons(P, w, h, n)
    shapes = {"i420": (h * 3 // 2, w), "nv12": ((h, w), (h // 2, w)), "rgb": (h, w, 3), "rgbp": (3, h, w)}
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP)
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    try:
        ce.upload(frames)
        ce.encode()
        for f in frames:
            e.encode(f)
        assert tuple(ce.read_recon_device(1).shape) == (3, h, w)            # the default format is planar RGB
        for fmt, shape in shapes.items():
            want = EM.recon_to(fmt, packed[1], coded(w), coded(h), w, h)
            for got in (ce.read_recon_device(1, fmt), e.read_recon_device(fmt)):
                parts = got if isinstance(got, tuple) else (got,)
                assert all(t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() for t in parts)
                if fmt == "nv12":
                    assert tuple(tuple(t.shape) for t in got) == shape
                    assert same(tuple(t.cpu().numpy() for t in got), want)
                else:
                    assert tuple(got.shape) == shape
                    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want)
    finally:
        ce.close()
        e.close()


# ---------------------------------------------------------------- refusals of the memory check


def test_host_pointers_and_short_allocations_are_refused_without_a_launch(P, torch):
    """the product's memory check answers with an error; the destination keeps its bytes and a valid call afterwards gives the right ones"""
    w, h, n = 64, 48, 2
    frames, packed = recons(P, w, h, n)
    L = P.load()
    ce = P.ClipEncoder(w, h, n, gop=GOP, qp=QP)
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    blocks = []
    try:
        ce.upload(frames)
        ce.encode()
        for f in frames:
            e.encode(f)
        good = Dest(torch, "rgbp", 0, w, h, "separate")
        ok = [(t.data_ptr(), t.stride(0)) for t in good.out]
        host = np.full((3, h, w), SENTINEL, np.uint8)
        # one row too short: a block of h - 1 rows 4096 bytes apart described as h rows (the allocation may be rounded up to whole pages: the
        # last row still begins behind it); and one row of a tensor described as the first of two, a gigabyte apart (torch's allocator
        # hands out pieces of larger segments: only such a distance is sure to leave the segment)
        pitch = 4096
        short = L.H264E_dev_malloc(0, (h - 2) * pitch + w)
        assert short
        blocks.append(short)
        fits = L.H264E_dev_malloc(0, (h - 1) * pitch + w)
        assert fits
        blocks.append(fits)
        one_row = torch.full((1, w), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        bad = [[(host[c].ctypes.data, w) for c in range(3)]]
        for k in range(3):
            for plane in ((host[k].ctypes.data, w), (short, pitch)):
                planes = list(ok)
                planes[k] = plane
                bad.append(planes)
        for planes in bad:
            with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
                ce.read_recon_device(1, "rgbp", out=planes)
            with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
                e.read_recon_device("rgbp", out=planes)
        e2 = P.Encoder(w, 2, gop=GOP, qp=QP)                               # a picture of two rows
        try:
            e2.encode(clip_frames(w, 2, 1)[0])
            with pytest.raises(P.H264EError, match="not inside one allocation"):
                e2.read_recon_device("nv12", out=[(one_row.data_ptr(), 1 << 30), (one_row.data_ptr(), w)])
        finally:
            e2.close()
        assert good.untouched() and (host == SENTINEL).all() and bool((one_row == SENTINEL).all())
        # the block that does hold h rows is accepted, and the tensors too
        want = EM.recon_to("rgbp", packed[1], coded(w), coded(h), w, h)
        ce.read_recon_device(1, "rgbp", out=[ok[0], ok[1], (fits, pitch)])
        back = np.empty((h - 1) * pitch + w, np.uint8)
        assert L.H264E_dev_memcpy(back.ctypes.data, fits, back.size, 0) == 0
        assert np.array_equal(np.stack([back[y * pitch: y * pitch + w] for y in range(h)]), want[2])
        check_all(torch, lambda fmt, out: ce.read_recon_device(1, fmt, out=out), packed[1], w, h, None, [("rgbp", 0)])
        check_all(torch, lambda fmt, out: e.read_recon_device(fmt, out=out), packed[1], w, h, None, [("rgb", 4)])
    finally:
        ce.close()
        e.close()
        for b in blocks:
            L.H264E_dev_free(b)


def test_wrong_device_is_refused(P, torch):
    """a tensor of another GPU than the encoder's (needs two visible devices)"""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    w, h, n = 64, 48, 2
    frames, packed = recons(P, w, h, n)
    e = P.Encoder(w, h, gop=GOP, qp=QP)
    try:
        e.encode(frames[0])
        other = torch.full((3, h, w), SENTINEL, dtype=torch.uint8, device="cuda:1")
        torch.cuda.synchronize(1)
        with pytest.raises(P.H264EError, match="not memory of device 0"):
            e.read_recon_device("rgbp", out=other, stream=0)
        assert bool((other == SENTINEL).all())
        check_all(torch, lambda fmt, out: e.read_recon_device(fmt, out=out), packed[0], w, h, None, [("rgbp", 0)])
    finally:
        e.close()
