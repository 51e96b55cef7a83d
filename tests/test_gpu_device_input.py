"""GPU: device-resident input on the MI355X (h264e_ingest_kernel, H264E_clip_upload_device / H264E_encode_device) with torch CUDA tensors
as the source: I420 against the oracle, the recorded reference streams and upload(); NV12 and RGB against the numpy model
(tests/ingest_model.py); ordering against the producer's stream; the refusal of host pointers; and both import orders of torch and
the library (each ships / links a HIP runtime of the same soname), each in a child process of its own."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import clips
import ingest_model as M
import oracle_lib
import pkg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "golden.json")))
GOLDEN_BIG = json.load(open(os.path.join(HERE, "golden", "golden_big.json")))
GEOMETRY = {g["name"]: g for g in json.load(open(os.path.join(HERE, "golden", "geometry.json")))}
TINY = ["ramp_2x2_qp26", "ramp_4x4_gop1", "ramp_2x2_kbps50", "ramp_6x6_kbps50", "noise_14x10_qp26", "ramp_18x18_qp10", "noise_34x50_qp51", "ramp_34x50_thr2_kbps200"]


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


def flags(s):
    t = s.split()
    d = dict(zip(t[0::2], t[1::2]))
    return dict(gop=int(d.get("--gop", 20)), qp=int(d.get("--qp", 33)), speed=int(d.get("--speed", 0)), kbps=int(d.get("--kbps", 0)),
                slices=int(d.get("--threads", 0)))


def dev(torch, arr, stride=None, offset=0):
    """`arr` (2-D, or (h, w, c) pixels) as a CUDA tensor; with `stride` / `offset`: a view into a larger 0xA5-filled buffer whose rows
    are `stride` bytes apart and which starts `offset` bytes into its allocation"""
    arr = np.ascontiguousarray(arr, np.uint8)
    t = torch.from_numpy(arr).cuda()
    if stride is None and not offset:
        return t
    rows, rb = arr.shape[0], arr[0].size
    stride = stride or rb
    buf = torch.full((offset + rows * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[offset: offset + rows * stride].view(rows, stride)[:, :rb]
    view.copy_(t.reshape(rows, rb))
    return view.unflatten(1, arr.shape[1:]) if arr.ndim == 3 else view


def i420_source(torch, frame, w, h, layout):
    y, u, v = M.split(frame, w, h)
    if layout == "packed":
        return dev(torch, np.asarray(frame).reshape(h * 3 // 2, w))
    if layout == "padded":
        return [dev(torch, y, w + 13, 1), dev(torch, u, w // 2 + 7, 3), dev(torch, v, w // 2 + 1, 2)]
    if layout == "separate":
        return [dev(torch, y), dev(torch, u), dev(torch, v)]
    if layout == "pairs":                   # explicit (pointer, stride) pairs; the tensors ride along to stay alive
        ts = [dev(torch, y, w + 3, 1), dev(torch, u), dev(torch, v, w // 2 + 5, 0)]
        torch.cuda.synchronize()            # a bare pointer carries no stream: the caller has synchronised
        return Pairs([(t.data_ptr(), t.stride(0)) for t in ts], ts)
    raise ValueError(layout)


class Pairs(list):
    def __init__(self, pairs, keep):
        super().__init__(pairs)
        self.keep = keep


def clip_stream(P, w, h, frames, feed, **kw):
    ce = P.ClipEncoder(w, h, len(frames), **kw)
    try:
        feed(ce)
        out, sizes, st = ce.encode()
        return out, sizes, ce.download(), st
    finally:
        ce.close()


# ---------------------------------------------------------------- I420


@pytest.mark.parametrize("w,h,n,layout", [
    (64, 48, 4, "packed"), (64, 48, 4, "padded"), (64, 48, 3, "separate"), (64, 48, 3, "pairs"),
    (176, 144, 3, "padded"), (176, 144, 3, "separate"), (200, 120, 3, "padded"), (200, 120, 3, "packed"),
    (202, 122, 3, "packed"), (202, 122, 3, "padded"), (202, 122, 3, "separate"), (202, 122, 3, "pairs"),
])
def test_i420_clip_encoder_matches_oracle_and_upload(P, torch, w, h, n, layout):
    c = clips.make("scene", w, h, n)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)
    got, sizes, slots, _ = clip_stream(P, w, h, c, lambda ce: ce.upload_device([i420_source(torch, f, w, h, layout) for f in c], "i420"), gop=30, qp=26)
    up, _, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload(c), gop=30, qp=26)
    assert np.array_equal(slots, c), "the input slots do not hold the source frames"
    assert got == up, "device input and upload() give different streams"
    assert got == want and sizes == want_sizes, "device input differs from the oracle"


@pytest.mark.parametrize("w,h,n,layout", [(64, 48, 4, "padded"), (176, 144, 3, "packed"), (200, 120, 3, "separate"), (202, 122, 3, "padded")])
def test_i420_per_frame_encoder_matches_oracle_and_encode(P, torch, w, h, n, layout):
    c = clips.make("scene", w, h, n)
    want, want_sizes = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)
    a = P.Encoder(w, h, gop=30, qp=26)
    parts = [a.encode_device(i420_source(torch, f, w, h, layout), "i420") for f in c]
    a.close()
    b = P.Encoder(w, h, gop=30, qp=26)
    host = [b.encode(f) for f in c]
    b.close()
    assert parts == host
    assert b"".join(parts) == want and [len(p) for p in parts] == want_sizes


@pytest.mark.parametrize("name", TINY)
def test_i420_tiny_pictures_match_reference_streams(P, torch, name):
    g = GEOMETRY[name]
    w, h, n = g["w"], g["h"], g["frames"]
    c = clips.make(g["clip"], w, h, n)
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    kw = flags(g["flags"])
    for layout in ("padded", "packed"):
        out, sizes, slots, _ = clip_stream(P, w, h, c, lambda ce: ce.upload_device([i420_source(torch, f, w, h, layout) for f in c], "i420"), **kw)
        e = P.Encoder(w, h, **kw)
        parts = [e.encode_device(i420_source(torch, f, w, h, layout), "i420") for f in c]
        e.close()
        assert np.array_equal(slots, c)
        assert sizes == g["frame_bytes"] and hashlib.md5(out).hexdigest() == g["md5"]
        assert [len(p) for p in parts] == g["frame_bytes"] and hashlib.md5(b"".join(parts)).hexdigest() == g["md5"]


@pytest.mark.parametrize("g", [g for g in GOLDEN if g["w"] * g["h"] <= 640 * 368], ids=lambda g: "%s_%dx%d_%s" % (g["clip"], g["w"], g["h"], g["flags"].replace(" ", "").replace("--", "_")))
def test_small_goldens_fed_as_device_i420(P, torch, g):
    """the reference's recorded streams (tests/golden/golden.json), the frames handed over as padded device planes"""
    w, h, n = g["w"], g["h"], g["frames"]
    c = clips.make(g["clip"], w, h, n)
    assert hashlib.md5(c.tobytes()).hexdigest() == g["input_md5"]
    out, sizes, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload_device([i420_source(torch, f, w, h, "padded") for f in c], "i420"), **flags(g["flags"]))
    assert sizes == g["frame_bytes"]
    assert len(out) == g["bytes"] and hashlib.md5(out).hexdigest() == g["md5"]


def test_1080p_synth_through_a_torch_tensor(P, torch):
    """synth_v1 at 1080p: generated on the device, brought to the host, moved into ONE torch tensor and fed back as device I420 --
    the reference's recorded stream (golden_big.json 1080p_30_thr8), and no launch repeated after an expired wait"""
    g = GOLDEN_BIG["1080p_30_thr8"]
    w, h, n = g["w"], g["h"], g["frames"]
    src = P.ClipEncoder(w, h, n)
    src.generate_synth()
    host = src.download()
    src.close()
    assert hashlib.md5(host.tobytes()).hexdigest() == g["input_md5"]
    t = torch.from_numpy(host).cuda().view(n, h * 3 // 2, w)
    ce = P.ClipEncoder(w, h, n, **flags(g["flags"]))
    ce.upload_device([t[i] for i in range(n)], "i420")
    t.zero_()                               # the frames have been read: the source may go
    out, sizes, st = ce.encode()
    ce.close()
    assert sizes == g["frame_bytes"]
    assert len(out) == g["bytes"] and hashlib.md5(out).hexdigest() == g["md5"]
    assert st.spin_relaunches == 0


@pytest.mark.parametrize("kw", [dict(slices=3), dict(kbps=200), dict(denoise=True), dict(slices=2, kbps=300, denoise=True)], ids=lambda k: "_".join(sorted(k)))
def test_i420_options_give_the_upload_stream(P, torch, kw):
    w, h, n = 176, 144, 5
    c = clips.make("scene", w, h, n)
    got, sizes, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload_device([i420_source(torch, f, w, h, "padded") for f in c], "i420"), gop=4, qp=28, **kw)
    up, up_sizes, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload(c), gop=4, qp=28, **kw)
    a = P.Encoder(w, h, gop=4, qp=28, **kw)
    devs = [a.encode_device(i420_source(torch, f, w, h, "separate"), "i420") for f in c]
    a.close()
    b = P.Encoder(w, h, gop=4, qp=28, **kw)
    host = [b.encode(f) for f in c]
    b.close()
    assert got == up and sizes == up_sizes
    assert devs == host
    if "kbps" not in kw and "denoise" not in kw:
        assert got == oracle_lib.encode_clip(c, w, h, gop=4, qp=28, **kw)[0]


@pytest.mark.parametrize("denoise", [False, True])
def test_bounded_ring_fed_in_chunks_rewind_and_reupload(P, torch, denoise):
    w, h, n = 64, 48, 8
    c = clips.make("scene", w, h, n)
    whole, _, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload(c), gop=30, qp=26, denoise=denoise)
    ring = P.ClipEncoder(w, h, n, gop=30, qp=26, resident=3, denoise=denoise)
    with pytest.raises(P.H264EError):
        ring.upload_device([i420_source(torch, f, w, h, "packed") for f in c[:4]], "i420")
    parts = []
    for f0 in range(0, n, 3):
        ring.upload_device([i420_source(torch, f, w, h, "padded") for f in c[f0:f0 + 3]], "i420", first=f0)
        pos, up = C.c_int(), C.c_int()
        ring.L.H264E_clip_position(ring.c, C.byref(pos), C.byref(up))
        assert (pos.value, up.value) == (f0, min(f0 + 3, n))
        parts.append(ring.encode(rewind=(f0 == 0))[0])
    ring.close()
    assert b"".join(parts) == whole
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26, denoise=denoise)
    ce.upload_device([i420_source(torch, f, w, h, "separate") for f in c], "i420")
    first = ce.encode()[0]
    assert ce.encode()[0] == first == whole
    c2 = c.copy()
    c2[4:] = clips.make("synth", w, h, n)[4:]
    ce.upload_device([i420_source(torch, f, w, h, "packed") for f in c2[4:]], "i420", first=4)
    changed = ce.encode()[0]
    ce.close()
    want, _, _, _ = clip_stream(P, w, h, c2, lambda e: e.upload(c2), gop=30, qp=26, denoise=denoise)
    assert changed == want and changed != first


def test_encode_multi_with_device_input(P, torch):
    w, h, n = 64, 48, 5
    cs = [clips.make(name, w, h, n) for name in ("scene", "synth", "noise")]
    encs = [P.ClipEncoder(w, h, n, gop=30, qp=26) for _ in cs]
    for e, c, layout in zip(encs, cs, ("padded", "packed", "separate")):
        e.upload_device([i420_source(torch, f, w, h, layout) for f in c], "i420")
    outs = P.ClipEncoder.encode_multi(encs)
    for e in encs:
        e.close()
    for c, (out, sizes, _) in zip(cs, outs):
        assert (out, sizes) == oracle_lib.encode_clip(c, w, h, gop=30, qp=26)


# ---------------------------------------------------------------- NV12 and RGB against the model


@pytest.mark.parametrize("w,h,n,padded", [(64, 48, 3, False), (64, 48, 3, True), (202, 122, 3, True), (200, 120, 2, False), (2, 2, 3, True), (6, 6, 3, False),
                                          (18, 34, 3, True), (34, 50, 2, True), (1920, 1080, 2, False)])
def test_nv12_matches_model(P, torch, w, h, n, padded):
    c = clips.make("scene" if w >= 64 else "ramp", w, h, n)
    srcs = []
    for f in c:
        y, uv = M.i420_to_nv12(f, w, h)
        srcs.append((dev(torch, y, w + 5, 3), dev(torch, uv, w + 9, 1)) if padded else (dev(torch, y), dev(torch, uv)))
    model = np.stack([M.nv12_to_i420(*M.i420_to_nv12(f, w, h)) for f in c])
    got, sizes, slots, _ = clip_stream(P, w, h, c, lambda ce: ce.upload_device(srcs, "nv12"), gop=30, qp=26)
    up, up_sizes, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload(model), gop=30, qp=26)
    e = P.Encoder(w, h, gop=30, qp=26)
    parts = [e.encode_device(s, "nv12") for s in srcs]
    e.close()
    assert np.array_equal(slots, model), "slot contents differ from the model"
    assert got == up and sizes == up_sizes
    assert b"".join(parts) == up


@pytest.mark.parametrize("w,h,n,pb,stride_pad,offset", [
    (64, 48, 3, 3, 0, 0), (64, 48, 3, 4, 0, 0), (64, 48, 2, 3, 1, 1), (202, 122, 2, 3, 1, 0), (202, 122, 2, 4, 4, 2), (200, 120, 2, 4, 0, 0),
    (2, 2, 3, 3, 0, 0), (4, 4, 3, 4, 0, 0), (6, 6, 3, 3, 5, 1), (18, 34, 2, 3, 1, 0), (34, 50, 2, 4, 0, 0), (1920, 1080, 2, 3, 0, 0), (1920, 1080, 2, 4, 0, 0),
])
def test_rgb_matches_model(P, torch, w, h, n, pb, stride_pad, offset):
    rgb = M.rgb_clip(w, h, n, pb)
    model = np.stack([M.rgb_to_i420(f) for f in rgb])
    srcs = [dev(torch, f, w * pb + stride_pad, offset) for f in rgb]
    got, sizes, slots, _ = clip_stream(P, w, h, rgb, lambda ce: ce.upload_device(srcs, "rgb"), gop=30, qp=26)
    up, up_sizes, _, _ = clip_stream(P, w, h, rgb, lambda ce: ce.upload(model), gop=30, qp=26)
    e = P.Encoder(w, h, gop=30, qp=26)
    parts = [e.encode_device(s, "rgb") for s in srcs]
    e.close()
    assert np.array_equal(slots, model), "slot contents differ from the model"
    assert got == up and sizes == up_sizes
    assert b"".join(parts) == up


# ---------------------------------------------------------------- ordering, refusals, import order


def test_frame_written_on_another_stream_is_waited_for_and_may_be_reused_at_once(P, torch):
    """a torch kernel writes the frame on a non-default stream behind a long queue of other work; the frame is handed over at once with
    that stream as the producer: the encoder must see the finished frame.  Right after the call returns the tensor is overwritten: the
    encoder must already have read it."""
    w, h, n = 1920, 1080, 3
    src = P.ClipEncoder(w, h, n)
    src.generate_synth()
    c = src.download()
    src.close()
    want, _, _, _ = clip_stream(P, w, h, c, lambda ce: ce.upload(c), gop=30, qp=26)
    staged = torch.from_numpy(c).cuda().view(n, h * 3 // 2, w)
    frame = torch.zeros((h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    busy = torch.ones((4096, 4096), device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    # the clip encoder: frame by frame through ONE tensor that is rewritten for every frame and trashed after every call
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26)
    e = P.Encoder(w, h, gop=30, qp=26)
    parts = []
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream != 0
        for i in range(n):
            for _ in range(20):
                busy = busy @ busy * 1e-4           # milliseconds of queued work in front of the write
            frame.copy_(staged[i])                  # the producer: a device-to-device kernel / copy on stream s
            ce.upload_device([frame], "i420", first=i)
            frame.fill_(0x55)
            for _ in range(20):
                busy = busy @ busy * 1e-4
            frame.copy_(staged[i])
            parts.append(e.encode_device(frame, "i420"))
            frame.fill_(0xAA)
    out, _, _ = ce.encode()
    slots = ce.download()
    ce.close()
    e.close()
    torch.cuda.synchronize()
    assert np.array_equal(slots, c), "the ingest did not wait for the producer's stream, or read the frame after the call had returned"
    assert out == want
    assert b"".join(parts) == want


def test_host_pointers_are_refused(P, torch):
    w, h = 64, 48
    c = clips.make("scene", w, h, 2)
    host = np.ascontiguousarray(c[0])
    good = i420_source(torch, c[0], w, h, "separate")
    ce = P.ClipEncoder(w, h, 2, gop=30, qp=26)
    e = P.Encoder(w, h, gop=30, qp=26)
    base = host.ctypes.data
    for planes in ([(base, w), (base + w * h, w // 2), (base + w * h * 5 // 4, w // 2)],
                   [(good[0].data_ptr(), w), (base + w * h, w // 2), (good[2].data_ptr(), w // 2)]):
        with pytest.raises(P.H264EError, match="not memory of device"):
            ce.upload_device([planes], "i420")
        with pytest.raises(P.H264EError, match="not memory of device"):
            e.encode_device(planes, "i420")
    pos, up = C.c_int(), C.c_int()
    ce.L.H264E_clip_position(ce.c, C.byref(pos), C.byref(up))
    assert (pos.value, up.value) == (0, 0)
    # both encoders still work
    ce.upload_device([i420_source(torch, f, w, h, "separate") for f in c], "i420")
    want = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)[0]
    assert ce.encode()[0] == want
    assert b"".join(e.encode_device(i420_source(torch, f, w, h, "packed"), "i420") for f in c) == want
    ce.close()
    e.close()


def test_plane_reaching_beyond_its_allocation_is_refused(P, torch):
    """a plane that starts in device memory but whose rows (by the stride given) run out of its allocation -- one of torch's allocator
    segments -- is refused before any launch: the kernel would read whatever lies there, or fault.  Every plane position, both entry
    points; a stride that keeps the plane inside the allocation is accepted."""
    w, h = 64, 48
    c = clips.make("scene", w, h, 1)
    good = i420_source(torch, c[0], w, h, "separate")
    torch.cuda.synchronize()
    ok = [(t.data_ptr(), t.stride(0)) for t in good]
    ce = P.ClipEncoder(w, h, 1, gop=30, qp=26)
    e = P.Encoder(w, h, gop=30, qp=26)
    far = 1 << 30                                   # rows a gigabyte apart: the last one is 23 GB (47 GB for luma) behind the first
    for k in range(3):
        planes = list(ok)
        planes[k] = (ok[k][0], far)
        with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
            ce.upload_device([planes], "i420")
        with pytest.raises(P.H264EError, match="not memory of device|not inside one allocation"):
            e.encode_device(planes, "i420")
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    d = P.DevFrame(format=P.DEV_FORMAT_RGB, pixel_bytes=4)      # straight through the C struct: RGB rows a gigabyte apart
    d.plane[0], d.stride[0] = rgb.data_ptr(), far
    assert ce.L.H264E_clip_upload_device(ce.c, 0, 1, C.byref(d)) == -1
    pos, up = C.c_int(), C.c_int()
    ce.L.H264E_clip_position(ce.c, C.byref(pos), C.byref(up))
    assert (pos.value, up.value) == (0, 0)
    ce.upload_device([ok], "i420")
    want = oracle_lib.encode_clip(c, w, h, gop=30, qp=26)[0]
    assert ce.encode()[0] == want
    assert e.encode_device(ok, "i420") == want
    ce.close()
    e.close()


CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, %(tests)r)
order = sys.argv[1]
import pkg
if order == "torch_first":
    import torch
    torch.zeros(1, device="cuda")
    P = pkg.load_pkg(); P.load()
else:
    P = pkg.load_pkg(); P.load()
    warm = P.Encoder(64, 48, gop=30, qp=26)             # the library's HIP runtime is up before torch is imported
    import torch
import numpy as np
import clips, ingest_model as M
w, h, n = 64, 48, 4
c = clips.make("scene", w, h, n)
ce = P.ClipEncoder(w, h, n, gop=30, qp=26)
ce.upload(c)
want = ce.encode()[0]
ce.close()
s = torch.cuda.Stream()
with torch.cuda.stream(s):
    frames = [torch.from_numpy(f.reshape(h * 3 // 2, w).copy()).cuda() for f in c]
    ce = P.ClipEncoder(w, h, n, gop=30, qp=26)
    ce.upload_device(frames, "i420")
    got = ce.encode()[0]
    ce.close()
    rgb = M.rgb_clip(w, h, 1, 3)[0]
    e = P.Encoder(w, h, gop=30, qp=26)
    a = e.encode_device(torch.from_numpy(rgb).cuda(), "rgb")
    e.close()
e = P.Encoder(w, h, gop=30, qp=26)
b = e.encode(M.rgb_to_i420(rgb))
e.close()
assert got == want, "device I420 differs from upload()"
assert a == b, "device RGB differs from the model"
print("CHILD_OK", order, hashlib.md5(got).hexdigest())
"""


@pytest.mark.parametrize("order", ["torch_first", "library_first"])
def test_both_import_orders_of_torch_and_the_library(order):
    """torch brings a HIP runtime of its own, the library links the system's, both of soname libamdhip64.so.7.  A torch pointer and a
    torch stream must be usable by the library in either order.  Each order in a fresh child process, under a time limit of its own.

    What the loader does by itself: torch first -> ONE runtime, torch's copy serves the library's NEEDED libamdhip64.so.7.  Library
    first -> TWO: torch's libraries ask for the FILE "libamdhip64.so" (RPATH $ORIGIN), which the loaded system copy does not satisfy,
    and torch's second runtime then finds no device (hipErrorNoDevice at its first stream, seen on the MI355X).  binding.load() therefore
    maps torch's runtime file in front of the library where a torch installation has one (binding._share_torch_runtime), so that
    either order ends with one runtime; this test is what holds it to that."""
    env = dict(os.environ, H264E_SHARE_DEVICE="1")          # (an encoder that an earlier, failed test left open must not decide this one)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD % dict(tests=HERE), order], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "CHILD_OK " + order in r.stdout, "order %s: exit %d\n%s\n%s" % (order, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
