"""ctypes mirror of include/h264e_mi355x.h (same names, argument meaning and status codes as the reference API,
/root/reference/src/h264-lab.h:83-312)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB = os.path.join(HERE, "lib", "libh264e_mi355x.so")

STATUS_SUCCESS, STATUS_BAD_ARGUMENT, STATUS_BAD_PARAMETER, STATUS_BAD_FRAME_TYPE = 0, 1, 2, 3
STATUS_SIZE_NOT_MULTIPLE_16, STATUS_SIZE_NOT_MULTIPLE_2 = 4, 5
FRAME_TYPE_DEFAULT, FRAME_TYPE_KEY, FRAME_TYPE_P = 0, 6, 2


class H264EError(RuntimeError):
    pass


class CreateParam(C.Structure):  # h264-lab.h:83-172 (H264E_SVC_API=1, H264E_MAX_THREADS=0): 56 bytes
    _fields_ = [(n, C.c_int) for n in (
        "width", "height", "gop", "vbv_size_bytes", "vbv_overflow_empty_frame_flag", "vbv_underflow_stuffing_flag",
        "fine_rate_control_flag", "const_input_flag", "max_long_term_reference_frames", "enableNEON",
        "temporal_denoise_flag", "sps_id", "num_layers", "inter_layer_pred_flag")]


NALU_CB = C.CFUNCTYPE(None, C.POINTER(C.c_ubyte), C.c_int, C.c_void_p)


class RunParam(C.Structure):  # h264-lab.h:177-226: 48 bytes
    _fields_ = [("encode_speed", C.c_int), ("frame_type", C.c_int), ("long_term_idx_use", C.c_int),
                ("long_term_idx_update", C.c_int), ("desired_frame_bytes", C.c_int), ("qp_min", C.c_int),
                ("qp_max", C.c_int), ("desired_nalu_bytes", C.c_int), ("nalu_callback", NALU_CB),
                ("nalu_callback_token", C.c_void_p)]


class IoYuv(C.Structure):  # h264-lab.h:231-237: 40 bytes
    _fields_ = [("yuv", C.c_void_p * 3), ("stride", C.c_int * 3)]


class ClipParam(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("width", "height", "gop", "qp", "speed", "vbv_size_bytes", "device", "max_chains",
                                       "first_idr_pic_id_state")] + [("mv_clusters_in", C.c_int32 * 2), ("slices", C.c_int), ("kbps", C.c_int), ("resident_frames", C.c_int), ("keep_records", C.c_int)]


class ClipStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "encode_ms", "readback_ms", "assemble_ms", "mb_kernel_ms", "splice_kernel_ms")] + \
               [(n, C.c_int) for n in ("kernel_launches", "chains", "rounds", "reencoded_gops")] + \
               [("mv_clusters_out", C.c_int32 * 2), ("next_idr_pic_id_state", C.c_int), ("first_frame", C.c_int), ("frames", C.c_int), ("spin_relaunches", C.c_int),
                ("relaunches_timed", C.c_int), ("processed_mbs", C.c_longlong), ("delivered_mbs", C.c_longlong), ("first_frame_ms_after_relaunch", C.c_double),
                ("kept_key_frames", C.c_int), ("kept_key_rows", C.c_int)]


class DevFrame(C.Structure):  # H264E_dev_frame_t: a frame in device memory (checked against H264E_struct_size(2) at load)
    _fields_ = [("format", C.c_int), ("pixel_bytes", C.c_int), ("plane", C.c_void_p * 3), ("stride", C.c_int * 3), ("producer_stream", C.c_void_p)]


class DevWindow(C.Structure):  # H264E_dev_window_t: the source's size and the window of it that is reduced to the encoder's picture
    _fields_ = [(n, C.c_int) for n in ("src_width", "src_height", "crop_x", "crop_y", "crop_width", "crop_height")]


DEV_FORMAT_I420, DEV_FORMAT_NV12, DEV_FORMAT_RGB, DEV_FORMAT_RGBP = 0, 1, 2, 3
H264E_SCENECUT_DEFAULT = 128        # include/h264e_mi355x.h
DEV_SAMPLE_U8, DEV_SAMPLE_F16, DEV_SAMPLE_BF16, DEV_SAMPLE_F32 = 0x00, 0x10, 0x20, 0x30       # bits 4-5 of the format: planar RGB only
DEV_FORMAT_RGBP_F16, DEV_FORMAT_RGBP_BF16, DEV_FORMAT_RGBP_F32 = DEV_FORMAT_RGBP | DEV_SAMPLE_F16, DEV_FORMAT_RGBP | DEV_SAMPLE_BF16, DEV_FORMAT_RGBP | DEV_SAMPLE_F32
_DEV_FORMATS = {"i420": DEV_FORMAT_I420, "nv12": DEV_FORMAT_NV12, "rgb": DEV_FORMAT_RGB, "rgbp": DEV_FORMAT_RGBP,
                "rgbp_f16": DEV_FORMAT_RGBP_F16, "rgbp_bf16": DEV_FORMAT_RGBP_BF16, "rgbp_f32": DEV_FORMAT_RGBP_F32}
# decoder surfaces: 16-bit samples with `depth` significant bits (bits 8-11 of the format: I420 and NV12) and 4:4:4 chroma (bit 12: I420)
DEV_CHROMA_444 = 0x1000
DEV_FORMAT_I444 = DEV_FORMAT_I420 | DEV_CHROMA_444


def DEV_DEPTH(d):
    """H264E_DEV_DEPTH: the format bits of 16-bit samples with d = 9 .. 16 significant bits, LSB aligned (an MSB-aligned P010 surface: 16)"""
    return (int(d) - 8) << 8


DEV_FORMAT_P016 = DEV_FORMAT_P010 = DEV_FORMAT_NV12 | DEV_DEPTH(16)
_DEV_FORMATS["i444"] = DEV_FORMAT_I444
# the names of the 16-bit formats: (layout bits, the only depth the name allows or None for depth=)
_HBD_FORMATS = {"i420_16": (DEV_FORMAT_I420, None), "nv12_16": (DEV_FORMAT_NV12, None), "i444_16": (DEV_FORMAT_I444, None),
                "p010": (DEV_FORMAT_NV12, 16), "p016": (DEV_FORMAT_NV12, 16)}
# capture and pro-video surfaces: 4:2:2 chroma (bit 14: I420 and NV12) and its packed orders (bits 2-3: on I420 | 4:2:2 alone)
DEV_CHROMA_422, DEV_PACK_YUYV, DEV_PACK_UYVY = 0x4000, 0x4, 0x8
DEV_FORMAT_I422, DEV_FORMAT_NV16 = DEV_FORMAT_I420 | DEV_CHROMA_422, DEV_FORMAT_NV12 | DEV_CHROMA_422
DEV_FORMAT_YUYV, DEV_FORMAT_UYVY = DEV_FORMAT_I422 | DEV_PACK_YUYV, DEV_FORMAT_I422 | DEV_PACK_UYVY
DEV_FORMAT_P216 = DEV_FORMAT_P210 = DEV_FORMAT_NV16 | DEV_DEPTH(16)
DEV_FORMAT_Y216 = DEV_FORMAT_Y210 = DEV_FORMAT_YUYV | DEV_DEPTH(16)
_DEV_FORMATS.update({"i422": DEV_FORMAT_I422, "nv16": DEV_FORMAT_NV16, "yuyv": DEV_FORMAT_YUYV, "yuy2": DEV_FORMAT_YUYV, "uyvy": DEV_FORMAT_UYVY})
_HBD_FORMATS.update({"i422_16": (DEV_FORMAT_I422, None), "nv16_16": (DEV_FORMAT_NV16, None), "yuyv_16": (DEV_FORMAT_YUYV, None), "uyvy_16": (DEV_FORMAT_UYVY, None),
                     "p210": (DEV_FORMAT_NV16, 16), "p216": (DEV_FORMAT_NV16, 16), "y210": (DEV_FORMAT_YUYV, 16), "y216": (DEV_FORMAT_YUYV, 16)})
# float planar RGB: format code -> (bytes per sample, the torch dtype's name, the __cuda_array_interface__ typestr or None)
_FLOAT_SAMPLES = {DEV_FORMAT_RGBP_F16: (2, "float16", "<f2"), DEV_FORMAT_RGBP_BF16: (2, "bfloat16", None), DEV_FORMAT_RGBP_F32: (4, "float32", "<f4")}


def hip_runtimes():
    """the HIP runtime libraries mapped into this process (see _share_torch_runtime: more than one is a broken process)"""
    try:
        with open("/proc/self/maps") as f:
            return sorted({line.split()[-1] for line in f if "/libamdhip64.so" in line})
    except OSError:
        return []


def _one_runtime():
    r = hip_runtimes()
    if len(r) > 1:
        raise H264EError("device input: two HIP runtimes are loaded (%s): memory and streams of one are unknown to the other.  Load the "
                         "library that owns the frames BEFORE this one (and do not set H264E_SYSTEM_HIP=1 next to torch), so that one runtime serves both" % ", ".join(r))


def _float_format_of(a):
    """the float planar RGB format code of one array by its sample type, or (None, the type's name)"""
    if hasattr(a, "data_ptr") and hasattr(a, "stride"):
        name = str(getattr(a, "dtype", "?"))
        for f, (_, dtype, _) in _FLOAT_SAMPLES.items():
            if name == "torch." + dtype:
                return f, name
        return None, name
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        for f, (_, _, typestr) in _FLOAT_SAMPLES.items():
            if typestr is not None and cai["typestr"] == typestr:
                return f, typestr
        return None, cai["typestr"]
    return None, "a (pointer, stride) pair"


def _dev_array(a, f=None, u16=None):
    """(pointer, shape, strides in bytes, producer stream or None) of one device array: an object with data_ptr() / stride() / shape
    (a torch tensor), one with __cuda_array_interface__, or an explicit (pointer, row stride in bytes) pair -- whose shape is not
    known, so nothing about it is checked here.  f: one of the float planar RGB formats -- the array must hold that sample type;
    u16: the name of a 16-bit format -- the array must hold uint16 or int16 samples; otherwise 8-bit samples."""
    if isinstance(a, (tuple, list)) and len(a) == 2 and all(isinstance(x, int) for x in a):
        return int(a[0]), None, (int(a[1]),), None
    if u16 is not None:
        return _dev_array16(a, u16)
    if f is not None and _float_format_of(a)[0] != f:
        raise H264EError("device input: format %r takes %s samples, not %s" % ([k for k, v in _DEV_FORMATS.items() if v == f][0], _FLOAT_SAMPLES[f][1], _float_format_of(a)[1]))
    item = _FLOAT_SAMPLES[f][0] if f is not None else 1
    if hasattr(a, "data_ptr") and hasattr(a, "stride"):
        if f is None and a.element_size() != 1:
            raise H264EError("device input must be 8-bit samples, not %s" % (getattr(a, "dtype", "?"),))
        stream = None
        torch = sys.modules.get("torch")            # never imported here: a tensor in hand means the caller has
        if torch is not None and getattr(a, "is_cuda", False):
            stream = torch.cuda.current_stream(a.device)
        return int(a.data_ptr()), tuple(a.shape), tuple(int(x) * item for x in a.stride()), stream
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        if f is None and cai["typestr"] not in ("|u1", "<u1", ">u1", "|i1"):
            raise H264EError("device input must be 8-bit samples, not %s" % cai["typestr"])
        shape = tuple(cai["shape"])
        strides = cai.get("strides")
        if strides is None:
            strides, acc = [], item
            for d in reversed(shape):
                strides.insert(0, acc)
                acc *= d
        st = cai.get("stream")
        return int(cai["data"][0]), shape, tuple(int(x) for x in strides), (st if st not in (None, 1, 2) else None)
    raise H264EError("device input: expected a tensor, an object with __cuda_array_interface__ or a (pointer, stride) pair, got %r" % type(a))


def _dev_array16(a, name):
    """_dev_array for uint16 / int16 samples (strides in bytes); anything else is refused with its type in the message"""
    if hasattr(a, "data_ptr") and hasattr(a, "stride"):
        if str(getattr(a, "dtype", "?")) not in ("torch.uint16", "torch.int16"):
            raise H264EError("device input: format %r takes 16-bit samples (uint16 or int16), not %s" % (name, getattr(a, "dtype", "?")))
        stream = None
        torch = sys.modules.get("torch")
        if torch is not None and getattr(a, "is_cuda", False):
            stream = torch.cuda.current_stream(a.device)
        return int(a.data_ptr()), tuple(a.shape), tuple(int(x) * 2 for x in a.stride()), stream
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is not None:
        if cai["typestr"] not in ("<u2", "<i2"):
            raise H264EError("device input: format %r takes 16-bit samples (<u2 or <i2), not %s" % (name, cai["typestr"]))
        shape = tuple(cai["shape"])
        strides = cai.get("strides")
        if strides is None:
            strides, acc = [], 2
            for d in reversed(shape):
                strides.insert(0, acc)
                acc *= d
        st = cai.get("stream")
        return int(cai["data"][0]), shape, tuple(int(x) for x in strides), (st if st not in (None, 1, 2) else None)
    raise H264EError("device input: expected a tensor, an object with __cuda_array_interface__ or a (pointer, stride) pair, got %r" % type(a))


def _plane_n(a, rows, w, sb, what, u16):
    """one (rows, w) plane of sb-byte samples, last axis contiguous, any row stride: (pointer, row stride in bytes, stream)"""
    ptr, shape, strides, stream = _dev_array(a, u16=u16)
    if shape is not None and (tuple(shape) != (rows, w) or strides[1] != sb):
        raise H264EError("device input: %s must be a (%d, %d) array whose last axis is contiguous, got shape %r strides %r (bytes)" % (what, rows, w, shape, strides))
    return ptr, strides[0], stream


def _hbd_planes(frame, f, name, w, h):
    """the planes of a 16-bit and / or 4:4:4 frame: [(pointer, row stride in bytes, stream)]"""
    sb = 2 if f & 0xf00 else 1
    u16 = name if sb == 2 else None
    if f & DEV_CHROMA_444:
        if isinstance(frame, (tuple, list)) and len(frame) == 3:
            return [_plane_n(a, h, w, sb, what, u16) for a, what in zip(frame, "YUV")]
        ptr, shape, strides, st = _dev_array(frame, u16=u16)
        if shape is None or tuple(shape) != (3, h, w) or strides[2] != sb:
            raise H264EError("device input: 4:4:4 must be a (3, %d, %d) array whose last axis is contiguous (any channel and row strides), "
                             "or three (%d, %d) planes, got shape %r strides %r (bytes)" % (h, w, h, w, shape, strides))
        return [(ptr + c * strides[0], strides[1], st) for c in range(3)]
    if (f & 3) == DEV_FORMAT_NV12:
        if not isinstance(frame, (tuple, list)) or len(frame) != 2:
            raise H264EError("device input: NV12 takes (y, uv)")
        return [_plane_n(frame[0], h, w, sb, "Y", u16), _plane_n(frame[1], h // 2, w, sb, "UV", u16)]
    if isinstance(frame, (tuple, list)) and len(frame) == 3:
        return [_plane_n(frame[0], h, w, sb, "Y", u16), _plane_n(frame[1], h // 2, w // 2, sb, "U", u16), _plane_n(frame[2], h // 2, w // 2, sb, "V", u16)]
    ptr, shape, strides, st = _dev_array(frame, u16=u16)
    if shape is not None and (tuple(shape) != (h * 3 // 2, w) or tuple(strides) != (w * sb, sb)):
        raise H264EError("device input: packed 16-bit I420 must be a contiguous (%d, %d) array, got shape %r strides %r (bytes)" % (h * 3 // 2, w, shape, strides))
    if shape is None and strides[0] != w * sb:
        raise H264EError("device input: packed 16-bit I420 has row stride %d, got %d" % (w * sb, strides[0]))
    return [(ptr, w * sb, st), (ptr + w * h * sb, w // 2 * sb, st), (ptr + (w * h + (w // 2) * (h // 2)) * sb, w // 2 * sb, st)]


def _c422_planes(frame, f, name, w, h):
    """the planes of a 4:2:2 frame of 8- or 16-bit samples: [(pointer, row stride in bytes, stream)]"""
    sb = 2 if f & 0xf00 else 1
    u16 = name if sb == 2 else None
    several = isinstance(frame, (tuple, list)) and not all(isinstance(x, int) for x in frame)
    if f & (DEV_PACK_YUYV | DEV_PACK_UYVY):
        if several and len(frame) == 1:
            frame = frame[0]
        ptr, shape, strides, st = _dev_array(frame, u16=u16)
        if shape is not None and not ((tuple(shape) == (h, 2 * w) and strides[1] == sb) or (tuple(shape) == (h, w, 2) and tuple(strides[1:]) == (2 * sb, sb))):
            raise H264EError("device input: packed 4:2:2 must be a (%d, %d) or (%d, %d, 2) array whose rows are contiguous (any row stride), got shape %r strides %r (bytes)"
                             % (h, 2 * w, h, w, shape, strides))
        return [(ptr, strides[0], st)]
    if several and len(frame) == (2 if (f & 3) == DEV_FORMAT_NV12 else 3):
        if (f & 3) == DEV_FORMAT_NV12:
            return [_plane_n(frame[0], h, w, sb, "Y", u16), _plane_n(frame[1], h, w, sb, "UV", u16)]
        return [_plane_n(frame[0], h, w, sb, "Y", u16), _plane_n(frame[1], h, w // 2, sb, "U", u16), _plane_n(frame[2], h, w // 2, sb, "V", u16)]
    if several:
        raise H264EError("device input: %s takes %s or one (%d, %d) array" % ("NV16" if (f & 3) == DEV_FORMAT_NV12 else "I422", "(y, uv)" if (f & 3) == DEV_FORMAT_NV12 else "(y, u, v)", 2 * h, w))
    ptr, shape, strides, st = _dev_array(frame, u16=u16)
    if (f & 3) == DEV_FORMAT_NV12:                  # the luma rows, then as many rows of U,V pairs: any row stride
        if shape is not None and (tuple(shape) != (2 * h, w) or strides[1] != sb):
            raise H264EError("device input: NV16 in one array must be (%d, %d) with a contiguous last axis, got shape %r strides %r (bytes)" % (2 * h, w, shape, strides))
        return [(ptr, strides[0], st), (ptr + h * strides[0], strides[0], st)]
    if shape is not None and (tuple(shape) != (2 * h, w) or tuple(strides) != (w * sb, sb)):
        raise H264EError("device input: packed I422 must be a contiguous (%d, %d) array, got shape %r strides %r (bytes)" % (2 * h, w, shape, strides))
    if shape is None and strides[0] != w * sb:
        raise H264EError("device input: packed I422 has row stride %d, got %d" % (w * sb, strides[0]))
    return [(ptr, w * sb, st), (ptr + w * h * sb, w // 2 * sb, st), (ptr + (w * h + (w // 2) * h) * sb, w // 2 * sb, st)]


def _require_uint8(a):
    """planar RGB takes unsigned 8-bit samples only: anything else is refused here, with its type in the message"""
    if hasattr(a, "data_ptr") and hasattr(a, "stride"):
        ok, name = str(getattr(a, "dtype", "")).endswith("uint8"), getattr(a, "dtype", "?")
    elif getattr(a, "__cuda_array_interface__", None) is not None:
        name = a.__cuda_array_interface__["typestr"]
        ok = name in ("|u1", "<u1", ">u1")
    else:
        return
    if not ok:
        raise H264EError("device input: planar RGB must be uint8 samples, not %s" % (name,))


def _dev_plane(a, rows, row_bytes, what):
    """one 2-D plane (or (h, w, c) pixels, c = the last axis): (pointer, row stride, stream)"""
    ptr, shape, strides, stream = _dev_array(a)
    if shape is not None:
        inner = 1
        for d in shape[1:]:
            inner *= d
        dense = all(strides[i] == (strides[i + 1] * shape[i + 1]) for i in range(1, len(shape) - 1)) and strides[-1] == 1
        if len(shape) < 2 or shape[0] != rows or inner != row_bytes or not dense:
            raise H264EError("device input: %s must be %d rows of %d contiguous bytes, got shape %r strides %r" % (what, rows, row_bytes, shape, strides))
    return ptr, strides[0], stream


def _float_plane(a, f, rows, w, what):
    """one (rows, w) plane of float samples, last axis contiguous: (pointer, row stride in bytes, stream)"""
    ptr, shape, strides, stream = _dev_array(a, f)
    if shape is not None and (tuple(shape) != (rows, w) or strides[1] != _FLOAT_SAMPLES[f][0]):
        raise H264EError("device input: %s must be a (%d, %d) array whose last axis is contiguous, got shape %r strides %r (bytes)" % (what, rows, w, shape, strides))
    return ptr, strides[0], stream


def dev_format(fmt, frame=None, depth=None):
    """the H264E_DEV_FORMAT_* code of a format name or number; "rgbpf" is float planar RGB with the sample type of `frame` (a float16,
    bfloat16 or float32 array, or three such planes); depth: the significant bits (9 .. 16, default 16) of the 16-bit names "i420_16",
    "nv12_16", "i444_16", "i422_16", "nv16_16", "yuyv_16" and "uyvy_16" ("p010", "p016", "p210", "p216", "y210" and "y216" are MSB aligned: 16)"""
    if isinstance(fmt, str) and fmt in _HBD_FORMATS:
        base, fixed = _HBD_FORMATS[fmt]
        d = 16 if depth is None else int(depth)
        if not 9 <= d <= 16 or (fixed is not None and d != fixed):
            raise H264EError("device input: depth %r for format %r (%s)" % (depth, fmt, "9 .. 16" if fixed is None else "an MSB-aligned surface: %d, or leave it out" % fixed))
        return base | DEV_DEPTH(d)
    if depth is not None:
        raise H264EError("device input: depth=%r with format %r: a depth belongs to the 16-bit formats %s" % (depth, fmt, ", ".join(sorted(_HBD_FORMATS))))
    if fmt != "rgbpf":
        return _DEV_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)
    arrays = list(frame) if isinstance(frame, (tuple, list)) and len(frame) == 3 else [frame]
    found = [_float_format_of(a) for a in arrays]
    for f, name in found:
        if f is None or f != found[0][0]:
            raise H264EError("device input: format 'rgbpf' takes float16, bfloat16 or float32 samples (one type for all planes), not %s" % (name,))
    return found[0][0]


def dev_frame(frame, fmt, w, h, stream=None, depth=None):
    """H264E_dev_frame_t for one frame of a w x h picture.  fmt "i420": three 2-D planes (y, u, v) or one packed (h*3/2, w) array;
    "nv12": (y of (h, w), uv of (h/2, w)); "rgb": one (h, w, 3 | 4) array; "rgbp": one uint8 (3, h, w) array (CHW: any channel and row
    strides, so views work without a copy) or three 2-D planes (r, g, b); "rgbp_f16", "rgbp_bf16", "rgbp_f32": the same of float
    samples in [0, 1], and "rgbpf" whichever of the three the array's dtype says; "i444": three (h, w) planes (y, u, v) or one (3, h, w)
    array with any channel and row strides; "i420_16", "nv12_16" ("p010", "p016"), "i444_16": the same shapes as their 8-bit layouts of
    torch.uint16 / torch.int16 ("<u2" / "<i2") samples with `depth` significant bits, LSB aligned (default 16: an MSB-aligned decoder
    surface), quantised to 8 bits as they are loaded.  4:2:2, chroma of the luma's height and half its width: "i422" three planes (y, u of
    (h, w/2), v) or one contiguous (2h, w) array in ffmpeg's buffer order; "nv16" (y, uv of (h, w)) or one (2h, w) array, luma rows first;
    "yuyv" (alias "yuy2") and "uyvy" ONE (h, 2w) or (h, w, 2) array with any row stride; "i422_16", "nv16_16", "yuyv_16", "uyvy_16" the same
    shapes of 16-bit samples with `depth`, "p210" / "p216" (nv16_16) and "y210" / "y216" (yuyv_16) MSB aligned.  Arrays: torch tensors, anything with
    __cuda_array_interface__ (no bfloat16 there), or (pointer, row stride in bytes) pairs.  stream: the hipStream_t (an int) that writes
    the frame; by default torch's current stream for torch tensors.  Returns (DevFrame, the objects that must stay alive during the call)."""
    f = dev_format(fmt, frame, depth)
    pb, planes = 0, []
    _one_runtime()
    if f & DEV_CHROMA_422 and not f & ~0x4f0d and (f & 3) < 2:
        planes = _c422_planes(frame, f, fmt, w, h)
    elif f & 0x1f00 and not f & ~0x1f03 and (f & 3) < 2:
        planes = _hbd_planes(frame, f, fmt, w, h)
    elif f == DEV_FORMAT_I420:
        if isinstance(frame, (tuple, list)) and len(frame) == 3:
            planes = [_dev_plane(frame[0], h, w, "Y"), _dev_plane(frame[1], h // 2, w // 2, "U"), _dev_plane(frame[2], h // 2, w // 2, "V")]
        else:
            ptr, shape, strides, st = _dev_array(frame)
            if shape is not None and (tuple(shape) != (h * 3 // 2, w) or tuple(strides) != (w, 1)):
                raise H264EError("device input: packed I420 must be a contiguous (%d, %d) array, got shape %r strides %r" % (h * 3 // 2, w, shape, strides))
            if shape is None and strides[0] != w:
                raise H264EError("device input: packed I420 has row stride %d, got %d" % (w, strides[0]))
            planes = [(ptr, w, st), (ptr + w * h, w // 2, st), (ptr + w * h + (w // 2) * (h // 2), w // 2, st)]
    elif f == DEV_FORMAT_NV12:
        if not isinstance(frame, (tuple, list)) or len(frame) != 2:
            raise H264EError("device input: NV12 takes (y, uv)")
        planes = [_dev_plane(frame[0], h, w, "Y"), _dev_plane(frame[1], h // 2, w, "UV")]
    elif f == DEV_FORMAT_RGB:
        ptr, shape, strides, st = _dev_array(frame)
        if shape is None:
            raise H264EError("device input: RGB needs an array with a shape (h, w, 3 | 4)")
        pb = shape[-1] if len(shape) == 3 else 0
        planes = [_dev_plane(frame, h, w * pb, "RGB")]
    elif f == DEV_FORMAT_RGBP:
        if isinstance(frame, (tuple, list)) and len(frame) == 3:
            for a in frame:
                _require_uint8(a)
            planes = [_dev_plane(a, h, w, what) for a, what in zip(frame, "RGB")]
        else:
            _require_uint8(frame)
            ptr, shape, strides, st = _dev_array(frame)
            if shape is None or tuple(shape) != (3, h, w) or strides[2] != 1:
                raise H264EError("device input: planar RGB must be a (3, %d, %d) array whose last axis is contiguous (any channel and row strides), "
                                 "or three (%d, %d) planes, got shape %r strides %r" % (h, w, h, w, shape, strides))
            planes = [(ptr + c * strides[0], strides[1], st) for c in range(3)]
    elif f in _FLOAT_SAMPLES:
        if isinstance(frame, (tuple, list)) and len(frame) == 3:
            planes = [_float_plane(a, f, h, w, what) for a, what in zip(frame, "RGB")]
        else:
            ptr, shape, strides, st = _dev_array(frame, f)
            if shape is None or tuple(shape) != (3, h, w) or strides[2] != _FLOAT_SAMPLES[f][0]:
                raise H264EError("device input: float planar RGB must be a (3, %d, %d) array whose last axis is contiguous (any channel and row strides), "
                                 "or three (%d, %d) planes, got shape %r strides %r (bytes)" % (h, w, h, w, shape, strides))
            planes = [(ptr + c * strides[0], strides[1], st) for c in range(3)]
    else:
        raise H264EError("device input: unknown format %r" % (fmt,))
    d = DevFrame(format=f, pixel_bytes=pb)
    for k, (ptr, stride, _) in enumerate(planes):
        d.plane[k], d.stride[k] = ptr, stride
    if stream is None:
        # torch's current stream; its default stream has handle 0, which the C API reads as "the caller has synchronised": make it so
        for st in {id(p[2]): p[2] for p in planes if p[2] is not None}.values():
            handle = getattr(st, "cuda_stream", st)
            if handle:
                stream = handle
            elif hasattr(st, "synchronize"):
                st.synchronize()
    d.producer_stream = int(stream) if stream else None
    return d, frame


def recon_out(fmt, w, h, device=0):
    """a fresh torch uint8 destination on GPU `device` for the reconstruction of a w x h picture: "i420" one packed (h*3/2, w) tensor,
    "nv12" (y of (h, w), uv of (h/2, w)), "rgb" (h, w, 3), "rgbp" (3, h, w); "rgbp_f16" / "rgbp_bf16" / "rgbp_f32" a (3, h, w) tensor of
    that float type, "rgbpf" float32"""
    f = DEV_FORMAT_RGBP_F32 if fmt == "rgbpf" else _DEV_FORMATS.get(fmt, fmt) if isinstance(fmt, str) else int(fmt)
    shapes = {DEV_FORMAT_I420: [(h * 3 // 2, w)], DEV_FORMAT_NV12: [(h, w), (h // 2, w)], DEV_FORMAT_RGB: [(h, w, 3)], DEV_FORMAT_RGBP: [(3, h, w)]}
    shapes.update({k: [(3, h, w)] for k in _FLOAT_SAMPLES})
    if f not in shapes:
        raise H264EError("read_recon_device: unknown format %r" % (fmt,))
    try:
        import torch
    except ImportError:
        raise H264EError("read_recon_device: out=None returns a torch tensor and torch cannot be imported -- pass the destination as out=")
    dtype = getattr(torch, _FLOAT_SAMPLES[f][1]) if f in _FLOAT_SAMPLES else torch.uint8
    made = [torch.empty(s, dtype=dtype, device=torch.device("cuda", device)) for s in shapes[f]]
    return made[0] if len(made) == 1 else tuple(made)


MATRIX_UNSPECIFIED, MATRIX_BT709, MATRIX_BT601 = 0, 1, 6       # include/h264e_mi355x.h (H.264 Table E-5)
_COLORS = {"bt709": (MATRIX_BT709, 0), "bt601": (MATRIX_BT601, 0), "bt709-full": (MATRIX_BT709, 1), "bt601-full": (MATRIX_BT601, 1)}


def color_pair(color):
    """(matrix, full_range) of a colour option: "bt709", "bt601", "bt709-full", "bt601-full", or such a pair (the library checks the values)"""
    if isinstance(color, str):
        if color not in _COLORS:
            raise H264EError("color %r: one of %s, or a (matrix, full_range) pair" % (color, ", ".join(sorted(_COLORS))))
        return _COLORS[color]
    try:
        matrix, full = color
        return int(matrix), int(full)
    except (TypeError, ValueError):
        raise H264EError("color %r: one of %s, or a (matrix, full_range) pair" % (color, ", ".join(sorted(_COLORS))))


TONEMAP_OFF, TONEMAP_PQ = 0, 1                                 # include/h264e_mi355x.h
TONECURVE_HABLE, TONECURVE_REINHARD, TONECURVE_CLIP = 0, 1, 2
_TRANSFERS = {"off": TONEMAP_OFF, "pq": TONEMAP_PQ}
_CURVES = {"hable": TONECURVE_HABLE, "reinhard": TONECURVE_REINHARD, "clip": TONECURVE_CLIP}


def tonemap_args(tonemap):
    """(transfer, curve, peak_nits, ref_white_nits) of a tonemap option: "pq" (or "off" / None), or a dict {"transfer": "pq", "curve":
    "hable" | "reinhard" | "clip", "peak": 1000, "ref_white": 203} with any of the last three left out (the library checks the values)"""
    what = "tonemap %r: \"pq\", \"off\" or a dict with transfer, curve (%s), peak, ref_white" % (tonemap, ", ".join(sorted(_CURVES)))
    if tonemap is None:
        return TONEMAP_OFF, TONECURVE_HABLE, 0.0, 0.0
    if isinstance(tonemap, str):
        tonemap = {"transfer": tonemap}
    if not isinstance(tonemap, dict) or set(tonemap) - {"transfer", "curve", "peak", "ref_white"}:
        raise H264EError(what)
    transfer, curve = tonemap.get("transfer", "pq"), tonemap.get("curve", "hable")
    if isinstance(transfer, str):
        if transfer not in _TRANSFERS:
            raise H264EError(what)
        transfer = _TRANSFERS[transfer]
    if isinstance(curve, str):
        if curve not in _CURVES:
            raise H264EError(what)
        curve = _CURVES[curve]
    try:
        return int(transfer), int(curve), float(tonemap.get("peak", 0) or 0), float(tonemap.get("ref_white", 0) or 0)
    except (TypeError, ValueError):
        raise H264EError(what)


def tonemap_tables(tonemap="pq", lib=None):
    """H264E_tonemap_tables: the tables the tone-map kernel will use for this option (a pure host function): (ycc int32[8], eotf
    float32[1024], scale float32[1024], thresh float32[256])"""
    L = load(lib)
    ycc, eotf, scale, thresh = np.zeros(8, np.int32), np.zeros(1024, np.float32), np.zeros(1024, np.float32), np.zeros(256, np.float32)
    if L.H264E_tonemap_tables(*tonemap_args(tonemap), ycc.ctypes.data, eotf.ctypes.data, scale.ctypes.data, thresh.ctypes.data):
        raise _err(L, "H264E_tonemap_tables")
    return ycc, eotf, scale, thresh


def fps_pair(fps):
    """(num, den) of a frame-rate option: an int, or a (num, den) pair"""
    if isinstance(fps, (tuple, list)):
        if len(fps) != 2:
            raise H264EError("fps %r: an int or a (num, den) pair" % (fps,))
        return int(fps[0]), int(fps[1])
    if isinstance(fps, bool) or not isinstance(fps, (int, np.integer)):
        raise H264EError("fps %r: an int or a (num, den) pair" % (fps,))
    return int(fps), 1


def dev_window(src_size, crop, w, h):
    """(DevWindow or None, (width, height) of the frames to describe): None when neither src_size nor crop is given -- the frames have the
    picture's size and go through the plain ingest"""
    if src_size is None and crop is None:
        return None, (w, h)
    sw, sh = (int(v) for v in (src_size if src_size is not None else (w, h)))
    win = DevWindow(sw, sh, 0, 0, 0, 0)
    if crop is not None:
        win.crop_x, win.crop_y, win.crop_width, win.crop_height = (int(v) for v in crop)
        if win.crop_width == 0:
            raise H264EError("device input: a crop of width 0 (leave crop out for the whole source)")
    return win, (sw, sh)


def lib_path():
    return os.environ.get("H264E_LIB", _DEFAULT_LIB)


def build():
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), "all"], stdout=subprocess.DEVNULL)


_libs = {}


def _share_torch_runtime(path):
    """One HIP runtime per process, whichever of torch and this library comes first.  torch ships a libamdhip64.so of its own and its
    libraries ask the loader for that FILE; this library asks for the soname libamdhip64.so.7.  torch first: torch's copy serves both.
    Library first: the system copy is bound, torch maps its own next to it, and that second runtime finds no device at all (measured
    on an MI355X: hipErrorNoDevice at torch's first stream).  So where a torch installation with a runtime of its own exists, that file
    is mapped BEFORE the library is (torch is only located, not imported): the library then binds to it by soname, and a later
    `import torch` finds the same file already mapped.  H264E_SYSTEM_HIP=1 keeps the system runtime."""
    if os.environ.get("H264E_SYSTEM_HIP") == "1" or hip_runtimes():
        return
    try:
        with open(path, "rb") as f:
            if b"libamdhip64.so" not in f.read():
                return                      # (the emulation libraries: no HIP runtime at all)
        import importlib.util
        spec = importlib.util.find_spec("torch")
        rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else None
        if rt and os.path.exists(rt):
            C.CDLL(rt, mode=C.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass                                # no torch, or no runtime of its own: the system's


def load(path=None):
    path = path or lib_path()
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise H264EError("HIP library %s not built: run `make -C h264-lab_amd/csrc` (there is no CPU fallback)" % path)
    _share_torch_runtime(path)
    L = C.CDLL(path)
    L.H264E_sizeof.argtypes = [C.POINTER(CreateParam), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.H264E_init.argtypes = [C.c_void_p, C.POINTER(CreateParam)]
    L.H264E_encode.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RunParam), C.POINTER(IoYuv), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.H264E_set_vbv_state.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_set_vbv_state.restype = None
    L.H264E_set_slices.argtypes = [C.c_void_p, C.c_int]
    L.H264E_set_denoise.argtypes = [C.c_void_p, C.c_int]
    L.H264E_set_color.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_set_frame_rate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_clip_set_color.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_clip_set_frame_rate.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_set_tonemap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    L.H264E_clip_set_tonemap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
    L.H264E_tonemap_tables.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.H264E_tonemap_state.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.H264E_clip_tonemap_state.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.H264E_close.argtypes = [C.c_void_p]
    L.H264E_close.restype = None
    L.H264E_set_device.argtypes = [C.c_int]
    L.H264E_set_device.restype = None
    L.H264E_last_error.restype = C.c_char_p
    L.H264E_clip_open.argtypes = [C.POINTER(C.c_void_p), C.POINTER(ClipParam), C.c_int]
    L.H264E_clip_upload.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.H264E_clip_generate_synth.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32]
    L.H264E_clip_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_int, C.POINTER(ClipStats)]
    L.H264E_clip_rewind.argtypes = [C.c_void_p]
    L.H264E_clip_rewind.restype = None
    L.H264E_clip_read_recon.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.H264E_clip_set_ssd_output.argtypes = [C.c_void_p, C.c_void_p]
    L.H264E_clip_set_ssd_output.restype = None
    L.H264E_clip_set_ssim_output.argtypes = [C.c_void_p, C.c_void_p]
    L.H264E_clip_quality_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_read_quality.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.H264E_ssim_planes.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.H264E_clip_set_denoise.argtypes = [C.c_void_p, C.c_int]
    L.H264E_clip_set_key_frames.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.H264E_clip_set_scenecut.argtypes = [C.c_void_p, C.c_int]
    L.H264E_clip_read_scenecut.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.H264E_clip_scenecut_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_set_qp_schedule.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.H264E_clip_set_lookahead.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.H264E_clip_read_lookahead.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.H264E_clip_lookahead_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_set_lookahead_search.argtypes = [C.c_void_p, C.c_int]
    L.H264E_clip_read_lookahead_motion.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.H264E_clip_set_lookahead_tree.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.H264E_clip_read_lookahead_tree.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.H264E_clip_read_lookahead_tree_sums.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.H264E_clip_lookahead_tree_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_set_denoise_motion.argtypes = [C.c_void_p, C.c_int]
    L.H264E_clip_read_denoised.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.H264E_clip_read_denoise_motion.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.H264E_clip_denoise_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_position.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.H264E_clip_position.restype = None
    L.H264E_clip_revalidate.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.H264E_clip_restart.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.H264E_clip_close.argtypes = [C.c_void_p]
    L.H264E_clip_close.restype = None
    L.h264e_hip_device_count.restype = C.c_int
    L.H264E_struct_size.argtypes = [C.c_int]
    if L.H264E_struct_size(2) != C.sizeof(DevFrame):
        raise H264EError("%s: H264E_dev_frame_t has %d bytes, this binding's mirror %d" % (path, L.H264E_struct_size(2), C.sizeof(DevFrame)))
    L.H264E_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RunParam), C.POINTER(DevFrame), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.H264E_clip_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(DevFrame)]
    L.H264E_encode_device_scaled.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(RunParam), C.POINTER(DevFrame), C.POINTER(DevWindow), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.H264E_clip_upload_device_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(DevFrame), C.POINTER(DevWindow)]
    L.H264E_read_recon_device.argtypes = [C.c_void_p, C.POINTER(DevFrame)]
    L.H264E_clip_read_recon_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(DevFrame)]
    L.H264E_clip_output_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_input_time.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
    L.H264E_clip_download.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.H264E_dev_malloc.argtypes = [C.c_int, C.c_size_t]
    L.H264E_dev_malloc.restype = C.c_void_p
    L.H264E_dev_free.argtypes = [C.c_void_p]
    L.H264E_dev_free.restype = None
    L.H264E_dev_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    _libs[path] = L
    return L


def _err(L, what):
    return H264EError("%s: %s" % (what, (L.H264E_last_error() or b"").decode()))


def psnr_from_ssd(ssd, w, h):
    """dB per plane from sums of squared differences [..., 3] (Y, U, V) of a w x h picture: 10 log10(255^2 samples / ssd), inf for 0"""
    ssd = np.asarray(ssd, np.float64)
    samples = np.array([w * h, (w // 2) * (h // 2), (w // 2) * (h // 2)], np.float64)
    with np.errstate(divide="ignore"):
        return np.where(ssd > 0, 10.0 * np.log10(255.0 * 255.0 * samples / np.where(ssd > 0, ssd, 1.0)), np.inf)


def ssim_planes(a, b, device=None, lib=None):
    """H264E_ssim_planes: the SSIM (8x8 windows in steps of 4, as x264 and ffmpeg's filter) of two 2-D uint8 planes of one shape in GPU
    memory -- torch tensors (views with any row stride are fine, the last axis contiguous), objects with __cuda_array_interface__ --
    by the encoder's own kernel.  Work queued on the tensors' streams is waited for first.  Returns a float."""
    L = load(lib)
    pa, sha, sta, stream_a = _dev_array(a)
    pb, shb, stb, stream_b = _dev_array(b)
    if sha is None or shb is None or len(sha) != 2 or tuple(sha) != tuple(shb) or sta[1] != 1 or stb[1] != 1:
        raise H264EError("ssim_planes: two 2-D uint8 arrays of one shape whose last axis is contiguous, got shapes %r, %r strides %r, %r" % (sha, shb, sta, stb))
    for st in (stream_a, stream_b):
        if st is not None and hasattr(st, "synchronize"):
            st.synchronize()
    if device is None:
        dev = getattr(a, "device", None)
        device = dev.index if getattr(dev, "index", None) is not None else -1
    out = C.c_double()
    if L.H264E_ssim_planes(int(device), pa, sta[0], pb, stb[0], sha[1], sha[0], C.byref(out)):
        raise _err(L, "H264E_ssim_planes")
    return out.value


class Encoder:
    """Frame-at-a-time encoder through the reference API: H264E_sizeof -> H264E_init -> H264E_encode."""

    def __init__(self, width, height, gop=20, qp=33, speed=0, kbps=0, const_input=1, vbv_size_bytes=100000 // 8, lib=None, slices=0, denoise=False,
                 color=None, fps=None, tonemap=None):
        self.L = load(lib)
        self.w, self.h = width, height
        self.cp = CreateParam(width=width, height=height, gop=gop, vbv_size_bytes=vbv_size_bytes, const_input_flag=const_input,
                              enableNEON=1, num_layers=1)
        sp, ss = C.c_int(), C.c_int()
        st = self.L.H264E_sizeof(C.byref(self.cp), C.byref(sp), C.byref(ss))
        if st:
            raise H264EError("H264E_sizeof status %d" % st)
        self.sizeof_persist, self.sizeof_scratch = sp.value, ss.value
        self.persist = C.create_string_buffer(sp.value + 64)
        self.scratch = C.create_string_buffer(ss.value + 64)
        st = self.L.H264E_init(self.persist, C.byref(self.cp))
        if st:
            raise _err(self.L, "H264E_init status %d" % st)
        if slices and self.L.H264E_set_slices(self.persist, slices):
            raise H264EError("H264E_set_slices(%d) refused" % slices)
        if denoise and self.L.H264E_set_denoise(self.persist, 1):       # the reference's temporal_denoise_flag (--denoise)
            raise _err(self.L, "H264E_set_denoise refused")
        if color is not None:
            self.set_color(color)
        if fps is not None:
            self.set_frame_rate(fps)
        if tonemap is not None:
            self.set_tonemap(tonemap)
        self.rp = RunParam(encode_speed=speed)
        if kbps:
            self.rp.desired_frame_bytes = kbps * 1000 // 8 // 30  # minih264e_test.c:596-600
            self.rp.qp_min, self.rp.qp_max = 10, 50
        else:
            self.rp.qp_min = self.rp.qp_max = qp

    def encode(self, frame, frame_type=FRAME_TYPE_DEFAULT):
        """frame: uint8 array of w*h*3/2 (packed I420).  Returns the coded bytes of this frame."""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        w, h = self.w, self.h
        base = frame.ctypes.data
        io = IoYuv((C.c_void_p * 3)(base, base + w * h, base + w * h * 5 // 4), (C.c_int * 3)(w, w // 2, w // 2))
        self.rp.frame_type = frame_type
        data, n = C.c_void_p(), C.c_int()
        st = self.L.H264E_encode(self.persist, self.scratch, C.byref(self.rp), C.byref(io), C.byref(data), C.byref(n))
        if st:
            raise _err(self.L, "H264E_encode status %d" % st)
        return C.string_at(data, n.value)

    def encode_planes(self, y, u, v, frame_type=FRAME_TYPE_DEFAULT):
        """Three separately allocated planes with any row stride (H264E_io_yuv_t, h264-lab.h:231-237): y, u, v are 2-D uint8 arrays
        (views into larger buffers are fine) whose LAST axis is contiguous; the row stride is taken from the array.  With
        const_input_flag = 0 the reconstruction is written back into these arrays (h264-lab.h:6719-6723)."""
        for a in (y, u, v):
            assert a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1
        io = IoYuv((C.c_void_p * 3)(y.ctypes.data, u.ctypes.data, v.ctypes.data), (C.c_int * 3)(y.strides[0], u.strides[0], v.strides[0]))
        self.rp.frame_type = frame_type
        data, n = C.c_void_p(), C.c_int()
        st = self.L.H264E_encode(self.persist, self.scratch, C.byref(self.rp), C.byref(io), C.byref(data), C.byref(n))
        if st:
            raise _err(self.L, "H264E_encode status %d" % st)
        return C.string_at(data, n.value)

    def encode_device(self, frame, fmt, frame_type=FRAME_TYPE_DEFAULT, stream=None, src_size=None, crop=None, depth=None):
        """H264E_encode_device: the frame is taken from GPU memory (see dev_frame for what `frame` may be: fmt "i420", "nv12", "rgb", "rgbp" or float "rgbp_f16" / "rgbp_bf16" / "rgbp_f32" / "rgbpf");
        needs const_input=1.  The frame's memory may be reused as soon as this returns.  src_size=(w, h): the frame has that size and is
        reduced to the encoder's picture (H264E_encode_device_scaled), crop=(x, y, w, h): only that window of it.  depth: the significant
        bits of the 16-bit formats "i420_16" / "nv12_16" / "i444_16" / "i422_16" / "nv16_16" / "yuyv_16" / "uyvy_16" (9 .. 16, default 16)."""
        win, (sw, sh) = dev_window(src_size, crop, self.w, self.h)
        d, _keep = dev_frame(frame, fmt, sw, sh, stream, depth)
        self.rp.frame_type = frame_type
        data, n = C.c_void_p(), C.c_int()
        if win is not None:
            st = self.L.H264E_encode_device_scaled(self.persist, self.scratch, C.byref(self.rp), C.byref(d), C.byref(win), C.byref(data), C.byref(n))
        else:
            st = self.L.H264E_encode_device(self.persist, self.scratch, C.byref(self.rp), C.byref(d), C.byref(data), C.byref(n))
        if st:
            raise _err(self.L, "H264E_encode_device%s status %d" % ("_scaled" if win is not None else "", st))
        return C.string_at(data, n.value)

    def read_recon_device(self, fmt="rgbp", out=None, stream=None):
        """H264E_read_recon_device: the reconstruction of the last encoded frame -- what a decoder shows for it -- into GPU memory as
        fmt "i420", "nv12", "rgb" or "rgbp" (converted by the inverse of the encoder's colour matrix), or float planar RGB in [0, 1]:
        "rgbp_f16", "rgbp_bf16", "rgbp_f32", "rgbpf" (the type of `out`; float32 for out=None).  out: the destination, described
        like an input frame (see dev_frame: tensors, CHW views, tuples of planes, (pointer, stride) pairs); only the rows' bytes are
        written.  out=None: a fresh torch tensor on device $H264E_DEVICE (default 0) -- (h*3/2, w) packed, (y, uv), (h, w, 3) or
        (3, h, w).  stream: the hipStream_t whose queued work may still use `out`; by default torch's current stream.  Returns out."""
        if out is None:
            out = recon_out(fmt, self.w, self.h, int(os.environ.get("H264E_DEVICE", "0")))
        d, _keep = dev_frame(out, fmt, self.w, self.h, stream)
        st = self.L.H264E_read_recon_device(self.persist, C.byref(d))
        if st:
            raise _err(self.L, "H264E_read_recon_device status %d" % st)
        return out

    def read_quality(self, ssd=True, ssim=True):
        """H264E_read_quality: the last call's input, as it lies in the encoder's input slot, against the reconstruction it left:
        (ssd uint64 [3], ssim float64 [3]) for Y, U, V; a metric that was not asked for is None"""
        d = np.zeros(3, np.uint64) if ssd else None
        s = np.zeros(3, np.float64) if ssim else None
        st = self.L.H264E_read_quality(self.persist, d.ctypes.data if ssd else None, s.ctypes.data if ssim else None)
        if st:
            raise _err(self.L, "H264E_read_quality status %d" % st)
        return d, s

    def set_color(self, color):
        """H264E_set_color: how RGB / RGBP device input is converted and what every SPS signals ("bt709", "bt601", "bt709-full",
        "bt601-full" or a (matrix, full_range) pair; (0, 0) = the default); only before the first frame."""
        st = self.L.H264E_set_color(self.persist, *color_pair(color))
        if st:
            raise _err(self.L, "H264E_set_color status %d" % st)

    def set_tonemap(self, tonemap):
        """H264E_set_tonemap: 16-bit "i420_16" / "nv12_16" / "p010" / "p016" device frames of depth 10 .. 16 are taken as HDR10 (PQ,
        BT.2020) and tone-mapped to the 8-bit BT.709 picture; "pq", a dict (see tonemap_args), or "off" / None; only before the first frame."""
        st = self.L.H264E_set_tonemap(self.persist, *tonemap_args(tonemap))
        if st:
            raise _err(self.L, "H264E_set_tonemap status %d" % st)

    def tonemap_state(self):
        """(on, bytes of the device table buffer, bytes of the window surface): 0 = not allocated"""
        s = (C.c_longlong * 3)()
        if self.L.H264E_tonemap_state(self.persist, s):
            raise _err(self.L, "H264E_tonemap_state")
        return tuple(s)

    def set_frame_rate(self, fps):
        """H264E_set_frame_rate: an int or a (num, den) pair, (0, 0) = none; only before the first frame."""
        st = self.L.H264E_set_frame_rate(self.persist, *fps_pair(fps))
        if st:
            raise _err(self.L, "H264E_set_frame_rate status %d" % st)

    def set_vbv_state(self, vbv_size_bytes, vbv_fullness_bytes):
        """H264E_set_vbv_state (h264-lab.h:6898-6913)"""
        self.L.H264E_set_vbv_state(self.persist, vbv_size_bytes, vbv_fullness_bytes)

    def close(self):
        if self.persist is not None:
            self.L.H264E_close(self.persist)
            self.persist = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ClipEncoder:
    """Whole-clip streaming encode on one GPU (H264E_clip_* extension): consecutive frames as a temporal wavefront."""

    def __init__(self, width, height, nframes, gop=30, qp=26, speed=0, device=0, max_chains=0, lib=None,
                 clusters_in=(0, 0), idr_state=0, slices=0, kbps=0, resident=0, keep_records=0, denoise=False, key_frames=None, scenecut=0,
                 color=None, fps=None, quality=None, qp_schedule=None, abr_kbps=0, lookahead=0, qp_range=(0, 0), lookahead_search=0,
                 denoise_motion=0, lookahead_tree=0, tonemap=None):
        self.L = load(lib)
        self.w, self.h, self.n = width, height, nframes
        self._ssd = self._ssim = None           # the registered metric arrays [nframes][3], owned here while registered
        self._q_frames = 0
        self.par = ClipParam(width, height, gop, qp, speed, 100000 // 8, device, max_chains, idr_state, (C.c_int32 * 2)(*clusters_in), slices, kbps, resident, keep_records)
        self.c = C.c_void_p()
        if self.L.H264E_clip_open(C.byref(self.c), C.byref(self.par), nframes):
            raise _err(self.L, "H264E_clip_open")
        try:
            if denoise:
                self.set_denoise(True)
            if key_frames:
                self.set_key_frames(key_frames)
            if scenecut:
                self.set_scenecut(scenecut)
            if color is not None:
                self.set_color(color)
            if fps is not None:
                self.set_frame_rate(fps)
            if tonemap is not None:
                self.set_tonemap(tonemap)
            if quality:
                self.set_quality(**(quality if isinstance(quality, dict) else {}))
            if qp_schedule is not None and len(qp_schedule):
                self.set_qp_schedule(qp_schedule)
            if abr_kbps:
                self.set_lookahead(abr_kbps, lookahead, qp_range)
            if lookahead_search:
                self.set_lookahead_search(lookahead_search)
            if denoise_motion:
                self.set_denoise_motion(denoise_motion)
            if lookahead_tree:
                self.set_lookahead_tree(*(lookahead_tree if isinstance(lookahead_tree, (tuple, list)) else (lookahead_tree,)))
        except H264EError:
            self.close()
            raise

    def set_quality(self, ssd=True, ssim=True):
        """Per-frame metrics of the following encodes, computed on the device (H264E_clip_set_ssd_output / _set_ssim_output): sums of
        squared differences and / or SSIM, input against reconstruction.  read_quality() hands out the last call's."""
        self._ssd = np.zeros((self.n, 3), np.uint64) if ssd else None
        self._ssim = np.zeros((self.n, 3), np.float64) if ssim else None
        self.L.H264E_clip_set_ssd_output(self.c, self._ssd.ctypes.data if ssd else None)
        if self.L.H264E_clip_set_ssim_output(self.c, self._ssim.ctypes.data if ssim else None):
            self.L.H264E_clip_set_ssd_output(self.c, None)
            self._ssd = self._ssim = None
            raise _err(self.L, "H264E_clip_set_ssim_output")
        self._q_frames = 0

    def read_quality(self):
        """(ssd uint64 [frames, 3], ssim float64 [frames, 3]) of the frames of the last encode() / encode_multi, Y, U, V; a metric that is
        off is None"""
        n = self._q_frames
        return (self._ssd[:n].copy() if self._ssd is not None else None), (self._ssim[:n].copy() if self._ssim is not None else None)

    def quality_time(self, enable=True):
        """(HIP-event milliseconds inside the SSD launches, inside the SSIM launches, frames they covered) timed so far; switches the
        timing of later encodes on or off"""
        a, b, n = C.c_double(), C.c_double(), C.c_longlong()
        self.L.H264E_clip_quality_time(self.c, int(bool(enable)), C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def set_denoise(self, on):
        """The temporal denoiser (H264E_clip_set_denoise): only while the clip stands at frame 0."""
        if self.L.H264E_clip_set_denoise(self.c, int(bool(on))):
            raise _err(self.L, "H264E_clip_set_denoise")

    def set_denoise_motion(self, mode):
        """The motion-compensated temporal denoiser (H264E_clip_set_denoise_motion): 0 = off, 1 = the previous denoised picture displaced
        by the lookahead's motion field, 2 = by that field refined; needs set_lookahead_search(1..8) first; only while the clip stands at
        frame 0.  denoise=True / set_denoise(True) stay the plain denoiser."""
        if self.L.H264E_clip_set_denoise_motion(self.c, int(mode)):
            raise _err(self.L, "H264E_clip_set_denoise_motion")

    def read_denoised(self, frame):
        """The denoised picture of a frame whose slot is still in the device's ring (H264E_clip_read_denoised), either denoiser's: packed
        I420, uint8 [w*h*3/2]"""
        out = np.empty(self.w * self.h * 3 // 2, np.uint8)
        if self.L.H264E_clip_read_denoised(self.c, int(frame), out.ctypes.data):
            raise _err(self.L, "H264E_clip_read_denoised")
        return out

    def read_denoise_motion(self, frame):
        """(mv int8 [nby, nbx, 2] as (vx, vy), sad uint16 [nby, nbx]) of a filtered frame that is still in the device's ring
        (H264E_clip_read_denoise_motion): per 16x16 luma block the vector the motion-compensated denoiser used, in luma samples, and
        its SAD against the previous denoised picture."""
        nbx, nby = C.c_int(), C.c_int()
        self.L.H264E_clip_read_denoise_motion(self.c, -1, None, C.byref(nbx), C.byref(nby))
        cells = np.zeros((nby.value, nbx.value), np.uint32)
        if self.L.H264E_clip_read_denoise_motion(self.c, int(frame), cells.ctypes.data, None, None):
            raise _err(self.L, "H264E_clip_read_denoise_motion")
        mv = np.stack([(cells & 0xff).astype(np.uint8).view(np.int8), ((cells >> 8) & 0xff).astype(np.uint8).view(np.int8)], axis=-1)
        return mv, (cells >> 16).astype(np.uint16)

    def denoise_time(self):
        """(HIP-event milliseconds inside the motion-compensated denoiser's kernel launches since open, frames they filtered)"""
        ms, n = C.c_double(), C.c_longlong()
        if self.L.H264E_clip_denoise_time(self.c, C.byref(ms), C.byref(n)):
            raise _err(self.L, "H264E_clip_denoise_time")
        return ms.value, n.value

    def set_color(self, color):
        """H264E_clip_set_color (see Encoder.set_color): only while the clip stands at frame 0, and BEFORE the frames are uploaded --
        frames in the input ring keep the bytes they were converted to."""
        if self.L.H264E_clip_set_color(self.c, *color_pair(color)):
            raise _err(self.L, "H264E_clip_set_color")

    def set_tonemap(self, tonemap):
        """H264E_clip_set_tonemap (see Encoder.set_tonemap): only while the clip stands at frame 0, and BEFORE the frames are uploaded;
        kept across a rewind."""
        if self.L.H264E_clip_set_tonemap(self.c, *tonemap_args(tonemap)):
            raise _err(self.L, "H264E_clip_set_tonemap")

    def tonemap_state(self):
        """(on, bytes of the device table buffer, bytes of the window surface): 0 = not allocated"""
        s = (C.c_longlong * 3)()
        if self.L.H264E_clip_tonemap_state(self.c, s):
            raise _err(self.L, "H264E_clip_tonemap_state")
        return tuple(s)

    def set_frame_rate(self, fps):
        """H264E_clip_set_frame_rate: an int or a (num, den) pair, (0, 0) = none; only while the clip stands at frame 0."""
        if self.L.H264E_clip_set_frame_rate(self.c, *fps_pair(fps)):
            raise _err(self.L, "H264E_clip_set_frame_rate")

    def set_key_frames(self, frames):
        """Key frames in addition to the periodic ones (H264E_clip_set_key_frames): an ascending list of frame numbers, [] clears it;
        only while the clip stands at frame 0."""
        frames = [int(f) for f in frames]
        if self.L.H264E_clip_set_key_frames(self.c, (C.c_int * max(len(frames), 1))(*frames), len(frames)):
            raise _err(self.L, "H264E_clip_set_key_frames")

    def set_scenecut(self, threshold=H264E_SCENECUT_DEFAULT):
        """Scene-cut detection (H264E_clip_set_scenecut): threshold in 1/1024 of the picture, 0 = off; only while the clip stands at frame 0."""
        if self.L.H264E_clip_set_scenecut(self.c, int(threshold)):
            raise _err(self.L, "H264E_clip_set_scenecut")

    def read_scenecut(self):
        """(dist, is_cut) of the frames encoded so far: D(f) as int32, and whether the detector made f a key frame, as bool"""
        nxt = C.c_int()
        self.L.H264E_clip_position(self.c, C.byref(nxt), None)
        dist, cut = np.zeros(nxt.value, np.int32), np.zeros(nxt.value, np.uint8)
        if self.L.H264E_clip_read_scenecut(self.c, 0, nxt.value, dist.ctypes.data, cut.ctypes.data):
            raise _err(self.L, "H264E_clip_read_scenecut")
        return dist, cut.astype(bool)

    def set_qp_schedule(self, qp):
        """A QP per frame (H264E_clip_set_qp_schedule): one value in 10..51 for every frame of the clip, [] clears it; only while the clip
        stands at frame 0.  The stream is the reference's for qp_min = qp_max = qp[f] on frame f."""
        q = np.asarray(qp, np.int64).reshape(-1)
        bad = np.flatnonzero((q < 0) | (q > 255))           # what a byte cannot carry to the library is refused here, in its words
        if len(bad):
            raise H264EError("H264E_clip_set_qp_schedule: set_qp_schedule: QP %d of frame %d is outside 10..51" % (q[bad[0]], bad[0]))
        q = np.ascontiguousarray(q, np.uint8)
        if self.L.H264E_clip_set_qp_schedule(self.c, q.ctypes.data if len(q) else None, len(q)):
            raise _err(self.L, "H264E_clip_set_qp_schedule")

    def set_lookahead(self, kbps, window=0, qp_range=(0, 0)):
        """The lookahead rate control (H264E_clip_set_lookahead): this project's own controller, NOT the reference's kbps mode -- one
        QP per window of `window` frames (0 = default), chosen inside qp_range (zeros = 10..50) from a cost pass over the input;
        kbps 0 switches it off; only while the clip stands at frame 0."""
        if self.L.H264E_clip_set_lookahead(self.c, int(kbps), int(window), int(qp_range[0]), int(qp_range[1])):
            raise _err(self.L, "H264E_clip_set_lookahead")

    def read_lookahead(self, costs=True, qp=True):
        """((intra uint64, inter uint64, intra_blocks int32), qp uint8) of the frames encoded so far: the cost records I(f), P(f), N(f)
        of the lookahead controller's cost pass as a triple, and the QP each frame was given; costs=False gives (None, None, None) for
        the triple, qp=False gives None for the QPs."""
        nxt = C.c_int()
        self.L.H264E_clip_position(self.c, C.byref(nxt), None)
        n = nxt.value
        i, p, b, q = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.uint8)
        if self.L.H264E_clip_read_lookahead(self.c, 0, n, i.ctypes.data if costs else None, p.ctypes.data if costs else None,
                                            b.ctypes.data if costs else None, q.ctypes.data if qp else None):
            raise _err(self.L, "H264E_clip_read_lookahead")
        return (i, p, b) if costs else (None, None, None), None if not qp else q

    def set_lookahead_search(self, r):
        """Motion search in the lookahead's cost pass (H264E_clip_set_lookahead_search): r = 0 switches it off, 1..8 searches +-r
        half-resolution samples per 8x8 block; only while the clip stands at frame 0 and before any frame has been analysed with
        another range."""
        if self.L.H264E_clip_set_lookahead_search(self.c, int(r)):
            raise _err(self.L, "H264E_clip_set_lookahead_search")

    def read_lookahead_motion(self, frame):
        """(mv int8 [nby, nbx, 2] as (dx, dy), cost uint16 [nby, nbx]) of an analysed frame whose field is still in the device's ring
        (H264E_clip_read_lookahead_motion): per 8x8 block of the half-resolution picture the vector the cost pass found, in
        half-resolution samples, and its SAD."""
        nbx, nby = C.c_int(), C.c_int()
        self.L.H264E_clip_read_lookahead_motion(self.c, -1, None, C.byref(nbx), C.byref(nby))
        cells = np.zeros((nby.value, nbx.value), np.uint32)
        if self.L.H264E_clip_read_lookahead_motion(self.c, int(frame), cells.ctypes.data, None, None):
            raise _err(self.L, "H264E_clip_read_lookahead_motion")
        mv = np.stack([(cells & 0xff).astype(np.uint8).view(np.int8), ((cells >> 8) & 0xff).astype(np.uint8).view(np.int8)], axis=-1)
        return mv, (cells >> 16).astype(np.uint16)

    def set_lookahead_tree(self, strength, ahead=-1):
        """The cost tree over the lookahead's motion field (H264E_clip_set_lookahead_tree): per-frame QP offsets inside a window, strength
        in quarter QP steps per doubling of a frame's importance (0 = off, 1..16), ahead = frames behind a window that its tree starts
        from (0..255, below 0 = the default); needs set_lookahead and set_lookahead_search(1..8) first; only while the clip stands at
        frame 0."""
        if self.L.H264E_clip_set_lookahead_tree(self.c, int(strength), int(ahead)):
            raise _err(self.L, "H264E_clip_set_lookahead_tree")

    def read_lookahead_tree(self, frame):
        """uint64 [nby, nbx]: what the blocks of a frame of a planned window received from the frames behind it
        (H264E_clip_read_lookahead_tree), as long as the map is in the device's ring"""
        nbx, nby = C.c_int(), C.c_int()
        self.L.H264E_clip_read_lookahead_tree(self.c, -1, None, C.byref(nbx), C.byref(nby))
        cells = np.zeros((nby.value, nbx.value), np.uint64)
        if self.L.H264E_clip_read_lookahead_tree(self.c, int(frame), cells.ctypes.data, None, None):
            raise _err(self.L, "H264E_clip_read_lookahead_tree")
        return cells

    def read_lookahead_tree_sums(self):
        """(S uint64, delta int8, base_qp uint8) of the frames encoded so far (H264E_clip_read_lookahead_tree_sums): what each frame
        received in the run that planned its window, the QP offset that became, and its window's base QP"""
        nxt = C.c_int()
        self.L.H264E_clip_position(self.c, C.byref(nxt), None)
        n = nxt.value
        s, d, q = np.zeros(n, np.uint64), np.zeros(n, np.int8), np.zeros(n, np.uint8)
        if self.L.H264E_clip_read_lookahead_tree_sums(self.c, 0, n, s.ctypes.data, d.ctypes.data, q.ctypes.data):
            raise _err(self.L, "H264E_clip_read_lookahead_tree_sums")
        return s, d, q

    def lookahead_tree_time(self):
        """(HIP-event milliseconds inside the cost tree's kernel launches since open, frame steps they made)"""
        ms, n = C.c_double(), C.c_longlong()
        self.L.H264E_clip_lookahead_tree_time(self.c, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def lookahead_time(self):
        """(HIP-event milliseconds inside the cost pass' kernel launches since open, frames they analysed)"""
        ms, n = C.c_double(), C.c_longlong()
        self.L.H264E_clip_lookahead_time(self.c, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def scenecut_time(self):
        """(HIP-event milliseconds inside the detector's kernel launches since open, frames they analysed)"""
        ms, n = C.c_double(), C.c_longlong()
        self.L.H264E_clip_scenecut_time(self.c, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def upload(self, clip, first=0):
        clip = np.ascontiguousarray(clip, dtype=np.uint8)
        n = clip.size // (self.w * self.h * 3 // 2)
        if self.L.H264E_clip_upload(self.c, first, n, clip.ctypes.data):
            raise _err(self.L, "H264E_clip_upload")

    def upload_device(self, frames, fmt, first=0, stream=None, src_size=None, crop=None, depth=None):
        """H264E_clip_upload_device: `frames` is a sequence of frames in GPU memory (see dev_frame: fmt "i420", "nv12", "rgb", "rgbp" or float "rgbp_f16" / "rgbp_bf16" / "rgbp_f32" / "rgbpf"), frame
        first + i from frames[i].  Their memory may be reused as soon as this returns.  src_size=(w, h): the frames have that size and are
        reduced to the clip's picture (H264E_clip_upload_device_scaled), crop=(x, y, w, h): only that window of them.  depth: the
        significant bits of the 16-bit formats "i420_16" / "nv12_16" / "i444_16" / "i422_16" / "nv16_16" / "yuyv_16" / "uyvy_16" (9 .. 16, default 16)."""
        win, (sw, sh) = dev_window(src_size, crop, self.w, self.h)
        made = [dev_frame(f, fmt, sw, sh, stream, depth) for f in frames]
        arr = (DevFrame * max(len(made), 1))(*[m[0] for m in made])
        if win is not None:
            if self.L.H264E_clip_upload_device_scaled(self.c, first, len(made), arr, C.byref(win)):
                raise _err(self.L, "H264E_clip_upload_device_scaled")
        elif self.L.H264E_clip_upload_device(self.c, first, len(made), arr):
            raise _err(self.L, "H264E_clip_upload_device")

    def input_time(self, enable=True):
        """(HIP-event milliseconds inside the ingest / scale launches of the device uploads timed so far, their frames); switches the
        timing of later uploads on or off"""
        ms, n = C.c_double(), C.c_longlong()
        self.L.H264E_clip_input_time(self.c, int(bool(enable)), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def download(self, first=0, nframes=None):
        """the resident input frames (packed I420) back to the host: whole-clip residency only"""
        n = self.n - first if nframes is None else nframes
        buf = np.empty((n, self.w * self.h * 3 // 2), np.uint8)
        if self.L.H264E_clip_download(self.c, first, n, buf.ctypes.data):
            raise _err(self.L, "H264E_clip_download")
        return buf

    def generate_synth(self, first=0, nframes=None, t0=0, seed=1):
        if self.L.H264E_clip_generate_synth(self.c, first, self.n if nframes is None else nframes, t0, seed):
            raise _err(self.L, "H264E_clip_generate_synth")

    def encode(self, profile=False, rewind=True, cap=None):
        """Encode the uploaded frames that are not encoded yet (after a rewind: all of them).  Returns (bytes, sizes, stats)."""
        if rewind:
            self.L.H264E_clip_rewind(self.c)
        cap = cap or (self.w * self.h * 3 // 2 * self.n + (1 << 20))
        out = np.empty(cap, np.uint8)
        nb = C.c_size_t()
        sizes = (C.c_int * self.n)()
        st = ClipStats()
        if self.L.H264E_clip_encode(self.c, out.ctypes.data, cap, C.byref(nb), sizes, int(profile), C.byref(st)):
            raise _err(self.L, "H264E_clip_encode")
        self._q_frames = st.frames
        return out[: nb.value].tobytes(), list(sizes)[: st.frames], st

    @staticmethod
    def encode_multi(encoders):
        """Encode several clips of one picture size on one device AT THE SAME TIME (H264E_clip_encode_multi: one host thread per clip,
        the clips' launches merged into one grid per round).  Returns a list of (bytes, sizes, stats), one per encoder."""
        n = len(encoders)
        L = encoders[0].L
        caps = [e.w * e.h * 3 // 2 * e.n + (1 << 20) for e in encoders]
        outs = [np.empty(c, np.uint8) for c in caps]
        sizes = [(C.c_int * e.n)() for e in encoders]
        sts = (ClipStats * n)()
        nb = (C.c_size_t * n)()
        for e in encoders:
            L.H264E_clip_rewind(e.c)
        L.H264E_clip_encode_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                              C.POINTER(C.POINTER(C.c_int)), C.POINTER(ClipStats)]
        L.H264E_clip_encode_multi.restype = C.c_int
        clips = (C.c_void_p * n)(*[e.c for e in encoders])
        outp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        capa = (C.c_size_t * n)(*caps)
        fb = (C.POINTER(C.c_int) * n)(*[C.cast(s, C.POINTER(C.c_int)) for s in sizes])
        if L.H264E_clip_encode_multi(clips, n, outp, capa, nb, fb, sts):
            raise _err(L, "H264E_clip_encode_multi")
        for i, e in enumerate(encoders):
            e._q_frames = sts[i].frames
        return [(outs[i][: nb[i]].tobytes(), list(sizes[i])[: sts[i].frames], sts[i]) for i in range(n)]

    def revalidate(self, exact_in):
        """(restart_frame or -1, restart_state, end_state) for the exact mv_clusters state in front of this shard"""
        rf = C.c_int()
        rs, es = (C.c_int32 * 2)(), (C.c_int32 * 2)()
        if self.L.H264E_clip_revalidate(self.c, (C.c_int32 * 2)(*exact_in), C.byref(rf), rs, es):
            raise _err(self.L, "H264E_clip_revalidate")
        return rf.value, (rs[0], rs[1]), (es[0], es[1])

    def restart(self, frame, state):
        if self.L.H264E_clip_restart(self.c, frame, (C.c_int32 * 2)(*state)):
            raise _err(self.L, "H264E_clip_restart")

    def read_records(self, frame):
        """per-macroblock (mvx, mvy, type, used_cand) of an encoded frame (keep_records=1)"""
        nmb = ((self.w + 15) // 16) * ((self.h + 15) // 16)
        buf = np.empty(nmb * 2, np.int32)
        self.L.H264E_clip_read_records.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        if self.L.H264E_clip_read_records(self.c, frame, buf.ctypes.data):
            raise _err(self.L, "H264E_clip_read_records")
        mv, rest = buf[0::2], buf[1::2]
        mvx = ((mv & 0xffff) ^ 0x8000) - 0x8000
        mvy = mv >> 16
        typ = ((rest & 0xff) ^ 0x80) - 0x80
        return [(int(mvx[i]), int(mvy[i]), int(typ[i]), int((rest[i] >> 8) & 0xff)) for i in range(nmb)]

    def read_recon(self, frame):
        cw, ch = (self.w + 15) // 16 * 16, (self.h + 15) // 16 * 16
        buf = np.empty(cw * ch * 3 // 2, np.uint8)
        if self.L.H264E_clip_read_recon(self.c, frame, buf.ctypes.data):
            raise _err(self.L, "H264E_clip_read_recon")
        return buf

    def read_recon_device(self, frame, fmt="rgbp", out=None, stream=None):
        """H264E_clip_read_recon_device: the reconstruction of `frame` (one of the last frames encoded, as read_recon), cropped to the
        picture, into GPU memory; fmt, out and stream as Encoder.read_recon_device (out=None: a fresh torch tensor on the clip's device)"""
        if out is None:
            out = recon_out(fmt, self.w, self.h, self.par.device)
        d, _keep = dev_frame(out, fmt, self.w, self.h, stream)
        if self.L.H264E_clip_read_recon_device(self.c, frame, C.byref(d)):
            raise _err(self.L, "H264E_clip_read_recon_device")
        return out

    def output_time(self, enable=True):
        """(HIP-event milliseconds inside the launches of the read_recon_device calls timed so far, their number); switches the timing
        of later calls on or off"""
        ms, n = C.c_double(), C.c_longlong()
        self.L.H264E_clip_output_time(self.c, int(bool(enable)), C.byref(ms), C.byref(n))
        return ms.value, n.value

    def close(self):
        if self.c:
            if self._ssd is not None or self._ssim is not None:     # the library must not keep pointers into arrays that go away
                self.L.H264E_clip_set_ssd_output(self.c, None)
                self.L.H264E_clip_set_ssim_output(self.c, None)
                self._ssd = self._ssim = None
            self.L.H264E_clip_close(self.c)
            self.c = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def encode_ladder(frames, fmt, src_size, rungs, crop=None, depth=None, **common):
    """One source in GPU memory, several encodes of it at different sizes.  frames: the device frames (see dev_frame), all of
    src_size=(w, h); rungs: a list of (width, height, dict of ClipEncoder options); crop=(x, y, w, h): the window of the source that every
    rung shows; common: ClipEncoder options of all rungs (a rung's own win), tonemap="pq" for an HDR10 source among them.  One ClipEncoder per rung is fed from the same frames -- by
    the scaling kernel, or the plain ingest where a rung has the window's size -- rungs of equal picture size are encoded at the same
    time (ClipEncoder.encode_multi), the others one after another.  depth: the significant bits of a 16-bit fmt (see dev_frame).
    Returns one (bytes, sizes, stats) per rung, in the order given."""
    frames = list(frames)
    sw, sh = (int(v) for v in src_size)
    encs, out = [], [None] * len(rungs)
    try:
        for w, h, opts in rungs:
            ce = ClipEncoder(w, h, len(frames), **dict(common, **(opts or {})))
            encs.append(ce)
            if crop is None and (w, h) == (sw, sh):
                ce.upload_device(frames, fmt, depth=depth)
            else:
                ce.upload_device(frames, fmt, src_size=(sw, sh), crop=crop, depth=depth)
        groups = {}
        for i, ce in enumerate(encs):
            groups.setdefault((ce.w, ce.h), []).append(i)
        for idx in groups.values():
            res = ClipEncoder.encode_multi([encs[i] for i in idx]) if len(idx) > 1 else [encs[idx[0]].encode()]
            for i, r in zip(idx, res):
                out[i] = r
    finally:
        for ce in encs:
            ce.close()
    return out
