"""h264-lab on MI355X: the reference's H264E_* encoder API served by hand-written HIP kernels (gfx950).

Python is only a thin ctypes mirror of the C API in include/h264e_mi355x.h, for tests and bench.py; the
product is lib/libh264e_mi355x.so (+ lib/encode_app).  There is no CPU fallback: loading fails loudly when
the HIP library has not been built, and encoder creation fails when no HIP device is present.
"""
from .binding import (  # noqa: F401
    CreateParam, RunParam, IoYuv, Encoder, ClipEncoder, ClipParam, ClipStats, load, lib_path, build, H264EError,
    psnr_from_ssd, ssim_planes,
    DevFrame, DevWindow, dev_frame, dev_window, recon_out, encode_ladder, DEV_FORMAT_I420, DEV_FORMAT_NV12, DEV_FORMAT_RGB, DEV_FORMAT_RGBP, DEV_FORMAT_RGBP_F16, DEV_FORMAT_RGBP_BF16, DEV_FORMAT_RGBP_F32,
    DEV_FORMAT_I444, DEV_FORMAT_P010, DEV_FORMAT_P016, DEV_CHROMA_444, DEV_DEPTH,
    DEV_CHROMA_422, DEV_PACK_YUYV, DEV_PACK_UYVY, DEV_FORMAT_I422, DEV_FORMAT_NV16, DEV_FORMAT_YUYV, DEV_FORMAT_UYVY,
    DEV_FORMAT_P210, DEV_FORMAT_P216, DEV_FORMAT_Y210, DEV_FORMAT_Y216,
    DEV_SAMPLE_U8, DEV_SAMPLE_F16, DEV_SAMPLE_BF16, DEV_SAMPLE_F32, dev_format, H264E_SCENECUT_DEFAULT,
    MATRIX_UNSPECIFIED, MATRIX_BT709, MATRIX_BT601,
    TONEMAP_OFF, TONEMAP_PQ, TONECURVE_HABLE, TONECURVE_REINHARD, TONECURVE_CLIP, tonemap_args, tonemap_tables,
    STATUS_SUCCESS, STATUS_BAD_ARGUMENT, STATUS_BAD_PARAMETER, STATUS_BAD_FRAME_TYPE, FRAME_TYPE_DEFAULT, FRAME_TYPE_KEY, FRAME_TYPE_P,
)
from .shard import StreamShard, shard_ranges  # noqa: F401
