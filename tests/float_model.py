"""The float sample types of planar RGB device frames (include/h264e_mi355x.h H264E_DEV_SAMPLE_F16 / _BF16 / _F32; the kernels'
fq_quant in h264-lab_amd/csrc/enc_ingest.h and egr_float_sample in enc_egress.h), restated in numpy.  The project has no reference for
this: the IEEE definition below IS the definition (tests/test_float_model.py holds it to exact rational arithmetic).

In:  a sample x is widened to float32 (exact for float16 and bfloat16), then q = clamp(rint(x *32 255), 0, 255): ONE float32 multiply,
     round to nearest even.  NaN, -inf, negative values and -0.0 give 0; +inf and values above 1 give 255.  From q on the frame is the
     8-bit planar RGB frame (tests/rgbp_model.py).
Out: an 8-bit value v becomes float32 v /32 255, ONE correctly rounded division; float16 and bfloat16 are that float32 value rounded to
     nearest even.

Samples travel as bit patterns here (uint16 for float16 and bfloat16, uint32 for float32): numpy has no bfloat16."""
import numpy as np

KINDS = ("f16", "bf16", "f32")
BYTES = {"f16": 2, "bf16": 2, "f32": 4}
BITS = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32}
FORMAT = {"f16": "rgbp_f16", "bf16": "rgbp_bf16", "f32": "rgbp_f32"}
TYPESTR = {"f16": "<f2", "bf16": None, "f32": "<f4"}


def widen(bits, kind):
    """the float32 values of an array of bit patterns"""
    bits = np.ascontiguousarray(bits, BITS[kind])
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    if kind == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.view(np.float32)


def quantise(bits, kind):
    """the 8-bit samples of an array of bit patterns (same shape)"""
    with np.errstate(all="ignore"):
        t = np.rint(widen(bits, kind) * np.float32(255))
    t = np.where(np.isnan(t), np.float32(0), t)
    return np.clip(t, 0, 255).astype(np.uint8)


def bf16_round(f32):
    """float32 values to bfloat16 bit patterns, nearest even (finite values)"""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dequantise(u8, kind):
    """the bit patterns the way out writes for an array of 8-bit values (same shape)"""
    f = np.asarray(u8, np.uint8).astype(np.float32) / np.float32(255)
    if kind == "f16":
        return f.astype(np.float16).view(np.uint16)
    if kind == "bf16":
        return bf16_round(f).reshape(f.shape)
    return f.view(np.uint32)


def table(kind):
    """the 256 bit patterns of the way out"""
    return dequantise(np.arange(256, dtype=np.uint8), kind)


def encode(values, kind):
    """bit patterns of float values (float32 array), rounded to nearest even: for building test pictures"""
    f = np.ascontiguousarray(values, np.float32)
    if kind == "f16":
        with np.errstate(all="ignore"):
            return f.astype(np.float16).view(np.uint16)
    if kind == "bf16":
        return bf16_round(f).reshape(f.shape)
    return f.view(np.uint32).copy()


def f32_edge_bits():
    """the float32 bit patterns a quantiser can get wrong: every k/255, every float32 within 3 ulps of a rounding boundary (k + 0.5)/255 on
    both sides, signed zeros and infinities, NaNs, denormals, 1 +- ulp, and 2^16 random patterns from a fixed seed"""
    out = []
    k = np.arange(256, dtype=np.float32)
    out.append((k / np.float32(255)).view(np.uint32))
    mid = ((np.arange(-1, 256, dtype=np.float64) + 0.5) / 255).astype(np.float32).view(np.uint32).astype(np.int64)
    for d in range(-3, 4):
        out.append(((mid + d) & 0xFFFFFFFF).astype(np.uint32))       # sign-magnitude: +d is d ulps away from zero
    special = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FA00000,
               0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00800000, 0x80800000,
               0x3F800000, 0x3F800001, 0x3F7FFFFF, 0xBF800000, 0x3F000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3B808081, 0x3B008081, 0x3B008080, 0x3B008082]
    out.append(np.array(special, np.uint32))
    out.append(np.random.RandomState(20260819).randint(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(out)


def all_patterns_picture():
    """a 256 x 256 picture of 16-bit samples whose three channels each hold all 65536 bit patterns, in different orders"""
    i = np.arange(65536, dtype=np.uint32)
    return np.stack([i, 65535 - i, (i * 40503 + 12345) & 0xFFFF]).astype(np.uint16).reshape(3, 256, 256)


def f32_edge_picture():
    """the float32 edge set as a (3, h, 256) picture (h even, padded with 0.5), the channels in different orders"""
    e = f32_edge_bits()
    rows = (e.size + 255) // 256
    rows += rows & 1
    flat = np.full(rows * 256, 0x3F000000, np.uint32)
    flat[: e.size] = e
    return np.stack([flat, flat[::-1], np.roll(flat, 4099)]).reshape(3, rows, 256)


def ramp_picture(w, h, kind, seed=0):
    """a (3, h, w) picture of bit patterns: values in and a little around [0, 1], boundaries included"""
    rs = np.random.RandomState(1000 + seed + 7 * w + h)
    v = rs.uniform(-0.1, 1.1, (3, h, w)).astype(np.float32)
    pick = rs.randint(0, 4, v.shape)
    v = np.where(pick == 0, ((rs.randint(0, 256, v.shape) + 0.5) / 255).astype(np.float32), v)      # near a rounding boundary
    v = np.where(pick == 1, (rs.randint(0, 256, v.shape) / 255).astype(np.float32), v)              # an exact level
    return encode(v, kind)
