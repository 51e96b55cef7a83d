"""The colour feature's definitions (include/h264e_mi355x.h H264E_set_color / H264E_set_frame_rate), restated in numpy and
plain Python.  The reference has neither RGB input nor a VUI, so these ARE the definitions:

  - the conversion keeps ingest_model's form with one of four coefficient rows,

        Y = ((yr R + yg G + yb B + 128) >> 8) + yo                        per pixel
        m = (a + b + c + d + 2) >> 2                                      per channel over each 2x2 block
        U = ((ur Rm + ug Gm + ub Bm + 128) >> 8) + 128,  V likewise       (arithmetic shifts, no clamp)

    the rows being Kr / Kb (BT.601: 0.299 / 0.114, BT.709: 0.2126 / 0.0722) scaled by 219/255 (luma) and 224/255 (chroma) for limited
    range, by 1 for full range, times 256, rounded to nearest -- and then ONE coefficient per row moved by 1 where needed so that luma
    sums to 220 or 256 and chroma to 0.  In the full-range chroma rows the 0.5 weight is 127, not the rounded 128 -- with 128 a
    saturated blue gives U = ((128*255 + 128) >> 8) + 128 = 256, a saturated red the same in V -- and the nearer of the other two
    coefficients takes the 1 that keeps the sum at 0.  Grey stays neutral, and no result leaves 16..235 / 16..240 or 0..255: check_row
    proves it over all 2^24 inputs.  With a window the order of rgbp_model holds: scale each channel, round to 8 bits, then this matrix;
  - the SPS carries the VUI of H.264 E.1.1 with exactly the fields vui_fields() lists; an Annex-B splitter, the un-escaper and an SPS
    parser that returns every field are here for the stream tests.

matrix is the H.264 matrix_coefficients code: 1 = BT.709, 6 = BT.601, 0 = unspecified (converted as 6 limited, nothing signalled)."""
import numpy as np

import ingest_model
import rgbp_model

BT709, BT601 = 1, 6

# (matrix, full_range): ((yr, yg, yb), yo, (ur, ug, ub), (vr, vg, vb))
ROWS = {
    (6, 0): ((66, 129, 25), 16, (-38, -74, 112), (112, -94, -18)),
    (1, 0): ((47, 157, 16), 16, (-26, -86, 112), (112, -102, -10)),
    (6, 1): ((77, 150, 29), 0, (-43, -84, 127), (127, -107, -20)),
    (1, 1): ((54, 183, 19), 0, (-29, -98, 127), (127, -116, -11)),
}
NAMES = {"bt709": (1, 0), "bt601": (6, 0), "bt709-full": (1, 1), "bt601-full": (6, 1)}
NEW_ROWS = [(1, 0), (6, 1), (1, 1)]         # what the feature adds: (6, 0) is the matrix the project had


def row(matrix, full):
    return ROWS[(matrix or 6, full)]


def ranges(full):
    """(luma lo, luma hi, chroma lo, chroma hi) the results must stay inside"""
    return (0, 255, 0, 255) if full else (16, 235, 16, 240)


def derived_row(matrix, full):
    """the row from its recipe, BEFORE the one-coefficient correction: every entry within 1 of the table's"""
    kr, kb = {6: (0.299, 0.114), 1: (0.2126, 0.0722)}[matrix]
    kg = 1 - kr - kb
    sy, sc = (1.0, 1.0) if full else (219 / 255, 224 / 255)
    y = [256 * sy * k for k in (kr, kg, kb)]
    u = [256 * sc * 0.5 * k / (1 - kb) for k in (-kr, -kg, 1 - kb)]
    v = [256 * sc * 0.5 * k / (1 - kr) for k in (1 - kr, -kg, -kb)]
    return [[int(np.floor(x + 0.5)) for x in r] for r in (y, u, v)]


def matrix_planes(r, g, b, mr, mg, mb, matrix, full):
    """int64 arrays: (Y of the pixels r, g, b; U, V of the block means mr, mg, mb) -- NOT cast to uint8"""
    (yr, yg, yb), yo, (ur, ug, ub), (vr, vg, vb) = row(matrix, full)
    y = ((yr * r + yg * g + yb * b + 128) >> 8) + yo
    u = ((ur * mr + ug * mg + ub * mb + 128) >> 8) + 128            # numpy's >> on signed integers is arithmetic
    v = ((vr * mr + vg * mg + vb * mb + 128) >> 8) + 128
    return y, u, v


def rgb_to_i420(rgb, matrix=0, full=0):
    """(h, w, 3 | 4) uint8 -> packed I420 (ingest_model.rgb_to_i420 with the chosen row)"""
    c = np.asarray(rgb)[:, :, :3].astype(np.int64)
    m = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
    y, u, v = matrix_planes(c[:, :, 0], c[:, :, 1], c[:, :, 2], m[:, :, 0], m[:, :, 1], m[:, :, 2], matrix, full)
    ylo, yhi, clo, chi = ranges(full)
    assert y.min() >= ylo and y.max() <= yhi and min(u.min(), v.min()) >= clo and max(u.max(), v.max()) <= chi
    return ingest_model.pack(y, u, v)


def to_i420(chw, matrix=0, full=0):
    """(3, h, w) uint8 -> the packed I420 picture the input slot holds"""
    chw = np.asarray(chw)
    assert chw.ndim == 3 and chw.shape[0] == 3 and chw.dtype == np.uint8
    return rgb_to_i420(np.ascontiguousarray(chw.transpose(1, 2, 0)), matrix, full)


def scale_to_i420(chw, dw, dh, crop=None, matrix=0, full=0):
    """a window of the (3, H, W) source -> dw x dh: rgbp_model's scaled, rounded RGB picture, then the matrix"""
    return to_i420(rgbp_model.scale_rgb(chw, dw, dh, crop), matrix, full)


def corner_frame(w, h):
    """(3, h, w): the eight corner colours of the RGB cube in vertical bands of 2x2 blocks (w, h even; bands repeat)"""
    f = np.empty((3, h, w), np.uint8)
    for x in range(0, w, 2):
        k = (x // 2) % 8
        for c in range(3):
            f[c, :, x: x + 2] = 255 * ((k >> c) & 1)
    return f


def check_row(matrix, full, chunk=1 << 20):
    """every one of the 2^24 (R, G, B) through the row, vectorised in chunks: the ranges before any uint8 cast (a 2x2 block of one colour
    has that colour as its mean, and every mean is some triple of bytes: the chroma rows are covered too), grey, black and white"""
    ylo, yhi, clo, chi = ranges(full)
    for lo in range(0, 1 << 24, chunk):
        n = np.arange(lo, lo + chunk, dtype=np.int64)
        r, g, b = n >> 16, (n >> 8) & 255, n & 255
        y, u, v = matrix_planes(r, g, b, r, g, b, matrix, full)
        assert y.min() >= ylo and y.max() <= yhi, (matrix, full, lo, int(y.min()), int(y.max()))
        assert u.min() >= clo and u.max() <= chi and v.min() >= clo and v.max() <= chi, \
            "matrix %d full %d: U %d..%d, V %d..%d, allowed %d..%d" % (matrix, full, u.min(), u.max(), v.min(), v.max(), clo, chi)
    k = np.arange(256, dtype=np.int64)
    y, u, v = matrix_planes(k, k, k, k, k, k, matrix, full)
    assert (u == 128).all() and (v == 128).all(), "grey is not neutral"
    assert (int(y[0]), int(y[255])) == (ylo, yhi), "black / white"
    assert (np.diff(y) >= 0).all()


# ---------------------------------------------------------------- Annex B and the SPS


def split_annexb(stream):
    """the NAL units of an Annex-B byte stream, each without its start code (still escaped)"""
    s = bytes(stream)
    starts, i = [], s.find(b"\x00\x00\x01")
    while i >= 0:
        starts.append(i)
        i = s.find(b"\x00\x00\x01", i + 3)
    nals = []
    for k, a in enumerate(starts):
        end = starts[k + 1] if k + 1 < len(starts) else len(s)
        while k + 1 < len(starts) and end > a + 3 and s[end - 1] == 0:      # the zero_byte of a 4-byte start code (a NAL ends with a non-zero byte)
            end -= 1
        nals.append(s[a + 3: end])
    assert b"".join(b"\x00\x00\x00\x01" + n for n in nals) == s, "the product writes 4-byte start codes and nothing between NALs"
    return nals


def unescape(nal):
    """the RBSP of a NAL: emulation_prevention_three_bytes removed"""
    out, zeros = bytearray(), 0
    for b in bytes(nal):
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


class _Bits:
    def __init__(self, data):
        self.d, self.p = data, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | ((self.d[self.p >> 3] >> (7 - (self.p & 7))) & 1)
            self.p += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + (self.u(z) if z else 0)


def parse_sps(nal):
    """every field of a baseline SPS NAL (escaped, without start code), in order, as a dict; "vui" is None or a dict of every VUI field
    that is present; asserts that nothing but the stop bit and alignment zeros follows"""
    rbsp = unescape(nal)
    b = _Bits(rbsp)
    f = {}
    f["nal_header"] = b.u(8)
    assert f["nal_header"] & 0x1f == 7
    f["profile_idc"], f["constraint_flags"], f["level_idc"] = b.u(8), b.u(8), b.u(8)
    assert f["profile_idc"] == 66
    f["sps_id"] = b.ue()
    f["log2_max_frame_num_minus4"] = b.ue()
    f["pic_order_cnt_type"] = b.ue()
    assert f["pic_order_cnt_type"] == 2
    f["num_ref_frames"] = b.ue()
    f["gaps_in_frame_num_value_allowed_flag"] = b.u(1)
    f["pic_width_in_mbs_minus1"], f["pic_height_in_map_units_minus1"] = b.ue(), b.ue()
    f["frame_mbs_only_flag"] = b.u(1)
    assert f["frame_mbs_only_flag"] == 1
    f["direct_8x8_inference_flag"] = b.u(1)
    f["frame_cropping_flag"] = b.u(1)
    if f["frame_cropping_flag"]:
        f["frame_crop"] = (b.ue(), b.ue(), b.ue(), b.ue())
    f["vui_parameters_present_flag"] = b.u(1)
    f["vui"] = None
    if f["vui_parameters_present_flag"]:
        v = f["vui"] = {}
        v["aspect_ratio_info_present_flag"] = b.u(1)
        assert not v["aspect_ratio_info_present_flag"]
        v["overscan_info_present_flag"] = b.u(1)
        assert not v["overscan_info_present_flag"]
        v["video_signal_type_present_flag"] = b.u(1)
        if v["video_signal_type_present_flag"]:
            v["video_format"], v["video_full_range_flag"], v["colour_description_present_flag"] = b.u(3), b.u(1), b.u(1)
            if v["colour_description_present_flag"]:
                v["colour_primaries"], v["transfer_characteristics"], v["matrix_coefficients"] = b.u(8), b.u(8), b.u(8)
        v["chroma_loc_info_present_flag"] = b.u(1)
        assert not v["chroma_loc_info_present_flag"]
        v["timing_info_present_flag"] = b.u(1)
        if v["timing_info_present_flag"]:
            v["num_units_in_tick"], v["time_scale"], v["fixed_frame_rate_flag"] = b.u(32), b.u(32), b.u(1)
        v["nal_hrd_parameters_present_flag"], v["vcl_hrd_parameters_present_flag"] = b.u(1), b.u(1)
        assert not v["nal_hrd_parameters_present_flag"] and not v["vcl_hrd_parameters_present_flag"]
        v["pic_struct_present_flag"] = b.u(1)
        v["bitstream_restriction_flag"] = b.u(1)
        assert not v["bitstream_restriction_flag"]
    assert b.u(1) == 1, "rbsp_stop_one_bit"
    assert b.p <= 8 * len(rbsp) and (b.p + 7) // 8 == len(rbsp), "bytes behind the SPS"
    while b.p < 8 * len(rbsp):
        assert b.u(1) == 0, "alignment bits"
    return f


def vui_fields(matrix=0, full=0, fps=None):
    """what parse_sps must return as "vui" for a colour and a frame rate (num, den): None when neither is set"""
    if not matrix and not fps:
        return None
    v = dict(aspect_ratio_info_present_flag=0, overscan_info_present_flag=0, video_signal_type_present_flag=int(matrix != 0))
    if matrix:
        v.update(video_format=5, video_full_range_flag=full, colour_description_present_flag=1,
                 colour_primaries=matrix, transfer_characteristics=matrix, matrix_coefficients=matrix)
    v.update(chroma_loc_info_present_flag=0, timing_info_present_flag=int(bool(fps)))
    if fps:
        v.update(num_units_in_tick=fps[1], time_scale=2 * fps[0], fixed_frame_rate_flag=1)
    v.update(nal_hrd_parameters_present_flag=0, vcl_hrd_parameters_present_flag=0, pic_struct_present_flag=0, bitstream_restriction_flag=0)
    return v


def is_sps(nal):
    return (nal[0] & 0x1f) == 7


def compare_streams(got, want, matrix=0, full=0, fps=None):
    """`got` is `want` (a stream without VUI) with nothing but its SPSs changed: same NAL count, every other NAL identical, every SPS
    parsing to the other's fields plus exactly vui_fields(...).  Returns the SPS NALs of `got`."""
    a, b = split_annexb(got), split_annexb(want)
    assert len(a) == len(b) and len(a) > 0, (len(a), len(b))
    spss = []
    for x, y in zip(a, b):
        if is_sps(y):
            assert is_sps(x)
            fx, fy = parse_sps(x), parse_sps(y)
            assert fy["vui"] is None and fy["vui_parameters_present_flag"] == 0
            vui = vui_fields(matrix, full, fps)
            assert fx["vui"] == vui, (fx["vui"], vui)
            assert fx["vui_parameters_present_flag"] == int(vui is not None)
            assert {k: v for k, v in fx.items() if not k.startswith("vui")} == {k: v for k, v in fy.items() if not k.startswith("vui")}
            if vui is None:
                assert x == y
            spss.append(x)
        else:
            assert x == y, "a NAL that is not an SPS differs"
    assert spss
    return spss
