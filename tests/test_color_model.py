"""CPU: the colour model (tests/color_model.py) is the stated definition and has the properties it promises -- exhaustively over all 2^24
RGB triples per table row -- and its bitstream helpers read what they should."""
import numpy as np
import pytest

import color_model as CM
import ingest_model
import rgbp_model


@pytest.mark.parametrize("matrix,full", sorted(CM.ROWS))
def test_row_keeps_its_range_over_all_inputs(matrix, full):
    """all 2^24 triples, before any uint8 cast: Y 16..235 and U, V 16..240, or 0..255 all three; grey, black and white"""
    CM.check_row(matrix, full)


@pytest.mark.parametrize("matrix,full", sorted(CM.ROWS))
def test_row_is_its_recipe_with_one_coefficient_moved(matrix, full):
    """every coefficient within 1 of the rounded recipe; at most one moved per row -- except full-range chroma, where the 0.5 weight
    is 127 instead of the rounded 128 (which overflows a byte) and one neighbour takes the 1 back: exactly those two"""
    (y, yo, u, v) = CM.row(matrix, full)
    assert sum(y) == (256 if full else 220) and sum(u) == 0 and sum(v) == 0 and yo == (0 if full else 16)
    for k, (have, made) in enumerate(zip((y, u, v), CM.derived_row(matrix, full))):
        diff = [a - b for a, b in zip(have, made)]
        assert max(abs(d) for d in diff) <= 1, (have, made)
        if full and k:
            assert max(made) == 128 and max(have) == 127 and sorted(diff) == [-1, 0, 1], (have, made)
        else:
            assert sorted(abs(d) for d in diff)[:2] == [0, 0], (have, made)


def test_default_row_is_the_existing_model():
    w, h = 64, 48
    hwc = ingest_model.rgb_clip(w, h, 2, 4)
    chw = rgbp_model.noisy_clip(128, 96, 1)[0]
    for t in range(2):
        for m in (0, 6):
            assert np.array_equal(CM.rgb_to_i420(hwc[t], m, 0), ingest_model.rgb_to_i420(hwc[t]))
    assert np.array_equal(CM.scale_to_i420(chw, w, h, (14, 6, 100, 80)), rgbp_model.scale_to_i420(chw, w, h, (14, 6, 100, 80)))
    assert np.array_equal(CM.to_i420(chw), rgbp_model.to_i420(chw))


def test_model_is_the_stated_definition():
    """pixel by pixel in plain Python integers, for every row"""
    w, h = 6, 4
    chw = rgbp_model.noisy_clip(w, h, 1)[0].astype(int).tolist()
    for (matrix, full), (yc, yo, uc, vc) in CM.ROWS.items():
        want = [((yc[0] * chw[0][j][i] + yc[1] * chw[1][j][i] + yc[2] * chw[2][j][i] + 128) >> 8) + yo for j in range(h) for i in range(w)]
        for mat in (uc, vc):
            for j in range(0, h, 2):
                for i in range(0, w, 2):
                    m = [(chw[c][j][i] + chw[c][j][i + 1] + chw[c][j + 1][i] + chw[c][j + 1][i + 1] + 2) >> 2 for c in range(3)]
                    want.append(((mat[0] * m[0] + mat[1] * m[1] + mat[2] * m[2] + 128) >> 8) + 128)
        assert list(CM.to_i420(np.array(chw, np.uint8), matrix, full)) == want


def test_corner_colours_and_constants():
    f = CM.corner_frame(16, 2)
    assert {tuple(f[:, 0, x]) for x in range(16)} == {(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)}
    for (matrix, full) in CM.ROWS:
        ylo, yhi, _, _ = CM.ranges(full)
        out = CM.to_i420(f, matrix, full)
        assert out[0] == ylo and out[14] == yhi and out[32] == 128 and out[32 + 7] == 128 and out[40] == 128
        # a constant colour stays that colour through any ratio
        const = np.empty((3, 96, 128), np.uint8)
        for c, val in enumerate((17, 200, 99)):
            const[c] = val
        y, u, v = (int(x) for x in CM.to_i420(const[:, :2, :2], matrix, full)[[0, 4, 5]])
        out = CM.scale_to_i420(const, 36, 20, (0, 0, 100, 52), matrix, full)
        assert (out[:720] == y).all() and (out[720:900] == u).all() and (out[900:] == v).all()


def test_bitstream_helpers():
    assert CM.unescape(bytes([0x67, 0, 0, 3, 0, 0, 3, 1, 0, 0, 3, 3, 5])) == bytes([0x67, 0, 0, 0, 0, 1, 0, 0, 3, 5])
    s = b"\x00\x00\x00\x01\x67\x42\x00\x00\x00\x01\x65\x88\x80"
    assert CM.split_annexb(s) == [b"\x67\x42", b"\x65\x88\x80"]
    # an SPS written bit by bit: 64x48, no cropping, VUI with bt709 full range and 30000/1001
    bits = "01100111" + format(66, "08b") + "00000000" + format(10, "08b") + "1" + "010" + "011" + "010" + "0" + "00100" + "011" + "1" + "1" + "0" + "1"
    bits += "0" + "0" + "1" + "101" + "1" + "1" + format(1, "08b") * 3 + "0" + "1" + format(1001, "032b") + format(60000, "032b") + "1" + "0" + "0" + "0" + "0" + "1"
    bits += "0" * (-len(bits) % 8)
    raw = bytes(int(bits[i: i + 8], 2) for i in range(0, len(bits), 8))
    esc, zeros = bytearray(), 0
    for b in raw:
        if zeros == 2 and b <= 3:
            esc.append(3)
            zeros = 0
        esc.append(b)
        zeros = zeros + 1 if b == 0 else 0
    f = CM.parse_sps(bytes(esc))
    assert (f["pic_width_in_mbs_minus1"], f["pic_height_in_map_units_minus1"], f["level_idc"], f["num_ref_frames"]) == (3, 2, 10, 1)
    assert f["vui"] == CM.vui_fields(1, 1, (30000, 1001))
    assert CM.vui_fields() is None and CM.vui_fields(0, 0, (25, 1))["video_signal_type_present_flag"] == 0
