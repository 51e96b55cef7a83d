"""CPU: the egress model (tests/egress_model.py) is the stated definition and has the properties it promises -- exhaustively over all 2^24
(Y, U, V) triples per table row."""
import numpy as np
import pytest

import color_model
import egress_model as EM


@pytest.mark.parametrize("key", sorted(EM.ROWS))
def test_row_fits_the_24_bit_multiply_over_all_inputs(key):
    """all 2^24 triples: every operand inside 24 signed bits, every product and sum inside 32; grey stays grey, black and white are 0 and 255"""
    EM.check_row(key)


@pytest.mark.parametrize("key", sorted(EM.ROWS))
def test_row_is_its_recipe(key):
    """Kr / Kb -> 2(1 - Kr), 2(1 - Kb), -2 Kb (1 - Kb)/Kg, -2 Kr (1 - Kr)/Kg, scaled by 255/224 (luma 255/219) for limited range, times 256, rounded"""
    assert EM.derived_row(*key) == EM.ROWS[key]
    assert sorted(EM.ROWS) == sorted(color_model.ROWS)


def test_grey_black_and_white():
    for key, (ky, yo, rv, gu, gv, bu) in EM.ROWS.items():
        black, white = (0, 255) if key[1] else (16, 235)
        assert white == yo + (255 if key[1] else 219)
        for y in range(256):
            want = min(max((ky * (y - yo) + 128) >> 8, 0), 255)
            assert [int(c) for c in EM.yuv_to_rgb(y, 128, 128, key)] == [want] * 3
        assert [int(c) for c in EM.yuv_to_rgb(black, 128, 128, key)] == [0, 0, 0]
        assert [int(c) for c in EM.yuv_to_rgb(white, 128, 128, key)] == [255, 255, 255]
    # the names and the default
    assert EM.row() == EM.row((0, 0)) == EM.row("bt601") == EM.ROWS[(6, 0)]
    assert EM.row("bt709-full") == EM.ROWS[(1, 1)]


def test_model_is_the_stated_definition():
    """a 6 x 4 picture inside a 16 x 16 coded one, pixel by pixel in plain Python integers, for every row: replicated chroma, arithmetic
    shifts, the clamp (random coded samples leave 0..255 often), the crop, and the four layouts"""
    W, H, w, h = 16, 16, 6, 4
    packed = np.random.default_rng(11).integers(0, 256, W * H * 3 // 2, dtype=np.uint8)
    p = packed.astype(int).tolist()
    Y = lambda i, j: p[j * W + i]
    U = lambda i, j: p[W * H + (j // 2) * (W // 2) + i // 2]
    V = lambda i, j: p[W * H * 5 // 4 + (j // 2) * (W // 2) + i // 2]
    clamp = lambda x: 0 if x < 0 else 255 if x > 255 else x
    clamped = 0
    for key, (ky, yo, rv, gu, gv, bu) in EM.ROWS.items():
        want = []
        for j in range(h):
            for i in range(w):
                c, d, e = Y(i, j) - yo, U(i, j) - 128, V(i, j) - 128
                raw = [(ky * c + rv * e + 128) >> 8, (ky * c + gu * d + gv * e + 128) >> 8, (ky * c + bu * d + 128) >> 8]
                clamped += sum(x != clamp(x) for x in raw)
                want.append([clamp(x) for x in raw])
        rgb = EM.recon_to("rgb", packed, W, H, w, h, key)
        assert rgb.shape == (h, w, 3) and rgb.reshape(-1, 3).tolist() == want
        rgba = EM.recon_to("rgb", packed, W, H, w, h, key, 4)
        assert rgba.shape == (h, w, 4) and np.array_equal(rgba[:, :, :3], rgb) and (rgba[:, :, 3] == 255).all()
        assert np.array_equal(EM.recon_to("rgbp", packed, W, H, w, h, key), rgb.transpose(2, 0, 1))
    assert clamped > 0
    i420 = EM.recon_to("i420", packed, W, H, w, h)
    assert i420.tolist() == [Y(i, j) for j in range(h) for i in range(w)] + [U(i, j) for j in range(0, h, 2) for i in range(0, w, 2)] + \
        [V(i, j) for j in range(0, h, 2) for i in range(0, w, 2)]
    y, uv = EM.recon_to("nv12", packed, W, H, w, h)
    assert y.shape == (h, w) and uv.shape == (h // 2, w)
    assert np.array_equal(y.reshape(-1), i420[: w * h])
    assert np.array_equal(uv[:, 0::2].reshape(-1), i420[w * h: w * h * 5 // 4]) and np.array_equal(uv[:, 1::2].reshape(-1), i420[w * h * 5 // 4:])
    # nothing to crop: the whole coded picture
    assert np.array_equal(EM.recon_to("i420", packed, W, H, W, H), packed)
