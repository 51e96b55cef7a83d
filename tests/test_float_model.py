"""CPU: the float sample model (tests/float_model.py) against exact rational arithmetic -- fractions.Fraction, every rounding to nearest
with ties to even, written out here without a floating-point operation:

  - the quantiser over all 65536 float16 and all 65536 bfloat16 bit patterns and the float32 edge set (every k/255, the neighbours of
    every rounding boundary, zeros, infinities, NaNs, denormals, 1 +- ulp, 2^16 random patterns);
  - the 256-entry tables of the way out for the three types;
  - and what the model promises in words: it is the torch expression of the issue, and v * (1 / 255.f) would NOT be the way out."""
from fractions import Fraction

import numpy as np
import pytest

import float_model as FM

# (exponent bits, mantissa bits) of the three types
LAYOUT = {"f16": (5, 10), "bf16": (8, 7), "f32": (8, 23)}


def decode(bits, kind):
    """the exact value of a bit pattern: a Fraction, or "nan" / "+inf" / "-inf" """
    eb, mb = LAYOUT[kind]
    bits = int(bits)
    sign, e, m = bits >> (eb + mb), (bits >> mb) & ((1 << eb) - 1), bits & ((1 << mb) - 1)
    bias = (1 << (eb - 1)) - 1
    if e == (1 << eb) - 1:
        return "nan" if m else ("-inf" if sign else "+inf")
    v = Fraction(m, 1 << mb) * Fraction(2) ** (1 - bias) if e == 0 else (1 + Fraction(m, 1 << mb)) * Fraction(2) ** (e - bias)
    return -v if sign else v


def round_to(v, kind):
    """the nearest value of type `kind` to the Fraction v >= 0, ties to even, as (a Fraction or "+inf")"""
    eb, mb = LAYOUT[kind]
    bias = (1 << (eb - 1)) - 1
    if v == 0:
        return v
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    ulp = Fraction(2) ** (max(e, 1 - bias) - mb)
    r = round(v / ulp) * ulp                    # round() of a Fraction: to nearest, ties to even
    return "+inf" if r >= Fraction(2) ** (bias + 1) else r


def encode_exact(v, kind):
    """the bit pattern of a Fraction v >= 0 that the type holds exactly"""
    eb, mb = LAYOUT[kind]
    bias = (1 << (eb - 1)) - 1
    if v == 0:
        return 0
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    if e < 1 - bias:
        m = v / Fraction(2) ** (1 - bias - mb)
        assert m.denominator == 1
        return int(m)
    m = (v / Fraction(2) ** e - 1) * (1 << mb)
    assert m.denominator == 1
    return ((e + bias) << mb) | int(m)


def quantise_exact(bits, kind):
    v = decode(bits, kind)
    if v == "nan" or v == "-inf":
        return 0
    if v == "+inf":
        return 255
    if v <= 0:
        return 0
    p = round_to(v * 255, "f32")                # the ONE float32 multiply
    if p == "+inf":
        return 255
    return min(int(round(p)), 255)              # rint: ties to even


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_quantiser_all_16_bit_patterns(kind):
    bits = np.arange(65536, dtype=np.uint16)
    got = FM.quantise(bits, kind)
    want = np.array([quantise_exact(b, kind) for b in bits], np.uint8)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s pattern 0x%04x: model %d, exact %d" % (kind, bad[0], got[bad[0]], want[bad[0]])
    assert set(got.tolist()) == set(range(256)) if kind == "f16" else got.max() == 255 and got.min() == 0


def test_quantiser_f32_edge_set():
    bits = FM.f32_edge_bits()
    assert bits.size > 65536 + 256 * 8
    got = FM.quantise(bits, "f32")
    want = np.array([quantise_exact(b, "f32") for b in bits], np.uint8)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "f32 pattern 0x%08x: model %d, exact %d" % (bits[bad[0]], got[bad[0]], want[bad[0]])
    # the set holds what it promises: every level exactly, both sides of every boundary, and the special values
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).view(np.uint32)
    assert np.array_equal(FM.quantise(k, "f32"), np.arange(256, dtype=np.uint8)) and np.isin(k, bits).all()
    for b, q in ((0x80000000, 0), (0x7F800000, 255), (0xFF800000, 0), (0x7FC00000, 0), (0xFFC00000, 0), (0x00000001, 0), (0x007FFFFF, 0),
                 (0x3F800001, 255), (0x3F7FFFFF, 255), (0xBF800000, 0), (0x7F7FFFFF, 255)):
        assert b in bits and FM.quantise(np.array([b], np.uint32), "f32")[0] == q, hex(b)
    mid = ((np.arange(0, 255, dtype=np.float64) + 0.5) / 255).astype(np.float32).view(np.uint32)
    lo, hi = FM.quantise(mid - 3, "f32"), FM.quantise(mid + 3, "f32")
    assert np.array_equal(lo, np.arange(0, 255)) and np.array_equal(hi, np.arange(1, 256))


@pytest.mark.parametrize("kind", FM.KINDS)
def test_output_tables(kind):
    got = FM.table(kind)
    assert got.shape == (256,) and got.dtype == FM.BITS[kind]
    for v in range(256):
        f = round_to(Fraction(v, 255), "f32")                                   # the ONE float32 division
        want = encode_exact(f if kind == "f32" else round_to(f, kind), kind)    # ... narrowed
        assert int(got[v]) == want, "%s table[%d]: model 0x%x, exact 0x%x" % (kind, v, got[v], want)
    # what goes out comes back in as itself
    assert np.array_equal(FM.quantise(got, kind), np.arange(256, dtype=np.uint8))


def test_reciprocal_multiply_is_not_the_way_out():
    v = np.arange(256, dtype=np.float32)
    wrong = (v * (np.float32(1) / np.float32(255))).view(np.uint32)
    assert (wrong != FM.table("f32")).any()


def test_model_is_the_torch_expression():
    torch = pytest.importorskip("torch")
    bits = FM.f32_edge_bits()
    x = torch.from_numpy(bits.view(np.float32).copy())
    want = torch.nan_to_num((x.float() * 255).round().clamp(0, 255), nan=0).to(torch.uint8).numpy()
    assert np.array_equal(FM.quantise(bits, "f32"), want)
    h = np.arange(65536, dtype=np.uint16)
    for kind, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        x = torch.from_numpy(h.view(np.int16).copy()).view(dtype)
        want = torch.nan_to_num((x.float() * 255).round().clamp(0, 255), nan=0).to(torch.uint8).numpy()
        assert np.array_equal(FM.quantise(h, kind), want), kind
    u8 = torch.arange(256, dtype=torch.uint8)
    for kind, dtype, view in (("f16", torch.float16, torch.int16), ("bf16", torch.bfloat16, torch.int16), ("f32", torch.float32, torch.int32)):
        want = (u8.float() / 255).to(dtype).view(view).numpy()
        assert np.array_equal(FM.table(kind).view(want.dtype), want), kind
