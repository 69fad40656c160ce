"""tests/save_ref.py -- the numpy restatement of the save tail the GPU tests compare against -- held to what the
reference itself states: its unit tests' numbers (tests/golden/save_kat.json, with citations), the oracle's integer
conversions, and f16::from_f32's own properties."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import save_ref as sr
from oracle.oracle import Oracle

KAT = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "save_kat.json")))
FMT = {"u8": sr.U8, "u16": sr.U16, "f16": sr.F16, "f32": sr.F32}


@pytest.fixture(scope="module")
def oracle():
    return Oracle(fused=True)


def test_premultiply_basic():
    k = KAT["premultiply_basic"]
    got = sr.premultiply([np.float32(c) for c in k["rgb"]], np.float32(k["alpha"]))
    for g, e in zip(got, k["expected"]):
        assert np.all(np.abs(g - np.float32(e)) <= k["tolerance"])


def test_spot_srgb_primaries():
    k = KAT["srgb_primaries"]
    got = sr.spot_color([np.float32(c) for c in k["rgb"]], np.float32(k["spot"]), k["spot_color"])
    for g, e in zip(got, k["expected"]):
        assert np.all(np.abs(g - np.float32(e)) <= k["tolerance"])


def test_spot_is_two_products_and_a_sum():
    # a value where a fused multiply-add would round differently from the scalar loop of spot.rs
    rng = np.random.default_rng(5)
    c = rng.uniform(-0.5, 1.5, 4096).astype(np.float32)
    s = rng.uniform(0, 1, 4096).astype(np.float32)
    got = sr.spot_color([c, c, c], s, (0.3, 0.6, 0.9, 0.7))[0]
    mix = np.float32(0.7) * s
    a = np.float32(mix * np.float32(0.3))
    b = np.float32(np.float32(np.float32(1) - mix) * c)
    assert np.array_equal(got, np.float32(a + b))
    fused = (a.astype(np.float64) + (np.float32(1) - mix).astype(np.float64) * c.astype(np.float64)).astype(np.float32)
    assert np.any(fused != got), "the sample set does not tell a fused evaluation apart"


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientation_maps(orientation):
    k = KAT["orientation_maps"]
    w, h = k["size"]
    src = np.arange(w * h, dtype=np.uint32).reshape(h, w, 1)
    dst = sr.orient(src, orientation)
    ow, oh = sr.oriented_size(orientation, w, h)
    assert dst.shape == (oh, ow, 1)
    want = np.array(k["source_index_of_dest"][str(orientation)], dtype=np.uint32).reshape(oh, ow)
    assert np.array_equal(dst[:, :, 0], want)  # src holds each pixel's raster index


def test_float16_reference_cases():
    for c in KAT["float16"]["cases"]:
        v = np.float32(float(c["f32"]))
        assert int(sr.f32_to_f16_bits(np.array([v]))[0]) == c["bits"], c


def test_float16_all_halves_round_trip():
    """Every half widened exactly to f32 and converted back.  Zeros, normal halves and infinities come back as they
    are; a NaN comes back as sign | 0x7E00.  A DENORMAL half h comes back as h >> 1: from_f32 as written shifts
    (mant | 0x800000) by shift + 14 = -unbiased, one more than the 2^-24 unit of f16 denormals asks for
    (2^-24 itself: 0x800000 >> 24 = 0), and it is the reference's bits the device has to give, so this pins them."""
    h = np.arange(65536, dtype=np.uint16)
    back = sr.f32_to_f16_bits(sr.f16_bits_to_f32(h))
    exp, mant = (h >> 10) & 0x1F, h & 0x3FF
    nan = (exp == 31) & (mant != 0)
    den = (exp == 0) & (mant != 0)
    same = ~nan & ~den
    assert same.sum() == 65536 - 2 * 1023 - 2 * 1023
    assert np.array_equal(back[same], h[same])
    assert np.array_equal(back[nan], (h[nan] & 0x8000) | 0x7E00)  # one payload for every NaN, the sign kept
    assert np.array_equal(back[den], (h[den] & 0x8000) | (mant[den] >> 1))
    assert np.array_equal(back, np.array([f16_scalar(v) for v in sr.f16_bits_to_f32(h)], dtype=np.uint16))


def f16_boundary_values():
    """f32 inputs around every rounding decision of f16::from_f32"""
    bits = []
    h = np.arange(0x0001, 0x7C00, dtype=np.uint32)  # every positive finite half: itself, its upper tie and the neighbours
    for hv in (h[:8], h[0x3F8:0x408], h[0x7BF8 - 1:0x7BFF], h[::257]):
        f = sr.f16_bits_to_f32(hv.astype(np.uint16)).view(np.uint32).astype(np.int64)
        nxt = sr.f16_bits_to_f32((hv + 1).astype(np.uint16)).astype(np.float64)
        tie = ((sr.f16_bits_to_f32(hv.astype(np.uint16)).astype(np.float64) + nxt) / 2).astype(np.float32).view(np.uint32)
        tie = tie.astype(np.int64)
        for d in (-1, 0, 1):
            bits += list(f + d) + list(tie + d)
    # 65504 (the last normal), the tie to infinity at 65520, its neighbours, 2^-24 / 2^-25 and theirs, f32 denormals
    for v in (65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 2.0 ** -15, 1e-10,
              5.96e-8, 5.97e-8, 8.9e-8, 1.19e-7, 6.1e-5, 6.09e-5):
        b = int(np.float32(v).view(np.uint32))
        bits += [b - 1, b, b + 1]
    bits += [0, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF]
    b = np.array(bits, dtype=np.int64) & 0x7FFFFFFF
    b = np.concatenate([b, b | 0x80000000]).astype(np.uint32)
    return b.view(np.float32)


def f16_scalar(v):
    """f16::from_f32 transcribed for one value with Python integers: the check of the vectorised form"""
    bits = int(np.float32(v).view(np.uint32))
    sign, exp, mant = bits >> 31, (bits >> 23) & 0xFF, bits & 0x7FFFFF
    if exp == 0:
        return sign << 15
    if exp == 255:
        return (sign << 15) | 0x7C00 | (0x200 if mant else 0)
    u = exp - 127
    if u < -24:
        return sign << 15
    if u < -14:
        return (sign << 15) | ((mant | 0x800000) >> ((-14 - u) + 14))
    if u > 15:
        return (sign << 15) | 0x7C00
    he, hm = u + 15, mant >> 13
    if (mant >> 12) & 1 and ((mant & 0xFFF) or (hm & 1)):
        hm += 1
    if hm > 0x3FF:
        return (sign << 15) | (0x7C00 if he >= 30 else (he + 1) << 10)
    return (sign << 15) | (he << 10) | hm


def test_float16_rounding_boundaries():
    v = f16_boundary_values()
    got = sr.f32_to_f16_bits(v)
    want = np.array([f16_scalar(x) for x in v], dtype=np.uint16)
    assert np.array_equal(got, want)
    # in the normal range the conversion is IEEE round-to-nearest-even; into denormals it truncates, so it can differ
    with np.errstate(over="ignore"):
        ieee = v.astype(np.float16).view(np.uint16)
    a = np.abs(v)
    normal = (a >= np.float32(2.0 ** -14)) & np.isfinite(v)
    assert np.array_equal(got[normal], ieee[normal])
    den = (a < np.float32(2.0 ** -14)) & (a >= np.float32(2.0 ** -24))
    assert np.any(got[den] != ieee[den]) and np.all(got[den] <= ieee[den])


def test_opaque_alpha_bytes():
    for c in KAT["opaque_alpha_bytes"]["cases"]:
        assert list(sr.opaque_alpha_bytes(FMT[c["format"]], c["bit_depth"], c["big_endian"])) == c["bytes"], c


def edge_samples(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-0.5, 1.5, n).astype(np.float32)
    edges = np.float32([0.0, -0.0, 1.0, 0.5, 1.0 / 255, 0.5 / 255, 1.5 / 255, 254.5 / 255, np.nan, np.inf, -np.inf, 1e-30,
                        -1e-30, 2.5 / 31, 0.5 / 65535, 1.5 / 65535, 2.5 / 1023, 1.0000001, 0.99999994])
    v[:edges.size] = edges
    return v


@pytest.mark.parametrize("depth", [1, 5, 8])
def test_u8_equals_the_oracle(oracle, depth):
    v = edge_samples(3000, depth)
    rng = np.random.default_rng(100 + depth)
    x = rng.integers(0, 5000, v.size)
    y = rng.integers(0, 5000, v.size)
    for ch in range(6):
        got = sr.f32_to_u8(v, x, y, ch, depth)
        want = [oracle.f32_to_u8(float(v[i]), int(x[i]), int(y[i]), ch, depth) for i in range(v.size)]
        assert np.array_equal(got, np.array(want, dtype=np.uint8)), (ch, depth)


@pytest.mark.parametrize("depth", [1, 10, 12, 16])
def test_u16_equals_the_oracle(oracle, depth):
    v = edge_samples(3000, 40 + depth)
    got = sr.f32_to_u16(v, depth)
    want = [int(oracle.lib.jxlo_f32_to_u16(C.c_float(float(x)), depth)) for x in v]
    assert np.array_equal(got, np.array(want, dtype=np.uint16))


def test_rust_clamp_keeps_nan_and_negative_zero():
    v = np.float32([np.nan, -0.0, -1.0, 2.0, 0.25])
    got = sr.rust_clamp(v, 0.0, 1.0)
    assert np.isnan(got[0]) and np.signbit(got[1]) and got[1] == 0
    assert list(got[2:]) == [0.0, 1.0, 0.25]


def test_save_assembles_channels_fill_and_byte_order(oracle):
    rng = np.random.default_rng(9)
    planes = [rng.uniform(-0.5, 1.5, (5, 7)).astype(np.float32) for _ in range(5)]
    d = sr.desc([2, 1, 0], sr.U16, 10, fill_opaque_alpha=True, big_endian=True, orientation=6)
    out = sr.save(oracle, d, planes)
    assert out.shape == (7, 5 * 4) and out.dtype == np.uint16
    raw = out.view(np.uint8).reshape(7, 5, 4, 2)
    val = raw[..., 0].astype(np.uint16) << 8 | raw[..., 1]  # big endian in memory
    for y in range(5):
        for x in range(7):
            dx, dy = sr.display_pixel(6, x, y, 7, 5)
            assert list(val[dy, dx, :3]) == [int(sr.f32_to_u16(planes[c][y, x], 10)) for c in (2, 1, 0)]
            assert val[dy, dx, 3] == 1023
