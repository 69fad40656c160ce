"""numpy float32 restatement of the reference's save tail (Frame::build_render_pipeline, jxl/src/frame/render.rs:793-903):
SpotColorStage (render/stages/spot.rs:40-67), PremultiplyAlphaStage (premultiply_alpha.rs:47-92), ConvertF32ToU8Stage /
ConvertF32ToU16Stage / ConvertF32ToF16Stage (convert.rs:570-606, :743-761, :841-860) and the save stage with its channel
order, endianness, opaque-alpha fill and orientation (render/save.rs:20-50, simple_pipeline/save.rs:14-89,
headers/image_metadata.rs:85-96).

Colour comes from the oracle (xyb_to_linear, from_linear, ycbcr_to_rgb); everything else is numpy in explicit f32 steps.
np.rint rounds to nearest even, as the oracle's fused build and the device do.  f16 is the integer algorithm of
jxl/src/util/float16.rs:82-141 on uint32 views -- it truncates into f16 denormals and gives every NaN one payload, which
astype(np.float16) does not.  Orientation is index arithmetic.

A save is a plain dict (`desc(...)`) with the fields of jxlh_save_desc; samples come back as uint8 / uint16 / uint16
(f16 bits) / uint32 (f32 bits) arrays in the byte order asked for, viewed natively."""
import os
import re
import sys

import numpy as np

U8, U16, F16, F32 = range(4)
SAMPLE_DTYPE = {U8: np.uint8, U16: np.uint16, F16: np.uint16, F32: np.uint32}
F16_CLAMP_PQ = (0.0, 1.0)           # frame/render.rs:746-750
F16_CLAMP_HLG = (-0.074, 1.1)

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dither = None


def dither_table():
    """the 32 x 32 table of ConvertF32ToU8Stage, as the oracle carries it"""
    global _dither
    if _dither is None:
        txt = open(os.path.join(_ROOT, "oracle", "dither_table.inc")).read()
        txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
        vals = [float(v.rstrip("fF")) for v in re.findall(r"[-+]?\d*\.\d+(?:[eE][-+]?\d+)?[fF]?|[-+]?\d+\.[fF]?", txt)]
        assert len(vals) == 1024, len(vals)
        _dither = np.array(vals, dtype=np.float64).astype(np.float32).reshape(32, 32)
    return _dither


def desc(channels, format=U8, bit_depth=None, fill_opaque_alpha=False, big_endian=False, orientation=1, f16_clamp=None,
         premultiply=None, spot=()):
    """channels: pipeline channels in output order (0..2 colour, 3 + ec extra channel); f16_clamp: (min, max) or None;
    premultiply: the alpha's pipeline channel or None; spot: [(ec, (r, g, b, scale)), ...]"""
    if bit_depth is None:
        bit_depth = {U8: 8, U16: 16}.get(format, 0)
    return dict(channels=list(channels), format=format, bit_depth=bit_depth, fill_opaque_alpha=bool(fill_opaque_alpha),
                big_endian=bool(big_endian), orientation=orientation, f16_clamp=f16_clamp, premultiply=premultiply,
                spot=list(spot))


# ---- stage 1: the colour stage, from the oracle
def colour_stage(oracle, planes, colour):
    """colour: None / ("none",), ("ycbcr",) or ("xyb", transfer, xyb_params, tf_param, lum) -> three f32 planes"""
    p = [np.ascontiguousarray(a, dtype=np.float32) for a in planes[:3]]
    if colour is None or colour[0] == "none":
        return [a.copy() for a in p]
    shape = p[0].shape
    if colour[0] == "ycbcr":
        return [np.asarray(a, dtype=np.float32).reshape(shape) for a in oracle.ycbcr_to_rgb(*p)]
    _, transfer, params, tf_param, lum = colour
    rgb = oracle.xyb_to_linear(params, *p)
    if transfer != "linear":
        rgb = oracle.from_linear(transfer, rgb, tf_param, lum)
    return [np.asarray(a, dtype=np.float32).reshape(shape) for a in rgb]


# ---- stage 2 / 3
def spot_color(rgb, s, rgba):
    """spot.rs:61-66: two products and one sum, each rounded to f32"""
    rgba = np.float32(rgba)
    with np.errstate(invalid="ignore", over="ignore"):
        mix = np.float32(rgba[3]) * s.astype(np.float32)
        out = []
        for k in range(3):
            a = (mix * rgba[k]).astype(np.float32)
            b = ((np.float32(1.0) - mix).astype(np.float32) * rgb[k]).astype(np.float32)
            out.append((a + b).astype(np.float32))
    return out


def premultiply(rgb, alpha):
    with np.errstate(invalid="ignore", over="ignore"):
        return [(c.astype(np.float32) * alpha.astype(np.float32)).astype(np.float32) for c in rgb]


# ---- stage 4: conversions
def f32_to_u8(v, x, y, ch, bit_depth=8):
    """f32_to_u8_simd: v, x, y broadcastable arrays; ch the PIPELINE channel"""
    maxv = np.float32((1 << bit_depth) - 1)
    d = dither_table()[(np.asarray(y) + 13 * ch) % 32, (np.asarray(x) + 23 * ch) % 32]
    with np.errstate(invalid="ignore", over="ignore"):
        dithered = ((np.asarray(v, np.float32) * maxv).astype(np.float32) + d).astype(np.float32)
        clamped = np.where(dithered > 0, dithered, np.float32(0))   # NaN -> 0
        clamped = np.where(clamped < maxv, clamped, maxv)
    return np.rint(clamped).astype(np.uint8)


def f32_to_u16(v, bit_depth=16):
    maxv = np.float32((1 << bit_depth) - 1)
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        clamped = np.where(v > 0, v, np.float32(0))
        clamped = np.where(clamped < 1, clamped, np.float32(1))
    return np.rint((clamped * maxv).astype(np.float32)).astype(np.uint16)


def rust_clamp(v, lo, hi):
    """f32::clamp: a NaN stays a NaN, -0.0 is not below 0.0 and stays"""
    v = np.array(v, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        v[v < np.float32(lo)] = np.float32(lo)
        v[v > np.float32(hi)] = np.float32(hi)
    return v


def f32_to_f16_bits(v):
    """f16::from_f32 (util/float16.rs:82-141) as written, on uint32 views"""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign = (bits >> 31) & 1
    exp = (bits >> 23) & 0xFF
    mant = bits & 0x007FFFFF
    unbiased = exp - 127
    out = np.zeros(bits.shape, dtype=np.int64)
    # normal f16: round to nearest even, with mantissa carry
    h_exp = unbiased + 15
    h_mant = mant >> 13
    round_bit = (mant >> 12) & 1
    sticky = mant & 0x0FFF
    h_mant = np.where((round_bit == 1) & ((sticky != 0) | ((h_mant & 1) == 1)), h_mant + 1, h_mant)
    normal = np.where(h_mant > 0x3FF, np.where(h_exp >= 30, 0x1F << 10, (h_exp + 1) << 10), (h_exp << 10) | h_mant)
    # f16 denormal: truncation
    shift = np.clip(-14 - unbiased, 0, 40)
    denorm = (mant | 0x00800000) >> (shift + 14)
    out = np.where(unbiased > 15, 0x1F << 10, normal)
    out = np.where(unbiased < -14, denorm, out)
    out = np.where(unbiased < -24, 0, out)
    out = np.where(exp == 255, np.where(mant == 0, 0x1F << 10, (0x1F << 10) | 0x0200), out)
    out = np.where(exp == 0, 0, out)
    return ((sign << 15) | out).astype(np.uint16)


def f16_bits_to_f32(h):
    """exact widening of every f16 (numpy's conversion in this direction is exact)"""
    return np.asarray(h, dtype=np.uint16).view(np.float16).astype(np.float32)


def opaque_alpha(fmt, bit_depth):
    """api/data_types.rs:114-149, as a native sample"""
    if fmt in (U8, U16):
        return (1 << bit_depth) - 1
    return 0x3C00 if fmt == F16 else 0x3F800000


def opaque_alpha_bytes(fmt, bit_depth, big_endian):
    n = SAMPLE_DTYPE[fmt]().itemsize
    return int(opaque_alpha(fmt, bit_depth)).to_bytes(n, "big" if big_endian else "little")


def convert(v, fmt, bit_depth, ch, x, y, f16_clamp=None):
    if fmt == U8:
        return f32_to_u8(v, x, y, ch, bit_depth)
    if fmt == U16:
        return f32_to_u16(v, bit_depth)
    if fmt == F16:
        if f16_clamp is not None:
            v = rust_clamp(v, *f16_clamp)
        return f32_to_f16_bits(v)
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()


# ---- stage 6: position
def display_pixel(orientation, x, y, w, h):
    """Orientation::display_pixel (headers/image_metadata.rs:85-96)"""
    return {1: (x, y), 2: (w - 1 - x, y), 3: (w - 1 - x, h - 1 - y), 4: (x, h - 1 - y), 5: (y, x), 6: (h - 1 - y, x),
            7: (h - 1 - y, w - 1 - x), 8: (y, w - 1 - x)}[orientation]


def oriented_size(orientation, w, h):
    return (h, w) if orientation >= 5 else (w, h)


def save_samples(oracle, d, planes, colour=None, origin=(0, 0)):
    """stages 1-5 on whole planes -> [h, w, samples per pixel] native samples of the UNORIENTED image (before byte order)"""
    planes = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
    h, w = planes[0].shape
    fmt, depth = d["format"], d["bit_depth"]
    colour_named = any(c < 3 for c in d["channels"])
    rgb = None
    if colour_named:
        rgb = colour_stage(oracle, planes, colour)
        for ec, rgba in d["spot"]:
            rgb = spot_color(rgb, planes[3 + ec], rgba)
        if d["premultiply"] is not None:
            rgb = premultiply(rgb, planes[d["premultiply"]])
    x = np.arange(w)[None, :] + origin[0]
    y = np.arange(h)[:, None] + origin[1]
    spp = len(d["channels"]) + (1 if d["fill_opaque_alpha"] else 0)
    out = np.zeros((h, w, spp), dtype=SAMPLE_DTYPE[fmt])
    for k, ch in enumerate(d["channels"]):
        v = rgb[ch] if ch < 3 else planes[ch]
        out[:, :, k] = convert(v, fmt, depth, ch, x, y, d["f16_clamp"])
    if d["fill_opaque_alpha"]:
        out[:, :, spp - 1] = opaque_alpha(fmt, depth)
    return out


def orient(samples, orientation):
    """[h, w, spp] -> the oriented image [oh, ow, spp], by index arithmetic"""
    h, w, spp = samples.shape
    ow, oh = oriented_size(orientation, w, h)
    out = np.zeros((oh, ow, spp), dtype=samples.dtype)
    ys, xs = np.mgrid[0:h, 0:w]
    dx, dy = display_pixel(orientation, xs, ys, w, h)
    out[dy, dx] = samples[ys, xs]
    return out


def byte_order(samples, big_endian):
    """native samples -> the array whose MEMORY holds them in the byte order asked for"""
    if samples.dtype.itemsize == 1:
        return samples
    native_big = sys.byteorder == "big"
    return samples.byteswap() if bool(big_endian) != native_big else samples


def save(oracle, d, planes, colour=None, origin=(0, 0)):
    """the whole save: [oh, ow * spp] samples as they lie in memory"""
    s = orient(save_samples(oracle, d, planes, colour, origin), d["orientation"])
    s = byte_order(s, d["big_endian"])
    return s.reshape(s.shape[0], -1)
