"""The expected full-size preview of an LF frame (Frame::render_lf_frame_rect / maybe_preview_lf_frame,
jxl/src/frame/lf_preview.rs:24-387), built from what exists: the oracle's Upsample8x and colour stage, and the
conversions, orientation and byte order of tests/save_ref.py.

What the preview does differently from a frame's save tail (lf_preview.rs:60,67,72,208-214): every converter is built
with ::new(0, ..) and every row is processed at position (0, 0), so all three colour channels convert as pipeline
channel 0 in row 0 with the column counted from the rect's left edge, and the f16 conversion never clamps.  For U8 that
is the dither value dither[0][(X - 8 * x0) % 32], X the image column."""
import numpy as np

import save_ref as sr


XYB_FACTORS = (1.0 / 3000.0, 1.0 / 700.0, 1.0 / 300.0)  # lf_quant_factors of the Modular XYB LF frames below; not the defaults


# ---- a Modular XYB LF frame, for the tests that fill a slot through jxlh_frame_save_lf
def modular_xyb(rng, w, h):
    """coded Y, X, B samples whose dequantised values are LF-like"""
    y = rng.integers(100, 500, size=(h, w)).astype(np.int32)
    x = rng.integers(-40, 40, size=(h, w)).astype(np.int32)
    b = rng.integers(-60, 60, size=(h, w)).astype(np.int32)
    return [y, x, b]


def render_modular_xyb(ctx, chans):
    from jxl_rs_amd import lib
    h, w = chans[0].shape
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = 0, 0
    for i, v in enumerate(XYB_FACTORS):
        p.lf_quant_factors[i] = v
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*chans, 8 | lib.MODULAR_XYB)
    ctx.frame_run()


# ---- the preview
def slot_size(image_w, image_h):
    return (image_w + 7) // 8, (image_h + 7) // 8


def upsampled_image(oracle, planes, image_w, image_h, weights8=None):
    """steps 1 and 2: Upsample8x of each WHOLE slot plane (so the 5x5 window mirrors against the slot, :127-140),
    cropped to the image"""
    return [oracle.upsample(8, np.ascontiguousarray(p, dtype=np.float32), weights8)[:image_h, :image_w].copy() for p in planes]


def preview_samples(oracle, d, planes, image_w, image_h, colour, rect=None, weights8=None, upsampled=None):
    """the samples of one rect (x0, y0, w, h in LF pixels; the whole slot by default):
    ([rows, columns, samples per pixel] native samples, (X0, Y0) of their first image pixel)"""
    sw, sh = slot_size(image_w, image_h)
    assert planes[0].shape == (sh, sw), (planes[0].shape, (sh, sw))
    x0, y0, w, h = (0, 0, sw, sh) if rect is None else rect
    up = upsampled if upsampled is not None else upsampled_image(oracle, planes, image_w, image_h, weights8)
    X0, Y0, X1, Y1 = 8 * x0, 8 * y0, min(8 * (x0 + w), image_w), min(8 * (y0 + h), image_h)
    rgb = sr.colour_stage(oracle, [p[Y0:Y1, X0:X1] for p in up], colour)
    fmt, depth = d["format"], d["bit_depth"]
    assert sorted(d["channels"]) == [0, 1, 2] and not d["spot"] and d["premultiply"] is None
    spp = 3 + (1 if d["fill_opaque_alpha"] else 0)
    out = np.zeros((Y1 - Y0, X1 - X0, spp), dtype=sr.SAMPLE_DTYPE[fmt])
    x = np.arange(X1 - X0)[None, :]  # X - 8 * x0
    for k, ch in enumerate(d["channels"]):
        out[:, :, k] = sr.convert(rgb[ch], fmt, depth, ch=0, x=x, y=0, f16_clamp=None)
    if d["fill_opaque_alpha"]:
        out[:, :, 3] = sr.opaque_alpha(fmt, depth)
    return out, (X0, Y0)


def paste(image, d, samples, origin, image_w, image_h):
    """writes a rect's samples at their display positions into the oriented image [oh, ow, spp] (native samples)"""
    hh, ww, _ = samples.shape
    ys, xs = np.mgrid[0:hh, 0:ww]
    dx, dy = sr.display_pixel(d["orientation"], xs + origin[0], ys + origin[1], image_w, image_h)
    image[dy, dx] = samples


def lf_preview_ref(oracle, d, planes, image_w, image_h, colour, rects=None, weights8=None, background=None):
    """the oriented image after the preview of `rects` (default: one rect covering the slot), as it lies in memory:
    [oh, ow * spp] samples in the byte order asked for.  background: the native sample value of pixels no rect covers
    (default 0)"""
    sw, sh = slot_size(image_w, image_h)
    rects = [(0, 0, sw, sh)] if rects is None else rects
    spp = 3 + (1 if d["fill_opaque_alpha"] else 0)
    ow, oh = sr.oriented_size(d["orientation"], image_w, image_h)
    img = np.zeros((oh, ow, spp), dtype=sr.SAMPLE_DTYPE[d["format"]])
    if background is not None:
        img[:] = background
    up = upsampled_image(oracle, planes, image_w, image_h, weights8)
    for r in rects:
        if r[2] == 0 or r[3] == 0:
            continue
        s, origin = preview_samples(oracle, d, planes, image_w, image_h, colour, r, upsampled=up)
        paste(img, d, s, origin, image_w, image_h)
    img = sr.byte_order(img, d["big_endian"])
    return img.reshape(oh, -1)


def covered_mask(d, image_w, image_h, rects):
    """bool [oh, ow]: the display pixels the rects write"""
    ow, oh = sr.oriented_size(d["orientation"], image_w, image_h)
    m = np.zeros((oh, ow, 1), dtype=bool)
    for x0, y0, w, h in rects:
        X0, Y0, X1, Y1 = 8 * x0, 8 * y0, min(8 * (x0 + w), image_w), min(8 * (y0 + h), image_h)
        if X1 > X0 and Y1 > Y0:
            paste(m, d, np.ones((Y1 - Y0, X1 - X0, 1), dtype=bool), (X0, Y0), image_w, image_h)
    return m[:, :, 0]
