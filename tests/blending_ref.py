"""numpy float32 restatement of the reference's frame blending: BlendingStage::process_row_chunk
(jxl/src/render/stages/blending.rs:97-166) followed by ExtendToImageDimensionsStage (render/stages/extend.rs:59-84),
built on patches_ref.perform_blending (which is held to the reference's own vectors).

The frame is perform_blending's `bg`; the reference slot named by a blending's `source` is its `fg`, read at image
coordinates (x0 + x, y0 + y).  Colour reads channels 0..2 of color.source, extra channel i reads channel 3 + i of
ec[i].source; a slot that is not set reads as zeros.  Frame pixels outside the image are dropped, image pixels outside
the frame take the source slot's value.

A blending is (mode, alpha_channel, clamp, source) with mode a BlendingMode value (headers/frame_header.rs:98-104)."""
from collections import namedtuple

import numpy as np

import patches_ref as pr

REPLACE, ADD, BLEND, ALPHA_WEIGHTED_ADD, MUL = range(5)
# From<&BlendingInfo> for PatchBlending (blending.rs:41-56)
MODE_MAP = {REPLACE: pr.NONE, ADD: pr.ADD, MUL: pr.MUL, BLEND: pr.BLEND_BELOW, ALPHA_WEIGHTED_ADD: pr.AWA_BELOW}

# x0, y0: FrameHeader::x0 / y0 (may be negative); image_w, image_h: FileHeader::size; color: a blending; ec: one blending
# per extra channel; ec_flags: EC_ALPHA / EC_ALPHA_ASSOCIATED per extra channel
BlendDesc = namedtuple("BlendDesc", "x0 y0 image_w image_h color ec ec_flags")


def patch_blending(b):
    mode, alpha, clamp, _source = b
    return (MODE_MAP[mode], alpha, bool(clamp))


def _slot(refs, s):
    if isinstance(refs, dict):
        return refs.get(s)
    return refs[s] if s < len(refs) else None


def source_planes(refs, desc):
    """the image-sized planes the stages read as `fg` / extend from: channel c from its own source slot, zeros when the
    slot is not set"""
    out = []
    for c in range(3 + len(desc.ec)):
        src = desc.color[3] if c < 3 else desc.ec[c - 3][3]
        r = _slot(refs, src)
        if r is None:
            out.append(np.zeros((desc.image_h, desc.image_w), np.float32))
        else:
            out.append(np.ascontiguousarray(r[c][:desc.image_h, :desc.image_w], dtype=np.float32).copy())
    return out


def blend_frame(frame_planes, refs, desc):
    """frame_planes: 3 + num_ec float32 [h, w] arrays already in the output colour space; refs: list or dict slot ->
    3 + num_ec planes (at least image-sized) or None; returns the 3 + num_ec image_h x image_w planes"""
    num_ec = len(desc.ec)
    assert len(frame_planes) == 3 + num_ec and len(desc.ec_flags) == num_ec
    h, w = frame_planes[0].shape
    canvas = source_planes(refs, desc)
    ix0, ix1 = max(desc.x0, 0), min(desc.x0 + w, desc.image_w)
    iy0, iy1 = max(desc.y0, 0), min(desc.y0 + h, desc.image_h)
    if ix0 >= ix1 or iy0 >= iy1:
        return canvas
    bg = [np.ascontiguousarray(p[iy0 - desc.y0:iy1 - desc.y0, ix0 - desc.x0:ix1 - desc.x0], dtype=np.float32).copy()
          for p in frame_planes]
    fg = [c[iy0:iy1, ix0:ix1].copy() for c in canvas]
    pr.perform_blending(bg, fg, patch_blending(desc.color), [patch_blending(b) for b in desc.ec], list(desc.ec_flags))
    for c, b in zip(canvas, bg):
        c[iy0:iy1, ix0:ix1] = b
    return canvas


# ---------------------------------------------------------------- the reference's row-chunk form, transcribed
def process_row_chunk(desc, refs, position, xsize, row):
    """blending.rs:104-166.  row: 3 + num_ec 1-D arrays of the frame's row position[1], starting at frame column
    position[0], xsize long, blended in place"""
    num_ec = len(desc.ec)
    fg_y0 = desc.y0 + position[1]
    fg_x0 = desc.x0 + position[0]
    fg_x1 = fg_x0 + xsize
    bg_x0 = 0
    bg_x1 = xsize
    if fg_x1 <= 0 or fg_x0 >= desc.image_w or fg_y0 < 0 or fg_y0 >= desc.image_h:
        return
    if fg_x0 < 0:
        bg_x0 -= fg_x0
        fg_x0 = 0
    if fg_x1 > desc.image_w:
        bg_x1 = bg_x0 + desc.image_w - fg_x0
        fg_x1 = desc.image_w
    zeros = np.zeros(desc.image_w, np.float32)
    fg_buf = [zeros[fg_x0:fg_x1] for _ in range(3 + num_ec)]
    rf = _slot(refs, desc.color[3])
    if rf is not None:
        for c in range(3):
            fg_buf[c] = rf[c][fg_y0][fg_x0:fg_x1]
    for i in range(num_ec):
        rf = _slot(refs, desc.ec[i][3])
        if rf is not None:
            fg_buf[3 + i] = rf[3 + i][fg_y0][fg_x0:fg_x1]
    bg = [r[bg_x0:bg_x1] for r in row]  # views: blended in place
    pr.perform_blending(bg, [np.asarray(f, np.float32) for f in fg_buf], patch_blending(desc.color),
                        [patch_blending(b) for b in desc.ec], list(desc.ec_flags))


def extend_row_chunk(desc, refs, position, xsize, c, row):
    """extend.rs:66-83.  position: image coordinates; row: xsize samples of channel c, overwritten"""
    x0 = position[0]
    x1 = x0 + xsize
    y0 = position[1]
    source = desc.color[3] if c < 3 else desc.ec[c - 3][3]
    rf = _slot(refs, source)
    bg = rf[c][y0] if rf is not None else np.zeros(desc.image_w, np.float32)
    row[0:xsize] = bg[x0:x1]


def blend_frame_chunked(frame_planes, refs, desc, rng, max_chunk=70):
    """the same image as blend_frame, made the way the reference's pipeline makes it: BlendingStage over row chunks of
    the FRAME at arbitrary positions and widths, the chunks' in-image part laid onto the image at the frame's origin,
    ExtendToImageDimensionsStage over row chunks of the IMAGE outside the frame's rectangle.  Pixels no stage wrote stay
    NaN, so a gap shows."""
    nch = 3 + len(desc.ec)
    h, w = frame_planes[0].shape
    image = [np.full((desc.image_h, desc.image_w), np.nan, np.float32) for _ in range(nch)]
    for y in range(h):
        x = 0
        while x < w:
            n = min(w - x, int(rng.integers(1, max_chunk)))
            row = [np.ascontiguousarray(p[y, x:x + n], dtype=np.float32).copy() for p in frame_planes]
            process_row_chunk(desc, refs, (x, y), n, row)
            iy = desc.y0 + y
            a, b = max(desc.x0 + x, 0), min(desc.x0 + x + n, desc.image_w)
            if 0 <= iy < desc.image_h and a < b:
                for c in range(nch):
                    image[c][iy, a:b] = row[c][a - desc.x0 - x:b - desc.x0 - x]
            x += n
    fx0, fx1 = max(desc.x0, 0), min(desc.x0 + w, desc.image_w)
    for y in range(desc.image_h):
        in_rows = desc.y0 <= y < desc.y0 + h and fx0 < fx1
        spans = [(0, fx0), (fx1, desc.image_w)] if in_rows else [(0, desc.image_w)]
        for a, b in spans:
            x = a
            while x < b:
                n = min(b - x, int(rng.integers(1, max_chunk)))
                for c in range(nch):
                    extend_row_chunk(desc, refs, (x, y), n, c, image[c][y, x:x + n])
                x += n
    return image
