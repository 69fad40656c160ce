"""tests/lf_preview_ref.py against tests/save_ref.py: where the reference's LF preview converts like a frame's save tail
and where it does not (jxl/src/frame/lf_preview.rs:60,67,72,208-214: every converter is built for channel 0 and every
row handed over at position (0, 0))."""
import json
import os

import numpy as np
import pytest

import lf_preview_ref as lp
import save_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = (0.2627, 0.678, 0.0593)
IW, IH = 61, 45  # slot 8 x 6; neither side a multiple of 8


def colour_tuple(oracle, tf="srgb", param=0.0, intensity=255.0):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["output_stage"]
    return ("xyb", tf, oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, intensity), param, LUM)


def slot_planes(seed, image_w=IW, image_h=IH):
    """a non-constant XYB image: X small around 0, Y and B in 0 .. 0.9, with a few values outside"""
    sw, sh = lp.slot_size(image_w, image_h)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.02, 0.02, (sh, sw)).astype(np.float32)
    y = rng.uniform(0.0, 0.9, (sh, sw)).astype(np.float32)
    b = (y + rng.uniform(-0.1, 0.1, (sh, sw))).astype(np.float32)
    y.flat[0], y.flat[-1] = 1.6, -0.3
    return [x, y, b]


@pytest.mark.parametrize("orientation", [1, 6, 8])
@pytest.mark.parametrize("fmt", [sr.U16, sr.F16, sr.F32], ids=["u16", "f16", "f32"])
def test_position_free_formats_equal_the_save_tail(oracle, fmt, orientation):
    planes = slot_planes(1)
    colour = colour_tuple(oracle)
    up = lp.upsampled_image(oracle, planes, IW, IH)
    for channels, fill in (([0, 1, 2], False), ([2, 1, 0], True)):
        d = sr.desc(channels, fmt, fill_opaque_alpha=fill, orientation=orientation, big_endian=orientation == 6)
        assert np.array_equal(lp.lf_preview_ref(oracle, d, planes, IW, IH, colour), sr.save(oracle, d, up, colour)), d


def test_u8_dithers_every_channel_and_row_like_channel_0_row_0(oracle):
    planes = slot_planes(2)
    colour = colour_tuple(oracle)
    up = lp.upsampled_image(oracle, planes, IW, IH)
    d = sr.desc([0, 1, 2], sr.U8)
    got = lp.lf_preview_ref(oracle, d, planes, IW, IH, colour).reshape(IH, IW, 3)
    want = sr.save(oracle, d, up, colour).reshape(IH, IW, 3)
    assert np.array_equal(got[0, :, 0], want[0, :, 0])  # channel 0, row 0: the one place the two agree by construction
    assert np.any(got[1:, :, 0] != want[1:, :, 0])      # no row term
    assert np.any(got[0, :, 1] != want[0, :, 1])        # no 23 * ch / 13 * ch term
    assert np.any(got[0, :, 2] != want[0, :, 2])
    # and it is exactly the save tail's conversion of every row and channel at (channel 0, row 0)
    rgb = sr.colour_stage(oracle, up, colour)
    for ch in range(3):
        assert np.array_equal(got[:, :, ch], sr.f32_to_u8(rgb[ch], np.arange(IW)[None, :], 0, 0))


def test_the_dither_phase_restarts_at_a_rects_left_edge(oracle):
    planes = slot_planes(3)
    colour = colour_tuple(oracle)
    sw, sh = lp.slot_size(IW, IH)
    d = sr.desc([0, 1, 2], sr.U8)
    one = lp.lf_preview_ref(oracle, d, planes, IW, IH, colour).reshape(IH, IW, 3)
    two = lp.lf_preview_ref(oracle, d, planes, IW, IH, colour, rects=[(0, 0, 3, sh), (3, 0, sw - 3, sh)]).reshape(IH, IW, 3)
    assert np.array_equal(one[:, :24], two[:, :24])  # the rect at x0 = 0 has the one-rect phase
    assert np.any(one[:, 24:] != two[:, 24:])        # 24 is no multiple of 32: the second rect's phase differs
    # ... and through nothing else: converted at the phase of its own left edge, the right part is the two-rect image
    up = lp.upsampled_image(oracle, planes, IW, IH)
    rgb = sr.colour_stage(oracle, up, colour)
    for ch in range(3):
        assert np.array_equal(two[:, 24:, ch], sr.f32_to_u8(rgb[ch][:, 24:], np.arange(IW - 24)[None, :], 0, 0))
    # the position-free formats do not see the split at all
    d16 = sr.desc([0, 1, 2], sr.U16)
    assert np.array_equal(lp.lf_preview_ref(oracle, d16, planes, IW, IH, colour),
                          lp.lf_preview_ref(oracle, d16, planes, IW, IH, colour, rects=[(0, 0, 3, sh), (3, 0, sw - 3, sh)]))


def test_f16_is_never_clamped(oracle):
    planes = slot_planes(4)
    colour = colour_tuple(oracle)
    up = lp.upsampled_image(oracle, planes, IW, IH)
    d = sr.desc([0, 1, 2], sr.F16, f16_clamp=sr.F16_CLAMP_PQ)
    got = lp.lf_preview_ref(oracle, d, planes, IW, IH, colour)
    assert np.array_equal(got, sr.save(oracle, sr.desc([0, 1, 2], sr.F16), up, colour))
    assert not np.array_equal(got, sr.save(oracle, d, up, colour))  # the input leaves [0, 1]: a clamp would show
