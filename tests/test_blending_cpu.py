"""The numpy restatement of frame blending (tests/blending_ref.py): its mode mapping held to the reference's own
blending vectors, its whole-image geometry held to a literal transcription of the reference's two row-chunk stages, and
unset slots reading as zeros channel by channel."""
import json
import os

import numpy as np
import pytest

import blending_ref as br
import patches_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "patches_kat.json")))

# The frame is the `bg` of perform_blending and the frame modes map onto the *below* patch modes.  Add and Mul are
# reached directly (frame = the case's bg, source = its fg); the fg-on-top cases with the roles exchanged (frame = the
# case's fg, source = its bg): their Replace becomes frame-mode Replace (-> None: the frame stays), BlendAbove becomes
# Blend (-> BlendBelow), AlphaWeightedAddAbove becomes AlphaWeightedAdd (-> AlphaWeightedAddBelow).
DIRECT = {pr.ADD: br.ADD, pr.MUL: br.MUL}
EXCHANGED = {pr.REPLACE: br.REPLACE, pr.BLEND_ABOVE: br.BLEND, pr.AWA_ABOVE: br.ALPHA_WEIGHTED_ADD}


def _frame_case(case):
    modes = [case["color_blending"][0]] + [b[0] for b in case["ec_blendings"]]
    if case["name"] in ("test_color_add", "test_color_mul_with_clamp"):
        table, frame, source = DIRECT, case["bg"], case["fg"]
    else:
        table, frame, source = EXCHANGED, case["fg"], case["bg"]
    assert all(m in table for m in modes), (case["name"], modes)

    def info(b):
        return (table[b[0]], b[1], bool(b[2]), 0)
    desc = br.BlendDesc(0, 0, 1, 1, info(case["color_blending"]), [info(b) for b in case["ec_blendings"]], case["ec_flags"])
    return desc, frame, source


def test_all_eight_reference_cases_are_reached():
    assert len(KAT["cases"]) == 8
    for case in KAT["cases"]:
        _frame_case(case)


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_mode_mapping_matches_reference_kat(case):
    desc, frame, source = _frame_case(case)
    planes = [np.array([[v]], np.float32) for v in frame]
    refs = [[np.array([[v]], np.float32) for v in source]]
    got = br.blend_frame(planes, refs, desc)
    for c in case["checked_channels"]:
        assert abs(float(got[c][0, 0]) - case["expected"][c]) <= KAT["max_abs_delta"], (c, float(got[c][0, 0]), case["expected"][c])


IMAGE_W, IMAGE_H = 97, 61
# (x0, y0, frame w, frame h): negative, inside, straddling each edge, wholly outside on every side, larger than the image
GEOMETRY = [
    (0, 0, IMAGE_W, IMAGE_H), (10, 7, 40, 30), (-13, -9, 50, 40), (-13, 20, 50, 20), (20, -9, 30, 40),
    (70, 10, 50, 20), (30, 40, 20, 50), (80, 50, 40, 30), (-5, -5, IMAGE_W + 20, IMAGE_H + 11),
    (-60, 10, 50, 20), (IMAGE_W, 10, 30, 20), (10, -45, 30, 40), (10, IMAGE_H, 30, 20), (-50, -50, 50, 50),
    (IMAGE_W + 3, IMAGE_H + 3, 8, 8), (96, 60, 1, 1), (-3, 0, 4, 1), (5, 5, 1, 37),
]


def _random_case(rng, num_ec, flags, geom):
    x0, y0, w, h = geom
    refs = [[rng.uniform(-0.5, 1.5, (IMAGE_H + 5, IMAGE_W + 9)).astype(np.float32) for _ in range(3 + num_ec)]
            for _ in range(3)] + [None]
    frame = [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(3 + num_ec)]

    def info():
        return (int(rng.integers(0, 5)), int(rng.integers(0, max(num_ec, 1))), bool(rng.integers(0, 2)), int(rng.integers(0, 4)))
    desc = br.BlendDesc(x0, y0, IMAGE_W, IMAGE_H, info(), [info() for _ in range(num_ec)], flags)
    return frame, refs, desc


@pytest.mark.parametrize("geom", GEOMETRY, ids=["x%d_y%d_%dx%d" % g for g in GEOMETRY])
def test_row_chunks_equal_whole_image(geom):
    for k, flags in enumerate(([], [pr.EC_ALPHA], [0, pr.EC_ALPHA | pr.EC_ALPHA_ASSOCIATED])):
        rng = np.random.default_rng(1000 * k + GEOMETRY.index(geom))
        frame, refs, desc = _random_case(rng, len(flags), flags, geom)
        whole = br.blend_frame(frame, refs, desc)
        chunked = br.blend_frame_chunked(frame, refs, desc, rng)
        for c, (a, b) in enumerate(zip(whole, chunked)):
            assert a.shape == (IMAGE_H, IMAGE_W)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (flags, c)


def test_frame_outside_the_image_leaves_the_source():
    rng = np.random.default_rng(3)
    frame, refs, desc = _random_case(rng, 1, [pr.EC_ALPHA], (IMAGE_W + 3, 0, 8, 8))
    got = br.blend_frame(frame, refs, desc)
    for c, want in enumerate(br.source_planes(refs, desc)):
        assert np.array_equal(got[c], want)


def test_unset_slots_read_as_zeros_per_channel():
    rng = np.random.default_rng(17)
    ref = [rng.uniform(-0.5, 1.5, (IMAGE_H, IMAGE_W)).astype(np.float32) for _ in range(5)]
    frame = [rng.uniform(-0.5, 1.5, (20, 30)).astype(np.float32) for _ in range(5)]
    zeros = [np.zeros((IMAGE_H, IMAGE_W), np.float32) for _ in range(5)]
    # colour from slot 2 (unset), extra channel 0 from slot 1 (set), extra channel 1 from slot 3 (unset)
    desc = br.BlendDesc(11, 13, IMAGE_W, IMAGE_H, (br.ADD, 0, False, 2), [(br.ADD, 0, False, 1), (br.MUL, 0, True, 3)], [0, 0])
    got = br.blend_frame(frame, {1: ref}, desc)
    # the same with explicit zero planes in the unset slots
    mixed = {1: ref, 2: zeros, 3: zeros}
    want = br.blend_frame(frame, mixed, desc)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    inside = (slice(13, 33), slice(11, 41))
    for c in range(3):  # frame + 0 inside, 0 outside
        assert np.array_equal(got[c][inside], frame[c] + np.float32(0))
        out = got[c].copy()
        out[inside] = 0
        assert not out.any()
    assert np.array_equal(got[3][inside], frame[3] + ref[3][inside])  # its own slot is set
    assert np.array_equal(got[3][0], ref[3][0])
    assert not got[4].any()  # Mul by a zero source, zero outside
