"""The numpy restatement of the patches stage (tests/patches_ref.py) held to the reference's own blending tests, and the
property the device kernel relies on: applying a dictionary in row chunks of any widths equals applying it whole."""
import json
import os

import numpy as np
import pytest

import patches_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "patches_kat.json")))


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_blending_matches_reference_kat(case):
    bg = [np.array([v], np.float32) for v in case["bg"]]
    fg = [np.array([v], np.float32) for v in case["fg"]]
    pr.perform_blending(bg, fg, tuple(case["color_blending"]), [tuple(b) for b in case["ec_blendings"]], case["ec_flags"])
    for c in case["checked_channels"]:
        assert abs(float(bg[c][0]) - case["expected"][c]) <= KAT["max_abs_delta"], (c, float(bg[c][0]), case["expected"][c])


def kat_row_planes(case):
    frame = [np.array(c, np.float32) for c in case["frame"]]
    refs = {s: [np.array(c, np.float32) for c in r] for s, r in enumerate(case["refs"])}
    patches = [tuple(p) for p in case["patches"]]
    blendings = [tuple(b) for b in case["blendings"]]
    return frame, refs, patches, blendings


@pytest.mark.parametrize("case", KAT["add_one_row_cases"], ids=[c["name"] for c in KAT["add_one_row_cases"]])
def test_add_one_row_matches_reference_kat(case):
    """placement, reference offsets, clipping and order of application, through apply_patches"""
    frame, refs, patches, blendings = kat_row_planes(case)
    pr.apply_patches(frame, patches, blendings, refs, case["ec_flags"])
    for c, (got, want) in enumerate(zip(frame, case["expected"])):
        assert np.max(np.abs(got - np.array(want, np.float32))) <= KAT["add_one_row_max_abs_delta"], (c, got, want)


def random_dictionary(rng, w, h, n, num_ec, ref_w=96, ref_h=80, slots=2):
    patches, blendings = [], []
    for _ in range(n):
        xs, ys = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        patches.append((int(rng.integers(0, w - xs + 1)), int(rng.integers(0, h - ys + 1)), int(rng.integers(0, slots)),
                        int(rng.integers(0, ref_w - xs + 1)), int(rng.integers(0, ref_h - ys + 1)), xs, ys))
        for _ in range(1 + num_ec):
            blendings.append((int(rng.integers(0, 8)), int(rng.integers(0, max(num_ec, 1))), bool(rng.integers(0, 2))))
    refs = [[rng.uniform(-0.5, 1.5, (ref_h, ref_w)).astype(np.float32) for _ in range(3 + num_ec)] for _ in range(slots)]
    return patches, blendings, refs


@pytest.mark.parametrize("num_ec,flags", [(0, []), (1, [pr.EC_ALPHA]), (2, [0, pr.EC_ALPHA | pr.EC_ALPHA_ASSOCIATED]),
                                          (2, [pr.EC_ALPHA, 0])])
def test_row_chunks_equal_whole_application(num_ec, flags):
    rng = np.random.default_rng(5 + num_ec)
    w, h = 157, 93
    patches, blendings, refs = random_dictionary(rng, w, h, 120, num_ec)
    base = [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(3 + num_ec)]
    whole = pr.apply_patches([p.copy() for p in base], patches, blendings, refs, flags)
    chunked = [p.copy() for p in base]
    y = 0
    while y < h:  # row chunks of random heights, each cut into random widths (the reference's row-chunked render)
        y1 = min(h, y + int(rng.integers(1, 9)))
        x = 0
        while x < w:
            x1 = min(w, x + int(rng.integers(1, 70)))
            pr.apply_patches(chunked, patches, blendings, refs, flags, x0=x, x1=x1, y0=y, y1=y1)
            x = x1
        y = y1
    for a, b in zip(whole, chunked):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # and the dictionary changed something (an empty comparison shows nothing)
    assert any(not np.array_equal(a, b) for a, b in zip(whole, base))


def test_order_of_application_matters():
    rng = np.random.default_rng(9)
    w, h = 64, 48
    patches, blendings, refs = random_dictionary(rng, w, h, 60, 1)
    base = [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(4)]
    fwd = pr.apply_patches([p.copy() for p in base], patches, blendings, refs, [pr.EC_ALPHA])
    rb = [blendings[2 * i:2 * i + 2] for i in range(len(patches))][::-1]
    rev = pr.apply_patches([p.copy() for p in base], patches[::-1], [b for pair in rb for b in pair], refs, [pr.EC_ALPHA])
    assert any(not np.array_equal(a, b) for a, b in zip(fwd, rev))


def test_alpha_channel_is_ignored_where_the_reference_does_not_read_it():
    # num_ec == 1: PatchesDictionary::read leaves alpha_channel at 0 (patches.rs:585-596)
    assert pr.sanitize((pr.BLEND_ABOVE, 5, 1), 1) == (pr.BLEND_ABOVE, 0, True)
    assert pr.sanitize((pr.ADD, 1, 0), 3) == (pr.ADD, 0, False)
    assert pr.sanitize((pr.AWA_BELOW, 2, 0), 3) == (pr.AWA_BELOW, 2, False)
