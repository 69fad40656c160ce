"""The inputs of tests/colour_domain_cases.py do what tests/test_gpu_colour_domain.py relies on, shown on the oracle
alone: the threshold rows straddle every branch point, the main sweep leaves most outputs finite and a good share inside
[0, 1] under every curve and parameter set, the Modular f32 intake hands every bit pattern on, and both oracle builds
run the whole set.  The shares are conditions on the INPUTS: if a parameter set breaks one, the inputs change, not the
cap."""
import numpy as np
import pytest

import colour_domain_cases as cd
import save_ref as sr

MAX_NON_FINITE = 0.03
MIN_IN_RANGE = 0.10


def test_plane_shapes_and_classes():
    main = cd.main_planes()
    assert cd.WIDTH % 4 != 0 and main[0].shape == (256, cd.WIDTH) and cd.main_values().size == 18944
    y = main[1].ravel().view(np.uint32)
    assert np.unique(y).size == 18944, "exponents 0..147 x 64 distinct mantissas x both signs"
    assert ((y >> 23) & 0xff).max() == 147 and np.uint32(0) in y and np.uint32(0x80000000) in y
    for p in (main[0], main[2]):  # permutations of the same values
        assert np.array_equal(np.sort(p.ravel().view(np.uint32)), np.sort(y))
    for planes in (main, cd.tail_planes(), cd.threshold_planes()[0], cd.display_planes()):
        assert all(p.dtype == np.float32 and p.shape == planes[0].shape for p in planes)
        assert planes[0].shape[1] == cd.WIDTH and planes[0].size < 65536
    tail = cd.tail_planes()
    for c in range(3):
        bits = tail[c].ravel().view(np.uint32)
        for special in (0x7f800000, 0xff800000) + cd.NAN_BITS + tuple(b | 0x80000000 for b in cd.NAN_BITS):
            assert np.uint32(special) in bits, (c, hex(special))
        assert set(range(148, 255)) <= set(((bits >> 23) & 0xff).tolist())
    # one channel alone: pixels whose other two channels are finite and small while this one is inf or NaN
    for c in range(3):
        others = [tail[k] for k in range(3) if k != c]
        alone = ~np.isfinite(tail[c]) & (np.abs(others[0]) <= 0.5) & (np.abs(others[1]) <= 0.5)
        assert alone.sum() >= len(cd.special_values()), c
    disp = cd.display_planes()
    assert disp[1].min() >= 0 and disp[1].max() <= 1 and np.abs(disp[0]).max() <= 0.03 and disp[2].min() >= 0


def test_parameter_sets_and_cases(oracle):
    assert tuple(cd.xyb_param_sets(oracle)) == cd.XYB_SETS
    ident = cd.xyb_param_sets(oracle)[cd.IDENTITY_XYB]
    assert ident.tolist() == np.eye(3).reshape(-1).tolist() + [0.0] * 6 + [1.0]  # matrix, both biases, 255 / target
    cases = cd.colour_cases()
    assert len(cases) == 16 * 4 + 2 and len({cd.case_id(c) for c in cases}) == len(cases)
    assert set(cd.ONE_EACH) <= set(cd.CURVE_IDS) and {cd.curve(n)[2] for n in cd.ONE_EACH} == set(oracle.TF_KINDS)
    for case in cases:
        label, colour = cd.colour_of(oracle, case)
        assert (colour[0] == "xyb") == (case[1] is not None) and label.startswith(case[0])


def test_threshold_rows_straddle_every_branch_point(oracle_any):
    """with the identity parameters and X = 0 the linear value is the sample's cube in R and G, and B's cube in B: at
    least 64 of the 129 neighbours lie strictly on either side of each branch point; 1.0 is hit exactly"""
    planes, slices = cd.threshold_planes()
    lin = oracle_any.xyb_to_linear(cd.xyb_param_sets(oracle_any)[cd.IDENTITY_XYB], *planes)
    with np.errstate(under="ignore"):
        cubes = [(v.ravel() * v.ravel()).astype(np.float32) * v.ravel() for v in planes]
    # two f32 products, nothing else (as values: Y + X - bias turns -0 into +0 before the cube)
    assert np.array_equal(lin[0], cubes[1]) and np.array_equal(lin[1], cubes[1]) and np.array_equal(lin[2], cubes[2])
    for t, s in zip(cd.THRESHOLDS, slices):
        v = lin[1][s]
        assert v.size == 2 * cd.THRESHOLD_ULPS + 1 and np.all(np.diff(v) > 0), t
        assert (v < t).sum() >= cd.THRESHOLD_ULPS and (v > t).sum() >= cd.THRESHOLD_ULPS, (t, (v < t).sum(), (v > t).sum())
        neg = lin[1][s.start + sum(x.stop - x.start for x in slices):][:v.size]
        assert np.array_equal(neg, -v), "the negated segment follows the positive ones"
    assert (lin[1][slices[-1]] == np.float32(1.0)).sum() == 1
    # the ends of the domain ride along: +-0, the smallest and the largest denormal, whose cubes are +-0
    edge = planes[1].ravel()[2 * slices[-1].stop:][:6].view(np.uint32)
    assert edge.tolist() == [0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x807fffff]


@pytest.mark.parametrize("name", cd.CURVE_IDS)
def test_main_sweep_stays_mostly_finite_and_partly_in_range(oracle, name):
    main = cd.main_planes()
    for label, colour in cd.colour_tuples(oracle, name):
        out = np.stack(sr.colour_stage(oracle, main, colour))
        non_finite = 1.0 - np.isfinite(out).mean()
        in_range = ((out >= 0) & (out <= 1)).mean()
        print(f"{label}: non-finite {non_finite:.4f}, in [0, 1] {in_range:.4f}")
        assert non_finite <= MAX_NON_FINITE, (label, non_finite)
        assert in_range >= MIN_IN_RANGE, (label, in_range)


def test_display_plane_fills_the_integer_ranges(oracle):
    """many distinct code values inside the range, at 8 and at 16 bits, under every curve of the read-out test"""
    disp = cd.display_planes()
    for name in cd.ONE_EACH:
        label, colour = cd.colour_tuples(oracle, name, ["default_255"])[0]
        u8 = sr.save(oracle, sr.desc([0, 1, 2], sr.U8), disp, colour)
        u16 = sr.save(oracle, sr.desc([0, 1, 2], sr.U16), disp, colour)
        inside = (u8 > 0) & (u8 < 255)
        assert inside.mean() >= 0.10 and np.unique(u8).size >= 100, (label, inside.mean(), np.unique(u8).size)
        assert np.unique(u16).size >= 1000, (label, np.unique(u16).size)


def test_two_restatements_of_the_integer_read_out_agree(oracle):
    """oracle.xyb_to_rgb_tf (C, one pass) and save_ref.save (numpy conversions behind the oracle's colour stage) give the
    same bytes on the tail, NaN -> 0 and +inf -> max included, and on the display plane (the fused build: the numpy
    conversions round ties to even, as it does)"""
    for planes in (cd.tail_planes(), cd.display_planes()):
        h, w = planes[0].shape
        for name in ("srgb", "pq_4000", "hlg_0.2", "gamma_2.4"):
            _, _, transfer, param = cd.curve(name)
            label, colour = cd.colour_tuples(oracle, name, ["default_255"])[0]
            for bits, fmt in ((8, sr.U8), (16, sr.U16)):
                for channels in (3, 4):
                    a = oracle.xyb_to_rgb_tf(colour[2], transfer, planes, w, h, channels, bits, param, cd.LUM)
                    b = sr.save(oracle, sr.desc([0, 1, 2], fmt, fill_opaque_alpha=channels == 4), planes, colour)
                    assert np.array_equal(a.reshape(b.shape), b), (label, bits, channels)


def test_integer_conversions_on_non_finite_samples(oracle):
    """what ConvertF32ToU8 / U16 make of NaN, +-inf and out-of-range samples: NaN -> 0, -inf -> 0, +inf -> max"""
    v = np.float32([np.nan, -np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0, -0.0])
    v = np.concatenate([v, cd.special_values()])
    x, y = np.arange(v.size), np.zeros(v.size, dtype=np.int64)
    want = np.where(np.isnan(v) | (v <= 0), 0, 1)
    for depth in (8, 5):
        assert np.array_equal(sr.f32_to_u8(v, x, y, 0, depth), want * ((1 << depth) - 1))
        assert [oracle.f32_to_u8(float(s), int(i), 0, 0, depth) for i, s in enumerate(v)] == (want * ((1 << depth) - 1)).tolist()
    for depth in (16, 10):
        assert np.array_equal(sr.f32_to_u16(v, depth), want * ((1 << depth) - 1))


def test_modular_f32_intake_widens_every_pattern_exactly(oracle):
    """sample_format 32 | 8 << 8: the planes the GPU test expects behind the intake are the bit patterns it put in"""
    for planes in (cd.main_planes(), cd.tail_planes(), cd.threshold_planes()[0], cd.display_planes()):
        for p in planes:
            got = oracle.modular_to_f32(p.view(np.int32), 32, 8)
            assert np.array_equal(np.asarray(got, np.float32).view(np.uint32).reshape(p.shape), p.view(np.uint32))


@pytest.mark.parametrize("name", cd.CURVE_IDS)
def test_both_oracle_builds_run_the_whole_set(oracle_any, name):
    """every plane x every curve x every parameter set through the fused and the unfused build: no trap, no crash"""
    for planes in (cd.main_planes(), cd.tail_planes(), cd.threshold_planes()[0], cd.display_planes()):
        for label, colour in cd.colour_tuples(oracle_any, name):
            out = sr.colour_stage(oracle_any, planes, colour)
            assert len(out) == 3 and all(o.shape == planes[0].shape and o.dtype == np.float32 for o in out), label


def test_comparison_rule():
    """float_bits_mismatch: equal bits pass; -0 vs +0 and inf vs max fail; any NaN answers a wanted NaN, of either sign;
    a number does not; a NaN where a number is wanted fails"""
    f = lambda *bits: np.array(bits, dtype=np.uint32)
    assert not cd.float_bits_mismatch(f(0, 0x80000000, 0x7f800000, 0x3f800000), f(0, 0x80000000, 0x7f800000, 0x3f800000)).any()
    assert cd.float_bits_mismatch(f(0x80000000, 0x7f7fffff, 0x3f800001), f(0, 0x7f800000, 0x3f800000)).all()
    assert not cd.float_bits_mismatch(f(0x7fc00000, 0xffc00000, 0x7f800001), f(0xffc00000, 0x7fc00001, 0xffffffff)).any()
    assert cd.float_bits_mismatch(f(0x7f800000, 0, 0x7fc00000), f(0x7fc00000, 0xffc00000, 0x7f800000)).all()
    h = lambda *bits: np.array(bits, dtype=np.uint16)
    assert not cd.float_bits_mismatch(h(0x7e00, 0xfe00, 0x3c00), h(0xfe00, 0x7e00, 0x3c00)).any()
    assert cd.float_bits_mismatch(h(0x7c00, 0x8000), h(0x7e00, 0x0000)).all()
