"""Splines on the host: the CPU restatement the GPU tests compare against (tests/splines_ref.py over
tests/cpp/splines_ref.c) and the library's jxlh_splines_build_segments are both held to the reference's own known
answers (the tests of jxl/src/features/spline.rs, numbers in tests/golden/splines_kat.json) at the reference's
tolerances; the library's builder equals the restatement bit for bit; every error of the reference comes back as
JXLH_ERR_INVALID_ARGUMENT.  tests/cpp/splines_host_check.cc runs the plain header (builder, bounds, binner) under the
address and undefined-behaviour sanitizers as a stand-alone program."""
import json
import os
import subprocess

import numpy as np
import pytest

import splines_ref
from helpers import bit_equal
from jxl_rs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def skat():
    with open(os.path.join(ROOT, "tests", "golden", "splines_kat.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ref():
    return splines_ref.Ref(fused=True)


@pytest.fixture(scope="module")
def ref_unfused():
    return splines_ref.Ref(fused=False)


def close(got, want, max_abs, max_rel=None):
    """assert_close! of the reference (tests/macros.rs:122-192): the absolute bound, and with `rel:` the relative one
    too, 2 |a - b| / (|a| + |b| + 1e-16)"""
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    err = np.abs(g - w)
    assert np.all(err <= max_abs), "abs %g > %g" % (err.max(), max_abs)
    if max_rel is not None:
        rel = 2.0 * err / (np.abs(g) + np.abs(w) + 1e-16)
        assert np.all(rel <= max_rel), "rel %g > %g" % (rel.max(), max_rel)


def segment_close(got, want, skat):
    """verify_segment_almost_equal (:1722-1736); want: a dict of the fixture"""
    t = skat["segment_tol"]
    w = [want["center_x"], want["center_y"], want["maximum_distance"], want["inv_sigma"],
         want["sigma_over_4_times_intensity"]] + list(want["color"])
    for g, v in zip(np.asarray(got, dtype=np.float32).reshape(8), w):
        close(g, F(v), t["abs"], t["rel"])


def build_lib(splines, adjustment, y_to_x_lf, y_to_b_lf, xsize, ysize, high_precision=False):
    st, seg = lib.try_build_spline_segments(splines, adjustment, y_to_x_lf, y_to_b_lf, xsize, ysize, high_precision)
    return st, seg


def cache_input(skat):
    k = skat["init_draw_cache"]
    splines = [splines_ref.kat_spline(q, s) for q, s in zip(k["splines"], k["starting_points"])]
    args = dict(adjustment=k["quantization_adjustment"], y_to_x_lf=k["y_to_x_lf"], y_to_b_lf=k["y_to_b_lf"],
                xsize=k["image_xsize"], ysize=k["image_ysize"], high_precision=k["high_precision"])
    return splines, args


# ---------------------------------------------------------------- the restatement against the reference's known answers
def test_dequantize(ref, skat):
    k = skat["dequantize"]
    assert len(k["cases"]) == 3
    for case in k["cases"]:
        want = case["want"]
        got = ref.dequantize(splines_ref.kat_spline(case["quantized"], want["control_points"][0]),
                             k["quantization_adjustment"], k["y_to_x"], k["y_to_b"], k["image_size"])
        assert got is not None
        pts, cd, sd, area = got
        close(pts, F(want["control_points"]), k["tol_points"])
        for c in range(3):
            close(cd[c], F(want["color_dct"][c]), k["tol_dct"])
        close(sd, F(want["sigma_dct"]), k["tol_dct"])
        assert area == want["estimated_area_reached"]


def test_centripetal_catmull_rom_spline(ref, skat):
    k = skat["catmull_rom"]
    got = ref.catmull_rom(k["control_points"])
    want = F(k["want"])
    assert got.shape == want.shape == (17, 2)
    close(got[:, 0], want[:, 0], k["tol_x"])  # (the reference compares x only)
    close(got[:, 1], want[:, 1], 1e-6)


def test_equally_spaced_points(ref, skat):
    k = skat["equally_spaced"]
    got = ref.equally_spaced(k["points"], k["desired"])
    close(got, F(k["want"]), k["tol"])


def test_dct32(ref, skat):
    k = skat["dct32"]
    coeffs = F([F(k["coeff_step"]) * F(i) for i in range(32)])
    for t, want in enumerate(k["want"]):
        close(ref.idct_original(coeffs, t), F(want), k["tol"])
        close(ref.idct_fast(coeffs, t), ref.idct_original(coeffs, t), k["tol_fast_vs_original"])


def test_spline_segments_add_segment(ref, skat):
    k = skat["add_segment"]
    got = ref.add_segment(k["center"], k["intensity"], k["color"], k["sigma"], k["high_precision"])
    segment_close(got, k["want"], skat)
    close(got[2], F(k["want"]["maximum_distance"]), 1e-5)  # 3.65961 in float32, to the digits given
    _, _, y_lo, y_hi = ref.segment_box(got, 1 << 20, 1 << 20)
    assert list(range(y_lo, y_hi)) == k["rows"] == list(range(16, 25))


def test_spline_segments_add_segments_from_points(ref, skat):
    k = skat["add_segments_from_points"]
    color = F([[F(0.1) * F(c) + F(0.05) * F(i) for i in range(32)] for c in range(3)])
    sigma = F([F(0.06) * F(i) for i in range(32)])
    length = F(np.sqrt(F(2.0))) + F(1.0)
    got = ref.segments_from_points(color, sigma, k["points"], length, k["desired"], k["high_precision"])
    assert got.shape == (3, 8)
    for g, want, rows in zip(got, k["want"], k["rows"]):
        segment_close(g, want, skat)
        _, _, y_lo, y_hi = ref.segment_box(g, 1 << 20, 1 << 20)
        assert (y_lo, y_hi - 1) == tuple(rows)
    assert got[1][3] < 0 and got[2][3] < 0  # negative inv_sigma


def test_init_draw_cache(ref, skat):
    k = skat["init_draw_cache"]
    splines, args = cache_input(skat)
    got = ref.build(splines, **args)
    assert got is not None and got.shape == (k["n_segments"], 8) == (1940, 8)
    for index, want in k["samples"]:
        segment_close(got[index], want, skat)
    assert (got[:, 3] < 0).any()


# ---------------------------------------------------------------- the library's builder
def test_library_builder_known_answers(skat):
    k = skat["init_draw_cache"]
    splines, args = cache_input(skat)
    st, got = build_lib(splines, **args)
    assert st == lib.OK and got.shape == (1940, 8)
    for index, want in k["samples"]:
        segment_close(got[index], want, skat)


def test_library_builder_equals_restatement_bit_for_bit(ref, skat):
    splines, args = cache_input(skat)
    cases = [(splines, args), ([splines_ref.CONSISTENCY_SPLINE], splines_ref.CONSISTENCY_ARGS)]
    k = skat["dequantize"]
    for case in k["cases"]:  # the three splines of the dequantize test, low and high precision, adjustments of both signs
        sp = splines_ref.kat_spline(case["quantized"], case["want"]["control_points"][0])
        for adj, hp in ((0, False), (3, True), (-2, False)):
            cases.append(([sp], dict(adjustment=adj, y_to_x_lf=0.25, y_to_b_lf=0.875, xsize=1 << 15, ysize=1 << 15,
                                     high_precision=hp)))
    for sp, a in cases:
        want = ref.build(sp, **a)
        st, got = build_lib(sp, **a)
        assert want is not None and st == lib.OK
        assert got.shape == want.shape and got.shape[0] > 100
        assert bit_equal(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]


def test_count_only_call_and_capacity(skat):
    splines, args = cache_input(skat)
    st, n = lib.try_build_spline_segments(splines, args["adjustment"], args["y_to_x_lf"], args["y_to_b_lf"],
                                          args["xsize"], args["ysize"], args["high_precision"], count_only=True)
    assert st == lib.OK and n == 1940
    st, n = lib.try_build_spline_segments([], 0, 0.0, 1.0, 64, 64, count_only=True)
    assert st == lib.OK and n == 0
    # a buffer that is too small: nothing partial
    import ctypes as C
    L = lib._lib()
    qs = (lib.QuantizedSpline * 1)()
    d = np.ascontiguousarray(np.asarray(splines_ref.CONSISTENCY_SPLINE[0], dtype=np.int64))
    qs[0].control_points, qs[0].n_points = d.ctypes.data, d.shape[0]
    qs[0].color_dct[:] = [int(v) for v in np.asarray(splines_ref.CONSISTENCY_SPLINE[1]).reshape(96)]
    qs[0].sigma_dct[:] = list(splines_ref.CONSISTENCY_SPLINE[2])
    qs[0].start_x, qs[0].start_y = splines_ref.CONSISTENCY_SPLINE[3]
    out = np.full((4, 8), 7.0, np.float32)
    count = C.c_size_t(0)
    st = L.jxlh_splines_build_segments(C.byref(qs), 1, 0, C.c_float(0.0), C.c_float(1.0), 500, 500, 0, out.ctypes.data, 4,
                                       C.byref(count))
    assert st == lib.ERR_INVALID_ARGUMENT and count.value > 4 and np.all(out == 7.0)
    assert L.jxlh_splines_build_segments(C.byref(qs), 1, 0, C.c_float(0.0), C.c_float(1.0), 500, 500, 0, None, 0,
                                         None) == lib.ERR_INVALID_ARGUMENT
    assert L.jxlh_splines_build_segments(None, 1, 0, C.c_float(0.0), C.c_float(1.0), 500, 500, 0, None, 0,
                                         C.byref(count)) == lib.ERR_INVALID_ARGUMENT


ZC, ZS = [[0] * 32] * 3, [0] * 32
ONE_SIGMA = [4] + [0] * 31
ERRORS = {
    # validate_spline_point_pos (:144-169): the starting point, a delta, a position
    "start out of range": ([((1, 1),), ZC, ONE_SIGMA, (float(1 << 23), 0.0)], 64, 64),
    "start below range": ([((1, 1),), ZC, ONE_SIGMA, (0.0, -float((1 << 23) + 1))], 64, 64),
    "start not a number": ([((1, 1),), ZC, ONE_SIGMA, (float("nan"), 0.0)], 64, 64),
    "start beyond i32": ([((1, 1),), ZC, ONE_SIGMA, (3e9, 0.0)], 64, 64),
    "delta out of range": ([((1 << 23, 0),), ZC, ONE_SIGMA, (0.0, 0.0)], 64, 64),
    "position out of range": ([((1 << 22, 0), (1 << 21, 0)), ZC, ONE_SIGMA, (float(1 << 22), 0.0)], 64, 64),
    # QuantizedSpline::read's DELTA_LIMIT (:206-210)
    "double delta beyond the limit": ([((1 << 30, 0),), ZC, ONE_SIGMA, (0.0, 0.0)], 64, 64),
    # SplinesDistanceTooLarge (:272-277): area_limit(1) = 1024 + 2^32 < the sum of 1100 deltas of 2^22 each
    "manhattan distance": ([((1 << 22, 0),) + ((-(1 << 23) + 1, 0), ((1 << 23) - 1, 0)) * 600, ZC, ONE_SIGMA, (0.0, 0.0)],
                           1, 1),
    # SplinesAreaTooLarge (:753-759): wide sigma weights on a long spline in a small image
    "estimated area": ([((4000, 4000), (0, 0), (0, 0)), ZC, [1 << 20] * 32, (0.0, 0.0)], 8, 8),
    # SplineAdjacentCoincidingControlPoints (:107-125)
    "coinciding control points": ([((5, 5), (-5, -5)), ZC, ONE_SIGMA, (10.0, 10.0)], 64, 64),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_every_error_of_the_reference_is_invalid_argument(ref, name):
    sp, xs, ys = ERRORS[name]
    sp = tuple(sp)
    assert ref.build([sp], 0, 0.0, 1.0, xs, ys) is None, "the restatement accepts it"
    st, _ = build_lib([sp], 0, 0.0, 1.0, xs, ys)
    assert st == lib.ERR_INVALID_ARGUMENT
    # ... and a valid spline in front of it does not change that
    st, _ = build_lib([splines_ref.CONSISTENCY_SPLINE, sp], 0, 0.0, 1.0, xs, ys)
    assert st == lib.ERR_INVALID_ARGUMENT


def test_null_control_points_with_points_is_invalid():
    import ctypes as C
    qs = (lib.QuantizedSpline * 1)()
    qs[0].control_points, qs[0].n_points = None, 3
    count = C.c_size_t(0)
    assert lib._lib().jxlh_splines_build_segments(C.byref(qs), 1, 0, C.c_float(0.0), C.c_float(1.0), 64, 64, 0, None, 0,
                                                  C.byref(count)) == lib.ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the draw: fused against unfused
def test_draw_fused_and_unfused_stay_together(ref, ref_unfused):
    """The two builds of the draw differ in five roundings per pixel and segment.  The reference holds no bound for its
    splines stage across back-ends (its consistency test is ignored for sqrt differences), so the bound here is this
    test's own: the figure of the reference's cross-format check (jxl_cli/src/lib.rs:87-163: a 16-bit output within
    1e-4 of the float one on a unit range), scaled by the range the spline can add, its peak
    |colour * sigma_over_4_times_intensity * 4| (the factor (erf - erf)^2 is at most 4), and never below the unit range.
    Five roundings of 2^-24 relative each on values of that range are about 3e-7 of it: the bound is loose by design,
    it catches a build that is not the same arithmetic, not a last-bit difference."""
    seg = ref.build([splines_ref.CONSISTENCY_SPLINE], **splines_ref.CONSISTENCY_ARGS)
    rng = np.random.default_rng(5)
    base = [rng.uniform(-0.5, 1.5, (220, 300)).astype(np.float32) for _ in range(3)]
    a, b = ref.draw(base, seg), ref_unfused.draw(base, seg)
    peak = float(np.max(np.abs(seg[:, 5:8]) * np.abs(seg[:, 4:5]) * 4.0))
    changed = False
    for c in range(3):
        assert not bit_equal(a[c], base[c])
        changed |= not bit_equal(a[c], b[c])
        err = np.abs(a[c].astype(np.float64) - b[c].astype(np.float64)).max()
        print("plane %d: fused vs unfused max abs %g, range %g" % (c, err, max(1.0, peak)))
        assert err <= 1e-4 * max(1.0, peak)
    assert changed, "the two builds are the same build"


def test_draw_rule_edges(ref):
    """the per-pixel rule's corner cases: wholly left -> column 0, wholly above -> nothing, NaN distance -> (0, 0)"""
    # a -0.0 that a segment touches comes back as +0.0 or a value, however small the segment's intensity is there
    base = [np.full((20, 30), -0.0, np.float32) for _ in range(3)]

    def touched(seg):
        out = ref.draw(base, F([seg]))
        return np.argwhere(out[0].view(np.uint32) != base[0].view(np.uint32))

    left = touched([-50.0, 10.0, 3.0, 1.0, 0.25, 1.0, 1.0, 1.0])
    assert len(left) and set(left[:, 1]) == {0} and left[:, 0].min() == 7 and left[:, 0].max() == 13
    assert len(touched([10.0, -50.0, 3.0, 1.0, 0.25, 1.0, 1.0, 1.0])) == 0
    assert len(touched([100.0, 10.0, 3.0, 1.0, 0.25, 1.0, 1.0, 1.0])) == 0
    assert len(touched([10.0, 100.0, 3.0, 1.0, 0.25, 1.0, 1.0, 1.0])) == 0
    assert ref.segment_box([5.0, 5.0, float("nan"), 1.0, 0.25, 1, 1, 1], 30, 20) == (0, 1, 0, 1)
    # half away from zero: 2.5 -> 3, and -0.5 -> -1 (a row above the frame), clamped to 0
    assert ref.segment_box([4.5, 4.5, 2.0, 1.0, 0.25, 1, 1, 1], 30, 20) == (3, 8, 3, 8)
    assert ref.segment_box([1.5, 1.5, 2.0, 1.0, 0.25, 1, 1, 1], 30, 20) == (0, 5, 0, 5)


# ---------------------------------------------------------------- the plain header under the sanitizers
def test_host_header_under_sanitizers(tmp_path, ref, skat):
    """tests/cpp/splines_host_check.cc: the builder, the bounds and the binner of csrc/splines_host.h in a stand-alone
    program built with the address and undefined-behaviour sanitizers (float-cast-overflow among them), run as a child
    process.  The segments the builder must produce come from the restatement, through a file."""
    exe = os.path.join(str(tmp_path), "splines_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "splines_host_check.cc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",  # the runtimes linked in: the child needs nothing from its environment
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "jxl_rs_amd", "csrc"), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    splines, args = cache_input(skat)
    want = ref.build(splines, **args)
    path = os.path.join(str(tmp_path), "cache.bin")
    with open(path, "wb") as f:
        k = skat["init_draw_cache"]
        hdr = np.array([len(splines), want.shape[0]], dtype=np.int64)
        f.write(hdr.tobytes())
        for sp in splines:
            d = np.asarray(sp[0], dtype=np.int64).reshape(-1, 2)
            f.write(np.array([d.shape[0]], dtype=np.int64).tobytes())
            f.write(d.tobytes())
            f.write(np.asarray(sp[1], dtype=np.int32).reshape(96).tobytes())
            f.write(np.asarray(sp[2], dtype=np.int32).reshape(32).tobytes())
            f.write(np.asarray(sp[3], dtype=np.float32).tobytes())
        f.write(want.tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "splines host check: ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
