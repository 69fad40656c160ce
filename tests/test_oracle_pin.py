"""Pins the CPU oracle against every known-answer vector the reference's own tests hold
for the hot path (tests/golden/reference_kat.json).

Mirrors jxl_transforms/src/tests.rs (IDCT / reinterpreting DCT vs f64 matrix definitions
with the reference's per-shape tolerances), frame/quant_weights.rs:1221-2139,
frame/coeff_order.rs:154-178, render/stages/gaborish.rs:132-145 and
modular/transforms/squeeze.rs:107-168 (SIMD tendency == scalar tendency).
"""
import numpy as np
import pytest


def check_close(a, b, tol):
    """tests.rs:175-183: abs OR rel error below tol."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    ab = np.abs(a - b)
    rel = ab / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    bad = ~((ab < tol) | (rel < tol))
    assert not bad.any(), f"max abs {ab.max()} (tol {tol}), {bad.sum()} bad"


# The reference's tolerances are calibrated on ONE draw: every test calls random_matrix(n, m), which seeds a fresh
# ChaCha12Rng::seed_from_u64(0) and fills the matrix row-major with random_range(-1.0..1.0) (tests.rs:246-255).
# oracle/ref_rng.py restates that generator, so the oracle is held to the reference's own tolerances on the
# reference's own inputs: the f64 definition sees the f64 draw, the fast path its f32 rounding (tests.rs:266-270,
# :300-304).
def ref_draw(n, m):
    from oracle.ref_rng import random_matrix
    return random_matrix(n, m)


def test_reference_rng_restatement_known_answers():
    """The ChaCha core of oracle/ref_rng.py against the published zero-key key streams (ChaCha20: the
    well-known 76 b8 e0 ad ...; ChaCha12 / ChaCha8: eSTREAM vectors) and the structure of the draw."""
    import struct
    from oracle import ref_rng as rr
    ks = lambda r: struct.pack("<16I", *rr.chacha_block([0] * 8, 0, 0, r)).hex()
    assert ks(20).startswith("76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7")
    assert ks(12).startswith("9bf49a6a0755f953811fce125f2683d50429c3bb49e074147e0089a52eae155f")
    assert ks(8).startswith("3e00ef2f895f40d67f5bb8e81f09a5a12c840ec3ce9a7f3b181be188ef711a1e")
    # block counter in words 12-13: the second block differs, and the generator walks the words in order
    assert rr.chacha_block([0] * 8, 1, 0, 12) != rr.chacha_block([0] * 8, 0, 0, 12)
    g = rr.ChaCha12Rng(bytes(32))
    w = rr.chacha_block([0] * 8, 0, 0, 12) + rr.chacha_block([0] * 8, 1, 0, 12)
    assert [g.next_u64() for _ in range(16)] == [w[2 * i] | (w[2 * i + 1] << 32) for i in range(16)]
    # seed expansion: PCG32 stream, 8 words, deterministic; every test of the reference sees the same prefix
    assert len(rr.seed_from_u64(0)) == 32 and rr.seed_from_u64(0) != rr.seed_from_u64(1)
    a, b = rr.random_matrix(4, 3), rr.random_matrix(6, 2)
    assert np.array_equal(a.reshape(-1), b.reshape(-1))
    assert (np.abs(a) < 1.0).all()
    big = rr.random_matrix(64, 64)
    assert abs(big.mean()) < 0.05 and 0.30 < big.var() < 0.37  # uniform(-1, 1): variance 1/3


def test_idct_weight_tables_match_reference_constants(oracle, kat):
    for n in (64, 128, 256):
        ref = np.array(kat["idct_weights"][str(n)], dtype=np.float32)
        assert np.array_equal(oracle.idct_weights(n), ref)
    have = set()
    for n in (4, 8, 16, 32):
        have |= set(oracle.idct_weights(n).tolist())
    want = set(np.array(kat["idct_weights"]["idct32_muls_in_order"], dtype=np.float32).tolist())
    assert have == want


def test_rdct_scale_tables_match_reference_constants(oracle, kat):
    for n in (2, 4, 8, 16, 32):
        ref = np.array(kat["rdct_scales"][str(n)], dtype=np.float32)
        assert np.array_equal(oracle.rdct_scales(n), ref), n


def test_idct1d_vs_f64_definition(oracle_unfused, kat):
    """tests.rs:257-288.  The reference runs its 1-D tests on ScalarDescriptor only (mul_add = a * b + c,
    jxl_simd/src/scalar.rs:118-120): that is the oracle's unfused build, held to the exact tolerances."""
    for n, tol in kat["tolerances"]["idct1d"]:
        x = ref_draw(n, 1)[:, 0]
        got = oracle_unfused.idct1d(x.astype(np.float32))
        want = oracle_unfused.slow_idct1d(x)
        check_close(got, want, tol)


def test_idct1d_fused_build_stays_with_the_scalar_one(oracle, oracle_unfused, kat):
    """No reference test runs the 1-D kernels with fused multiply-adds; the fused build (what the GPU must equal)
    is tied to the pinned scalar build: same draw, difference within twice the shape's tolerance (two evaluations
    that are each within tol of the f64 definition)."""
    for n, tol in kat["tolerances"]["idct1d"]:
        x = ref_draw(n, 1)[:, 0].astype(np.float32)
        check_close(oracle.idct1d(x), oracle_unfused.idct1d(x), 2 * tol)


def test_rdct1d_vs_f64_definition(oracle_unfused):
    # tests.rs:185-244 (ScalarDescriptor, like the 1-D IDCT tests)
    for n, tol in ((2, 1e-6), (4, 1e-6), (8, 1e-6), (16, 5e-6), (32, 5e-6)):
        x = ref_draw(n, 1)[:, 0]
        got = oracle_unfused.rdct1d(x.astype(np.float32))
        slow = oracle_unfused.slow_dct1d(x)
        i = np.arange(n)
        scales = np.cos(i / (16 * n) * np.pi) * np.cos(i / (8 * n) * np.pi) * np.cos(i / (4 * n) * np.pi) * n
        check_close(got, slow / scales, tol)


def test_idct2d_all_shapes_vs_f64_definition(oracle_any, kat):
    shapes = kat["tolerances"]["idct2d"]
    assert len(shapes) == 22
    for rows, cols, tol in shapes:
        x = ref_draw(rows, cols)
        got = oracle_any.idct2d(x.astype(np.float32).reshape(-1), rows, cols)
        want = oracle_any.slow_idct2d(x)
        check_close(got, want, tol)


def test_rdct2d_all_shapes_vs_f64_definition(oracle_any, kat):
    shapes = kat["tolerances"]["rdct2d"]
    assert len(shapes) == 17
    for rows, cols, tol in shapes:
        x = ref_draw(rows, cols)
        got = oracle_any.rdct2d(x.astype(np.float32))
        want = oracle_any.slow_rdct2d(x)
        assert got.shape == want.shape == (min(rows, cols), max(rows, cols))
        check_close(got, want, tol)


def test_idct2d_layout_is_transpose_detecting(oracle):
    # a single horizontal-frequency coefficient must produce a pattern varying along x only
    for rows, cols in ((8, 8), (16, 8), (8, 16), (32, 32), (64, 32)):
        c = np.zeros(rows * cols, dtype=np.float32)
        # horizontal frequency u=1, vertical v=0
        if rows < cols:
            c[0 * cols + 1] = 1.0
        else:
            c[1 * rows + 0] = 1.0
        px = oracle.idct2d(c, rows, cols)
        assert np.allclose(px, px[0:1, :], atol=1e-6), (rows, cols)
        assert px[0, 0] > 0 > px[0, -1]


def test_default_dequant_tables_vs_libjxl_samples(oracle, kat):
    target = kat["dequant_default_samples"]
    idx = 0
    for t in range(27):
        tab = oracle.table_for_type[t]
        size = oracle.table_size[tab]
        table = oracle.library_dequant_table(tab)
        for c in range(3):
            for j in range(0, size, size // 10):
                assert abs(table[c * size + j] - target[idx]) < 1e-5, (t, c, j)
                idx += 1
    assert idx == len(target)


def test_dequant_table_sizes(oracle):
    assert sum(oracle.table_size) == 2056 * 64  # quant_weights.rs:1135


def test_natural_coeff_order_goldens(oracle, kat):
    assert oracle.natural_coeff_order(0).tolist() == kat["coeff_orders"]["COEFF_ORDER_1X1"]
    assert oracle.natural_coeff_order(7).tolist() == kat["coeff_orders"]["COEFF_ORDER_2X1"]
    for t in range(27):
        o = oracle.natural_coeff_order(t)
        assert sorted(o.tolist()) == list(range(o.size))  # a permutation
        cx, cy = oracle.covered_x[t], oracle.covered_y[t]
        # the first cx*cy entries are the LLF corner: min(cx,cy) rows x max cols, stride 8*max
        mx, mn = max(cx, cy), min(cx, cy)
        llf = sorted(o[: cx * cy].tolist())
        assert llf == sorted(y * 8 * mx + x for y in range(mn) for x in range(mx))


def test_gaborish_checkerboard(oracle_any, kat):
    g = kat["gaborish_checkerboard"]
    out = oracle_any.gaborish(np.array(g["input"], dtype=np.float32), g["w1"], g["w2"])
    assert np.abs(out - np.array(g["output"])).max() < g["tol"]


def test_squeeze_tendency_simd_form_equals_scalar_definition(oracle):
    rng = np.random.default_rng(5)
    L = oracle.lib
    for scale in (4, 300, 70000, 1 << 24):
        v = rng.integers(-scale, scale + 1, size=(20000, 3))
        for a, b, c in v:
            assert L.jxlo_smooth_tendency_i32(int(a), int(b), int(c)) == L.jxlo_smooth_tendency(int(a), int(b), int(c))


# ---------------------------------------------------------------- output stages (XYB -> sRGB u8)
def test_xyb_stage_srgb_primaries_known_answer(oracle_any, kat):
    """xyb.rs:289-312: three XYB pixels that are the sRGB primaries at intensity 255"""
    k = kat["output_stage"]
    p = oracle_any.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, k["intensity_target"])
    x, y, b = (np.array(r, dtype=np.float32) for r in k["srgb_primaries_input_xyb"])
    r, g, bb = oracle_any.xyb_to_linear(p, x, y, b)
    want = np.array(k["srgb_primaries_output_rgb"], dtype=np.float32)   # rows: R, G, B planes
    for got, w in zip((r, g, bb), want):
        assert np.abs(got - w).max() < k["srgb_primaries_tol"], (got, w)


def test_srgb_transfer_matches_pow_definition(oracle_any, kat):
    """tf.rs:601-611: the rational-polynomial sRGB curve vs the pow() definition, tol 1e-6; also odd symmetry"""
    k = kat["output_stage"]
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(0, 1, 20000), rng.uniform(0, 0.004, 2000), [0.0, 0.0031308, 1.0]]).astype(np.float32)
    got = oracle_any.linear_to_srgb(v)
    a = v.astype(np.float64)
    naive = np.where(a <= 0.0031308, a * 12.92, 1.055 * a ** (1 / 2.4) - 0.055)
    assert np.abs(got - naive).max() < k["srgb_tf_vs_pow_tol"] * 2   # naive here is f64; the reference compares f32 pow
    assert np.array_equal(oracle_any.linear_to_srgb(-v), -got)


def test_u8_conversion_dither_properties(oracle_any):
    """convert.rs:14-18: the dither table averages 0 and stays inside (-0.49219, 0.49219), so an exact
    code value k/255 converts to k for every position and channel; out-of-range input clamps"""
    for (x, y, c) in [(0, 0, 0), (31, 5, 1), (32, 40, 2), (1000, 999, 1)]:
        for k in (0, 1, 127, 128, 254, 255):
            assert oracle_any.f32_to_u8(k / 255.0, x, y, c) == k
        assert oracle_any.f32_to_u8(-3.0, x, y, c) == 0
        assert oracle_any.f32_to_u8(7.0, x, y, c) == 255
    # 16-bit conversion (convert.rs:743-761): clamp, scale, round; exact code values survive
    L = oracle_any.lib
    for k in (0, 1, 257, 32768, 65534, 65535):
        assert L.jxlo_f32_to_u16(k / 65535.0, 16) == k
    assert L.jxlo_f32_to_u16(-1.0, 16) == 0 and L.jxlo_f32_to_u16(3.0, 16) == 65535
    # a mid-grey half-step flips with the dither: both neighbours occur over a 32x32 period
    vals = {oracle_any.f32_to_u8(100.5 / 255.0, x, y, 0) for x in range(32) for y in range(32)}
    assert vals == {100, 101}


def test_tendency_clamps_equal_min_form_on_full_i32_range(oracle_any):
    """The device kernel (k_squeeze.hip) computes the reference's SIMD tendency (squeeze.rs:107-141) with its
    two parity clamps folded into x = min(x, 2|a-b|+1, 2|b-c|) and the sign applied as (x ^ s) - s.  Proved
    here against the oracle's line-by-line restatement, including wrapping extremes."""
    L = oracle_any.lib
    rng = np.random.default_rng(9)

    def wrap(x):
        return (x + 2**31) % 2**32 - 2**31

    def min_form(a, b, c):
        a_b, b_c, a_c = wrap(a - b), wrap(b - c), wrap(a - c)
        ab = wrap(-a_b) if a_b < 0 else a_b
        bc = wrap(-b_c) if b_c < 0 else b_c
        ac = wrap(-a_c) if a_c < 0 else a_c
        skip = b_c != 0 and a_b != 0 and (a_b ^ b_c) < 0
        x = wrap(wrap(2 + ac) + ((ab * 0x55555556) >> 32)) >> 2
        x = min(x, wrap((ab << 1) + 1), wrap(bc << 1))
        if skip:
            x = 0
        s = a_c >> 31
        return wrap((x ^ s) - s)

    special = [-2**31, -2**31 + 1, -2**30, -1, 0, 1, 2, 3, 2**30, 2**31 - 2, 2**31 - 1]
    triples = [(a, b, c) for a in special for b in special for c in special]
    for scale in (2**8, 2**20, 2**31 - 1):
        arr = rng.integers(-scale, scale, size=(3000, 3), dtype=np.int64)
        triples += [tuple(int(v) for v in t) for t in arr]
    for a, b, c in triples:
        assert min_form(a, b, c) == L.jxlo_smooth_tendency_i32(a, b, c), (a, b, c)


# ---------------------------------------------------------------- chroma-subsampled frames
def test_chroma_upsample_known_answers(oracle_any, kat):
    """the reference's own vectors, exact (render/stages/chroma_upsample.rs:200-236)"""
    k = kat["chroma_upsample"]
    row = np.array([k["input"]], np.float32)
    assert np.array_equal(oracle_any.chroma_upsample(row, True)[0], np.float32(k["expected"]))
    assert np.array_equal(oracle_any.chroma_upsample(row.T, False)[:, 0], np.float32(k["expected"]))
    # a constant plane stays constant, a single sample is replicated (mirror on both sides)
    assert np.array_equal(oracle_any.chroma_upsample(np.full((3, 5), 0.37, np.float32), True), np.full((3, 10), np.float32(0.37)))
    assert np.array_equal(oracle_any.chroma_upsample(np.array([[2.5]], np.float32), False), np.full((2, 1), np.float32(2.5)))


def test_ycbcr_stage_known_answer(oracle_any, kat):
    """render/stages/ycbcr.rs:126-152: the three sRGB primaries"""
    k = kat["ycbcr"]
    rgb = oracle_any.ycbcr_to_rgb(k["cb"], k["y"], k["cr"])
    for c in range(3):
        assert np.max(np.abs(rgb[c] - np.float32(k["expected_rgb"][c]))) <= k["tol"]
    # grey: Cb = Cr = 0 leaves R = G = B = Y + 128/255
    r, g, b = oracle_any.ycbcr_to_rgb([0.0], [0.25], [0.0])
    assert r[0] == g[0] == b[0] == np.float32(0.25) + np.float32(128.0) / np.float32(255.0)


@pytest.mark.parametrize("sub", [((1, 0, 1), (1, 0, 1)), ((1, 0, 1), (0, 0, 0)), ((0, 0, 0), (1, 0, 1)), ((1, 0, 0), (0, 0, 1))])
def test_subsampled_frame_is_the_444_decode_of_the_aligned_blocks(oracle, sub):
    """Structure of K1e (frame/group.rs:223-250, :485-504): with a constant LF image, a sub-sampled channel is
    the 4:4:4 reconstruction of the blocks aligned to its sampling, gathered and chroma-upsampled; the other
    channels are untouched."""
    import copy
    from jxl_rs_amd import synth
    from helpers import oracle_params_from, run_oracle_frame
    hs, vs = sub
    wl = synth.make_vardct(300, 270, mix=synth.MIX_8X8, seed=5, epf_iters=0, gab=False, lf_smoothing=False, hshift=hs, vshift=vs)
    for i, v in enumerate((700, 3, -40)):
        wl.lf_q[i][:] = v
    got, _ = run_oracle_frame(oracle, wl)
    wl0 = copy.copy(wl)
    wl0.opts = dict(wl.opts, hshift=(0, 0, 0), vshift=(0, 0, 0))
    p0 = oracle_params_from(oracle, wl0)
    p0.xsize_blocks, p0.ysize_blocks = wl.xblocks, wl.yblocks
    lf = [oracle.dequant_lf_channel(p0, 0, wl.lf_q[1]), oracle.dequant_lf_channel(p0, 1, wl.lf_q[0]),
          oracle.dequant_lf_channel(p0, 2, wl.lf_q[2])]
    full = [np.zeros((wl.yblocks * 8, wl.xblocks * 8), np.float32) for _ in range(3)]
    for g in range(wl.coeffs.shape[0]):
        oracle.decode_group(p0, g, wl.coeffs[g], wl.transform_map, wl.raw_quant, wl.ytox, wl.ytob, lf, wl.tables, full)
    for c in range(3):
        H, W = full[c].shape
        b = full[c].reshape(H // 8, 8, W // 8, 8)[::1 << vs[c], :, ::1 << hs[c], :]
        sub_plane = b.reshape(b.shape[0] * 8, b.shape[2] * 8)
        cw, ch = -(-wl.xsize // (1 << hs[c])), -(-wl.ysize // (1 << vs[c]))
        sub_plane = np.ascontiguousarray(sub_plane[:ch, :cw])
        if hs[c]:
            sub_plane = oracle.chroma_upsample(sub_plane, True)
        if vs[c]:
            sub_plane = oracle.chroma_upsample(sub_plane, False)
        want = sub_plane[:wl.ysize, :wl.xsize]
        assert np.array_equal(got[c].view(np.uint32), want.view(np.uint32)), f"channel {c}"


# ---------------------------------------------------------------- 2x / 4x / 8x upsampling
@pytest.mark.parametrize("n", [2, 4, 8])
def test_upsampling_matches_the_reference_tests_expectations(oracle_any, kat, n):
    """render/stages/upsample.rs:516-852: an impulse in a 7x7 image paints the kernel -- output pixel (i, j) of
    the 5n x 5n footprint equals weights[index_map[mapped_i][mapped_j]] clamped to [0, 1], with the reference's
    own triangular index tables and position mapping; the n-pixel border stays zero; the response is symmetric;
    a constant image stays constant."""
    k = kat["upsampling"]
    w = np.float32(k[f"weights{n}"])
    im = np.array(k["index_maps"][str(n)])
    img = np.zeros((7, 7), np.float32)
    img[3, 3] = 1.0
    out = oracle_any.upsample(n, img)
    assert out.shape == (7 * n, 7 * n)
    eps = k["impulse_tol"]
    assert np.abs(out[:n]).max() <= eps and np.abs(out[-n:]).max() <= eps
    assert np.abs(out[:, :n]).max() <= eps and np.abs(out[:, -n:]).max() <= eps
    half = n // 2
    for i in range(5 * n):
        for j in range(5 * n):
            if n == 2:  # upsample.rs:601-611
                di, ki, dj, kj = i % 2, i // 2, j % 2, j // 2
                mi = 4 - ki if di == 0 else ki
                mj = 4 - kj if dj == 0 else kj
            else:       # upsample.rs:683-693, :836-846
                mi = (4 - i // n + (i % half) * 5) if (i % n) < half else (i // n + (half - 1 - (i % half)) * 5)
                mj = (4 - j // n + (j % half) * 5) if (j % n) < half else (j // n + (half - 1 - (j % half)) * 5)
            want = min(max(w[im[mi][mj]], 0.0), 1.0)
            assert abs(out[n + i, n + j] - want) <= eps, (i, j)
    assert np.array_equal(out, out[::-1, ::-1])
    const = oracle_any.upsample(n, np.full((30, 17), 0.777, np.float32))
    assert np.abs(const - np.float32(0.777)).max() <= k["constant_tol"][str(n)]
    # the expanded kernels: every phase sums to 1 (the weights are a partition of unity)
    kern = oracle_any.upsample_kernels(n)
    assert np.abs(kern.reshape(n * n, 25).sum(axis=1) - 1.0).max() < 1e-5


# ---------------------------------------------------------------- noise synthesis
def test_xorshift128plus_golden(oracle_any, kat):
    """util/xorshift128plus.rs:77-735: 64 fills of 8 lanes after new_with_seed(12345), bit for bit"""
    k = kat["noise"]
    want = np.array([int(v, 16) for v in k["xorshift_golden"]], dtype=np.uint64).reshape(64, 8)
    assert np.array_equal(oracle_any.xorshift_golden(k["xorshift_seed"], 64), want)


def test_noise_stage_known_answers(oracle_any, kat):
    """render/stages/noise.rs:205-325: ConvolveNoise on a 2x2 ramp; AddNoise against goldens generated by libjxl"""
    k = kat["noise"]
    conv = oracle_any.noise_convolve(np.array(k["convolve_input"], np.float32).reshape(2, 2))
    assert np.max(np.abs(conv.ravel() - np.float32(k["convolve_expected"]))) <= k["convolve_tol"]
    a = (np.float32(k["add_input_start"]) + np.float32(k["add_input_step"]) * np.arange(64, dtype=np.float32)).reshape(8, 8)
    out = oracle_any.noise_add(k["add_lut"], 0.0, 1.0, [a, a, a], [a, a, a])  # ColorCorrelationParams::default()
    for c in range(3):
        assert np.max(np.abs(out[c].ravel() - np.float32(k["add_expected"][c]))) <= k["add_tol"]
    # strength: piecewise linear through the LUT, clamped (features/noise.rs:21-41)
    lut = [0.0, 0.1, 0.2, 0.4, 0.8, 1.6, 0.3, 0.5]
    assert oracle_any.noise_strength(lut, -1.0) == 0.0
    assert abs(oracle_any.noise_strength(lut, 0.5 / 6) - 0.05) < 1e-7
    assert oracle_any.noise_strength(lut, 4.5 / 6) == 1.0           # (0.8 + 1.6) / 2 clamps to 1
    assert abs(oracle_any.noise_strength(lut, 100.0) - 0.5) < 1e-7  # beyond the table: last entry


def test_noise_generation_structure(oracle):
    """frame/decode.rs:578-668: values in [1, 2); tiles are seeded by their corner, so a tile's content does not
    depend on the image around it as long as its own extent is the same; the frame indices reseed everything"""
    a = oracle.noise_generate(1, 2, 600, 300)
    assert all(p.min() >= 1.0 and p.max() < 2.0 for p in a)
    b = oracle.noise_generate(1, 2, 512, 256)
    for c in range(3):
        assert np.array_equal(a[c][:256, :512], b[c])
    c2 = oracle.noise_generate(1, 3, 600, 300)
    assert not np.array_equal(a[0], c2[0])
    assert abs(float(a[0].mean()) - 1.5) < 0.01


# ---------------------------------------------------------------- transfer functions (FromLinearStage)
def test_transfer_functions_against_their_definitions(oracle_any, kat):
    """color/tf.rs:575-800 checks each approximation against the defining formula on samples in [-1, 1]; the same
    comparisons (f64 definitions) with the reference's tolerances"""
    tol = kat["transfer_functions"]["tolerances"]
    x = np.linspace(-1, 1, 100001).astype(np.float32)
    a = np.abs(x.astype(np.float64))
    sign = np.sign(x)
    got = oracle_any.from_linear("srgb", [x, x, x])[1]
    assert np.abs(got - np.where(np.abs(x) <= np.float32(0.0031308), a * 12.92, 1.055 * a ** (1 / 2.4) - 0.055) * sign).max() <= tol["srgb_vs_pow"]
    got = oracle_any.from_linear("bt709", [x, x, x])[2]
    keep = np.abs(x) != np.float32(0.018)   # `0.018 > a` vs the definition's `a <= 0.018`: the one sample they disagree on
    want = np.where(np.abs(x) < np.float32(0.018), a * 4.5, 1.099 * a ** 0.45 - 0.099) * sign
    assert np.abs(got - want)[keep].max() <= tol["bt709_vs_pow"]
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    for it in (9900.0, 10000.0, 10100.0):
        got = oracle_any.from_linear("pq", [x, x, x], param=it)[0]
        xp = (a * it / 10000.0) ** m1
        want = ((c1 + xp * c2) / (1 + xp * c3)) ** m2 * sign
        # the SIMD form differs from the scalar one by up to 2e-5 near zero (tf.rs:690-706); away from it both meet 8e-7
        near0 = a < 1e-3
        assert np.abs(got - want)[~near0].max() <= tol["pq_vs_precise"]
        assert np.abs(got - want)[near0 & (a > 0)].max() <= tol["pq_simd_vs_scalar"]
    got = oracle_any.from_linear("hlg", [x, x, x], param=0.0)[0]   # exponent 0: OOTF skipped (|exp| < 0.1)
    A, C = 0.17883277, 0.5599107295
    B = 1 - 4 * A
    want = np.where(a <= 1 / 12, np.sqrt(3 * a), A * np.log(np.maximum(12 * a - B, 1e-30)) + C) * sign
    assert np.abs(got - want).max() <= tol["hlg_vs_precise"]
    xs = np.linspace(1e-3, 1, 4000).astype(np.float32)
    for g in (0.45, 1 / 2.2, 0.9):
        got = oracle_any.from_linear("gamma", [xs, xs, xs], param=g)[0]
        assert np.abs(got / xs.astype(np.float64) ** g - 1).max() <= tol["powf_rel"]
    # HLG inverse OOTF: mult = mixed^exponent on the luminance mix
    r, g_, b = [np.float32([v]) for v in (0.4, 0.3, 0.2)]
    lum = (0.2627, 0.678, 0.0593)
    e = -0.1667
    out = oracle_any.from_linear("hlg", [r, g_, b], param=e, lum=lum)
    mixed = 0.4 * lum[0] + 0.3 * lum[1] + 0.2 * lum[2]
    sc = [v * mixed ** e for v in (0.4, 0.3, 0.2)]
    want = [np.sqrt(3 * v) if v <= 1 / 12 else A * np.log(12 * v - B) + C for v in sc]
    assert max(abs(float(out[i][0]) - want[i]) for i in range(3)) < 2e-5


# ---------------------------------------------------------------- smooth unsqueeze (progressive previews)
# The reference's own tests of convolve_2d_simd / convolve_1d_simd (modular/transforms/squeeze.rs:1243-1319, run on
# ScalarDescriptor -> the unfused build, truncating convert).
def test_smooth_convolve_constant_input_is_identity(oracle_any):
    for val in (-1000.0, -1.0, 0.0, 1.0, 42.0, 255.0, 10000.0):
        n = np.full(25, val, dtype=np.float32)
        assert (oracle_any.smooth_convolve(n, True) == int(val)).all(), val
        assert (oracle_any.smooth_convolve(n, False) == int(val)).all(), val


def test_smooth_convolve_2d_symmetry(oracle_any):
    def imp(k):
        n = np.zeros(25, dtype=np.float32)
        n[k] = 10000.0
        return oracle_any.smooth_convolve(n, True)
    o, h, v = imp(6), imp(8), imp(16)
    assert (o[0], o[1], o[2], o[3]) == (h[1], h[0], h[3], h[2])
    assert (o[0], o[1], o[2], o[3]) == (v[2], v[3], v[0], v[1])
    assert len(set(o.tolist())) > 1  # the impulse response is not flat: the checks above are not vacuous


def test_smooth_convolve_1d_symmetry(oracle_any):
    def imp(k):
        n = np.zeros(25, dtype=np.float32)
        n[k] = 10000.0
        return oracle_any.smooth_convolve(n, False)
    a, b = imp(7), imp(17)
    assert (a == b).all()
    c, d = imp(6), imp(8)
    assert c[0] == d[1] and c[1] == d[0] and c[0] != c[1]


def _smooth_numpy(kind, avg, out_w, out_h, x0, y0, conv):
    """Independent restatement of the three sliding-window drivers (squeeze.rs:908-1225) on a padded copy: rows
    mirror ('symmetric'), columns clamp ('edge'), exactly what load_row_to_scratch (step.rs:372-420) produces."""
    fx, fy = kind != 1, kind != 0
    if (out_w // 2 if fx else out_w) == 0 or (out_h // 2 if fy else out_h) == 0:
        return np.zeros((out_h, out_w), dtype=np.int32)
    P = 2 + max(avg.shape) + out_w + out_h  # generous: np.pad handles pads longer than the array for these modes
    pad = np.pad(np.pad(avg, ((P, P), (0, 0)), mode="symmetric") if avg.shape[0] > 1
                 else np.repeat(avg, 2 * P + 1, axis=0), ((0, 0), (P, P)), mode="edge").astype(np.float32)
    out = np.zeros((out_h, out_w), dtype=np.int32)
    cx0, cy0 = (x0 // 2 if fx else x0), (y0 // 2 if fy else y0)
    for iy in range((out_h + 1) // 2 if fy else out_h):
        for ix in range((out_w + 1) // 2 if fx else out_w):
            win = pad[P + cy0 + iy - 2:P + cy0 + iy + 3, P + cx0 + ix - 2:P + cx0 + ix + 3]
            o = conv((win.T if kind == 1 else win).reshape(25), kind == 2)
            for k, val in enumerate(o):
                ox = 2 * ix + (k & 1) if fx else ix
                oy = (2 * iy + (k >> 1 if kind == 2 else k)) if fy else iy
                if ox < out_w and oy < out_h:
                    out[oy, ox] = val
    return out


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_smooth_unsqueeze_window_walk_vs_padded_restatement(oracle_any, kind):
    rng = np.random.default_rng(40 + kind)
    fx, fy = kind != 1, kind != 0
    for (w, h) in [(1, 1), (2, 2), (3, 1), (1, 3), (5, 4), (8, 8), (9, 7), (17, 2), (2, 13), (16, 11)]:
        aw, ah = ((w + 1) // 2 if fx else w), ((h + 1) // 2 if fy else h)
        avg = rng.integers(-2000, 2000, size=(ah, aw)).astype(np.int32)
        want = _smooth_numpy(kind, avg, w, h, 0, 0, oracle_any.smooth_convolve)
        got = oracle_any.smooth_unsqueeze(kind, avg, w, h)
        assert (got == want).all(), (kind, w, h)
    # a grid tile of a larger channel: the rectangle's origin moves the window, the clamps stay the channel's
    W, H = 37, 29
    avg = rng.integers(-2000, 2000, size=((H + 1) // 2 if fy else H, (W + 1) // 2 if fx else W)).astype(np.int32)
    whole = oracle_any.smooth_unsqueeze(kind, avg, W, H)
    for (x0, y0, w, h) in [(0, 0, 16, 16), (16, 0, 16, 16), (32, 16, 5, 13), (16, 16, 16, 13)]:
        tile = oracle_any.smooth_unsqueeze(kind, avg, w, h, x0, y0)
        assert (tile == whole[y0:y0 + h, x0:x0 + w]).all(), (kind, x0, y0)
        assert (tile == _smooth_numpy(kind, avg, w, h, x0, y0, oracle_any.smooth_convolve)).all()


def test_smooth_unsqueeze_x86_convert_differs_from_the_other_backends(oracle):
    """cvtps after the +-0.5 (x86 back-ends) rounds |sum| up to the NEXT integer whenever frac(|sum|) is in (0, 0.5):
    the back-ends disagree by one level on about half the samples; the product implements the truncating form."""
    rng = np.random.default_rng(44)
    avg = rng.integers(-500, 500, size=(32, 32)).astype(np.int32)
    a = oracle.smooth_unsqueeze(2, avg, 64, 64)
    b = oracle.smooth_unsqueeze(2, avg, 64, 64, cvt_rne=True)
    d = np.abs(a.astype(np.int64) - b)
    assert d.max() == 1 and 0.2 < (d != 0).mean() < 0.8
    assert (np.abs(b) >= np.abs(a)).all()


# ---------------------------------------------------------------- the self-correcting ("Weighted") predictor
def test_weighted_predictor_libjxl_golden(oracle):
    """predict_and_update_errors (modular/predict.rs:561-592): an LCG drives header, positions, neighbours and the
    corrected values; the four expected (prediction, property) pairs were generated with libjxl's predictor."""
    import ctypes as C

    class Lcg:
        def __init__(self):
            self.out = 1

        def next(self):
            self.out = self.out * 48271 % 0x7FFFFFFF
            return self.out
    rng = Lcg()
    header = [rng.next() % 32 for _ in range(7)] + [rng.next() % 16 for _ in range(4)]  # p1c p2c p3ca..e, w0..w3
    L = oracle.lib
    hdr = (C.c_uint32 * 11)(*header)
    xsize = ysize = 8
    st = L.jxlo_wp_new(hdr, xsize)
    got = []
    for _ in range(4):
        x, y = rng.next() % xsize, rng.next() % ysize
        top, left, topright, topleft, toptop = [rng.next() % 256 for _ in range(5)]
        nb = (C.c_int32 * 5)(top, left, topright, topleft, toptop)
        prop = C.c_int32()
        pred = L.jxlo_wp_predict(st, x, y, nb, C.byref(prop))
        L.jxlo_wp_update(st, rng.next() % 256, x, y)
        got.append((pred, prop.value))
    L.jxlo_wp_free(st)
    assert got == [(135, 0), (110, -60), (165, 0), (153, -60)]


def test_weighted_predictor_reproduces_flat_and_ramp_images(oracle):
    """Sanity on whole images through the palette step: with every index a delta entry of value 0 the output is the
    predictor's own extrapolation -- a constant image stays constant, and the first pixel is 0 + entry."""
    w, h = 19, 11
    pal = np.zeros((1, 1), np.int32)           # one delta entry: 0
    idx = np.zeros((h, w), np.int32)
    hdr = (16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12)  # the header's defaults (headers/modular.rs:16-66)
    out = oracle.palette_delta_wp(idx, pal, 0, 1, 1, 8, hdr)
    assert (out == 0).all()
    pal2 = np.array([[0, 37]], np.int32)       # entry 1 is a colour: absolute 37
    idx2 = np.zeros((h, w), np.int32)
    idx2[0, 0] = 1
    out2 = oracle.palette_delta_wp(idx2, pal2, 1, 1, 1, 8, hdr)
    assert out2[0, 0, 0] == 37 and (out2[0, 0, 1:] == 37).all()  # West-like extrapolation along the first row


# ---------------------------------------------------------------- the unsqueeze step as the device computes it
def _unsqueeze_step_d_state(avg, res, nx, d):
    """numpy transcription of unsqueeze_step (jxl_rs_amd/csrc/k_squeeze.hip): the recurrence on d = prev - avg with the
    sign of avg - next applied up front; wrapping i32 arithmetic as on the device"""
    i32, u32 = np.int32, np.uint32
    with np.errstate(over="ignore"):
        b_c = (avg.astype(u32) - nx.astype(u32)).astype(i32)
        sm = (b_c >> 31).astype(u32)
        nsm = b_c.astype(u32) >> u32(31)
        bc = (b_c.astype(u32) ^ sm) + nsm
        k2, u, rs = bc + u32(2), bc << u32(1), res.astype(u32) + nsm
        e = ((d.astype(u32) ^ sm) + nsm).astype(i32)
        e3 = ((e.astype(np.int64) * 0x55555556) >> 32).astype(i32)
        s = (e.astype(u32) + e3.astype(u32) + k2).astype(i32) >> 2
        t1 = ((e.astype(u32) << u32(1)) + u32(1)).astype(i32)
        x = np.maximum(np.minimum(np.minimum(s, t1), u.astype(i32)), 0)
        diff = ((x.astype(u32) ^ sm) + rs).astype(i32)
        h = (diff.astype(u32) + (diff >> 31).astype(u32) + u32(1)).astype(i32) >> 1
        d2 = (b_c.astype(u32) - h.astype(u32)).astype(i32)
        b = (avg.astype(u32) - h.astype(u32)).astype(i32)
        a = (b.astype(u32) + diff.astype(u32)).astype(i32)
    return a, b, d2


@pytest.mark.parametrize("bits", [3, 9, 17, 24, 28])
def test_unsqueeze_d_state_restatement_equals_the_reference_forms(oracle, bits):
    """The device runs the squeeze recurrence in a restated form with half the dependent instructions.  It must equal
    the reference's scalar i64 definition (= the oracle) wherever the reference is well defined, i.e. wherever its own
    i32 SIMD form and its i64 scalar form agree: step operands below 2^29 (beyond that the two reference forms differ
    from EACH OTHER on ~10 % of random inputs at 2^30 and ~40 % at 2^31, so there is nothing to be equal to).  Whole
    lines are driven with inputs up to 2^28: the outputs of a step can exceed its inputs."""
    rng = np.random.default_rng(bits)
    lim = 1 << bits
    h, w = 64, 257
    avg = rng.integers(-lim, lim, size=(h, (w + 1) // 2), dtype=np.int64).astype(np.int32)
    res = rng.integers(-lim, lim, size=(h, w // 2), dtype=np.int64).astype(np.int32)
    avg[1::3, 1:] = avg[1::3, :-1] + rng.integers(-3, 4, size=avg[1::3, 1:].shape)  # near-flat runs: small tendencies
    res[::2] = rng.integers(-4, 5, size=res[::2].shape)
    out = np.zeros((h, w), np.int32)
    d = np.zeros(h, np.int32)
    nr = w // 2
    for x in range(nr):
        cur = avg[:, x]
        nx = avg[:, x + 1] if x + 1 < avg.shape[1] else cur
        a, b, d = _unsqueeze_step_d_state(cur, res[:, x], nx, d)
        out[:, 2 * x], out[:, 2 * x + 1] = a, b
    out[:, w - 1] = avg[:, nr]
    assert np.array_equal(out, oracle.unsqueeze_h(avg, res, w))


def _device_form_h(avg, res, w):
    """a whole horizontal step with the device's restated recurrence (numpy transcription above)"""
    h = avg.shape[0]
    out, d, nr = np.zeros((h, w), np.int32), np.zeros(h, np.int32), w // 2
    for x in range(nr):
        cur = avg[:, x]
        nx = avg[:, x + 1] if x + 1 < avg.shape[1] else cur
        a, b, d = _unsqueeze_step_d_state(cur, res[:, x], nx, d)
        out[:, 2 * x], out[:, 2 * x + 1] = a, b
    if w & 1:
        out[:, w - 1] = avg[:, nr]
    return out


def test_squeeze_forms_agree_up_to_2_28_and_the_reference_splits_beyond(oracle):
    """The input bound include/jxl_hip.h documents for the squeeze entry points.  The reference holds TWO forms of the
    step -- `unsqueeze_scalar` on i64 (squeeze.rs:187-194) for remainder columns / rows and the wrapping i32
    `unsqueeze_impl` + `smooth_tendency_impl` (squeeze.rs:107-185) for everything its SIMD back-end covers.  Both are
    restated in the oracle.  For samples in [-2^28, 2^28) the two agree with each other and with the device's form on
    every sample; from 2^29 on the reference's own forms give different results for the same input (which one a
    sample gets depends on its position inside the SIMD tiling), so there is no reference value to equal."""
    h, w = 128, 257
    for bits in (8, 20, 27, 28):
        rng = np.random.default_rng(100 + bits)
        lim = 1 << bits
        avg = rng.integers(-lim, lim, size=(h, (w + 1) // 2), dtype=np.int64).astype(np.int32)
        res = rng.integers(-lim, lim, size=(h, w // 2), dtype=np.int64).astype(np.int32)
        sc = oracle.unsqueeze_h(avg, res, w)
        si = oracle.unsqueeze_h(avg, res, w, simd_form=True)
        assert np.array_equal(sc, si), bits
        assert np.array_equal(_device_form_h(avg, res, w), sc), bits
        a2 = np.ascontiguousarray(avg.T)
        r2 = np.ascontiguousarray(res.T)
        assert np.array_equal(oracle.unsqueeze_v(a2, r2, w), sc.T)
        assert np.array_equal(oracle.unsqueeze_v(a2, r2, w, simd_form=True), sc.T)
    for bits, least in ((30, 0.05), (31, 0.3)):
        rng = np.random.default_rng(100 + bits)
        lim = 1 << bits
        avg = rng.integers(-lim, lim, size=(h, (w + 1) // 2), dtype=np.int64).astype(np.int32)
        res = rng.integers(-lim, lim, size=(h, w // 2), dtype=np.int64).astype(np.int32)
        split = np.mean(oracle.unsqueeze_h(avg, res, w) != oracle.unsqueeze_h(avg, res, w, simd_form=True))
        assert split > least, (bits, split)


# adjust_quant_bias (group.rs:85-96) restated in numpy float32 from the reference's own operations: the I32Vec abs of
# every back-end wraps (jxl_simd scalar.rs:247 `Wrapping(self.0.abs())` in a release build, _mm_abs_epi32 sse42.rs:756,
# _mm256_abs_epi32 avx.rs:821, _mm512_abs_epi32 avx512.rs:1004, vabsq_s32 neon.rs:635), so `2 > abs(i32::MIN)` holds
# and i32::MIN takes the bias branch.
def _ref_adjust_quant_bias(q, c, biases):
    q = np.asarray(q, dtype=np.int32)
    b = np.asarray(biases, dtype=np.float32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        quant = q.astype(np.float32)
        adjusted = quant - b[3] / quant
        return np.where(np.int32(2) > np.abs(q), quant * b[c], adjusted).astype(np.float32)


_QB_EDGES = np.array([-2**31, -2**31 + 1, -2, -1, 0, 1, 2, 2**31 - 1], dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("biases", [
    (1.0 - 0.05465007, 1.0 - 0.07005449, 1.0 - 0.049935103, 0.145),  # the library default (headers/transform_data.rs)
    (0.5, 1e-6, 1e6, -3.25),
    (0.0, -0.75, 65504.0, 4.0),
], ids=["default", "custom_a", "custom_b"])
def test_oracle_adjust_quant_bias_at_i32_edges(oracle_any, biases):
    """The oracle's dequantised value at q in {MIN, MIN+1, -2, -1, 0, 1, 2, MAX} equals the reference expression
    bit for bit -- i32::MIN included, where a plain `-q` is undefined behaviour in C and a non-wrapping |q| picks
    the other branch (the adjusted value, -2.1474836e9 instead of MIN * bias_c)."""
    assert np.abs(np.int32(-2**31)) == np.int32(-2**31)  # numpy's abs wraps like the reference's
    for c in range(3):
        got = oracle_any.adjust_quant_bias(_QB_EDGES, c, biases)
        want = _ref_adjust_quant_bias(_QB_EDGES, c, biases)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c, got, want)
        # MIN takes the bias branch: exactly (f32)MIN * bias_c
        assert got[0].view(np.uint32) == (np.float32(-2**31) * np.float32(biases[c])).view(np.uint32)


def test_oracle_adjust_quant_bias_wide_sweep(oracle):
    """Every |q| < 2^12 and a random sample of the whole i32 range, default biases, all three channels."""
    rng = np.random.default_rng(85)
    q = np.concatenate([np.arange(-4096, 4097), rng.integers(-2**31, 2**31, size=1 << 16, dtype=np.int64),
                        _QB_EDGES]).astype(np.int32)
    b = (0.94534993, 0.9299455, 0.9500649, 0.145)
    for c in range(3):
        assert np.array_equal(oracle.adjust_quant_bias(q, c, b).view(np.uint32),
                              _ref_adjust_quant_bias(q, c, b).view(np.uint32)), c
