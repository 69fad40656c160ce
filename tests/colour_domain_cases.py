"""Input planes and parameter sets that walk the colour stage (csrc/color_device.h: XybStage, then one of six transfer
curves, or YCbCr, or nothing) over the whole binary32 domain.  Plain numpy, deterministic, no GPU: shared by
tests/test_colour_domain_cpu.py, which proves on the oracle that the inputs do what they are meant to, and
tests/test_gpu_colour_domain.py, which holds the device to the oracle on them.

Every set of planes is (X, Y, B) as float32 [h, WIDTH]; WIDTH is even but no multiple of 4, so the four-pixel lanes of
every consumer run a row tail.  A set's pad (the last row's remainder) repeats its own first values: it adds no class."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH = 74          # 18 four-pixel lanes and a tail of 2; 18 944 = 256 rows of it
LUM = (0.2627, 0.678, 0.0593)

# the branch points of the curves, as the f32 constants the code compares against (color/tf.rs): sRGB, BT.709, PQ's
# small-value polynomial, HLG's square-root part, and 1.0 (the top of the nominal range; the integer formats' clamp)
THRESHOLDS = (np.float32(0.0031308), np.float32(0.018), np.float32(1e-4), np.float32(1.0) / np.float32(12.0),
              np.float32(1.0))
THRESHOLD_ULPS = 64


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _rows(values, width=WIDTH):
    """the values as [h, width], the last row filled up with the first values again"""
    values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    n = -(-values.size // width) * width
    return np.resize(values.view(np.uint32), n).view(np.float32).reshape(-1, width)  # (on bits: NaN payloads survive)


def _permuted(values, seed):
    """a fixed permutation, on the bit patterns"""
    bits = np.ascontiguousarray(values, dtype=np.float32).reshape(-1).view(np.uint32)
    return bits[np.random.default_rng(seed).permutation(bits.size)].view(np.float32)


def mantissas(n_random, seed):
    """0, 1, all ones, the top bit alone, then n_random fixed random ones"""
    rnd = np.random.default_rng(seed).integers(2, 0x7fffff, size=n_random, dtype=np.uint32)
    return np.concatenate([np.array([0, 1, 0x7fffff, 0x400000], dtype=np.uint32), rnd])


def sweep_values(exponents, mant):
    """every biased exponent x every mantissa x both signs, positive half first"""
    e = np.asarray(exponents, dtype=np.uint32)[:, None] << np.uint32(23)
    pos = (e | np.asarray(mant, dtype=np.uint32)[None, :]).reshape(-1)
    return _f32(np.concatenate([pos, pos | np.uint32(0x80000000)]))


def main_values():
    """biased exponents 0..147 (zero, the denormals, everything below 2^21) x 64 mantissas x both signs: 18 944 values.
    Past 2^21 the cube of XybStage and the degree-4 polynomials in sqrt|x| overflow and a plane is mostly NaN: that
    part of the domain is the tail's."""
    return sweep_values(np.arange(0, 148), mantissas(60, 0xC01))


def main_planes():
    """Y walks the sweep in order; X and B are fixed permutations of the same values"""
    y = main_values()
    return [_rows(_permuted(y, 0xC02)), _rows(y), _rows(_permuted(y, 0xC03))]


NAN_BITS = (0x7fc00000, 0x7fc00001, 0x7fffffff,   # quiet: the default NaN, a low payload bit, all ones
            0x7f800001, 0x7fa00000, 0x7fbfffff)   # signalling: the smallest, the second mantissa bit, all but the quiet bit


def special_values():
    """+-inf, then the quiet and signalling NaN patterns of both signs"""
    pos = np.array((0x7f800000,) + NAN_BITS, dtype=np.uint32)
    return _f32(np.concatenate([pos, pos | np.uint32(0x80000000)]))


def tail_values():
    """biased exponents 148..254 (2^21 up to the largest finite value) x 5 mantissas x both signs, +-inf and the NaNs"""
    return np.concatenate([sweep_values(np.arange(148, 255), mantissas(1, 0xC04)), special_values()])


def tail_planes():
    """The tail values in all three channels of a pixel (X and B permuted), then in ONE channel of a pixel only, the
    other two holding 0 / 0.25 / 0.5 in turn: what one channel's inf or NaN does to the other two (0 * inf in the matrix
    of XybStage, the luminance mix of the HLG OOTF) shows there."""
    v = tail_values()
    alone = np.concatenate([sweep_values(np.arange(148, 255), [0]), special_values()])
    calm = np.float32([0.0, 0.25, 0.5])[np.arange(alone.size) % 3]
    chan = [[_permuted(v, 0xC05)], [v], [_permuted(v, 0xC06)]]
    for c in range(3):
        for k in range(3):
            chan[k].append(alone if k == c else calm)
    return [_rows(np.concatenate(p)) for p in chan]


def _neighbours(centre, n):
    """the 2 n + 1 floats around a positive normal `centre`, ascending"""
    b = np.float32(centre).view(np.uint32).astype(np.int64)
    return _f32((b + np.arange(-n, n + 1)).astype(np.uint32))


def threshold_segments():
    """(threshold, values): float32(cbrt(t)) and its +-64 neighbours in ulps.  With IDENTITY_XYB and X = 0 the linear
    value of a sample is its cube (two f32 products), so these straddle t"""
    return [(t, _neighbours(np.float32(np.cbrt(np.float64(t))), THRESHOLD_ULPS)) for t in THRESHOLDS]


def threshold_planes():
    """X = 0, Y = the threshold segments and their negatives, +-0, the smallest and the largest denormal of both signs;
    B = Y reversed.  Returns (planes, slices): slices[i] is where THRESHOLDS[i]'s positive segment lies in Y.ravel()"""
    segs = [v for _, v in threshold_segments()]
    slices, at = [], 0
    for v in segs:
        slices.append(slice(at, at + v.size))
        at += v.size
    edge = _f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff])
    y = np.concatenate(segs + [-np.concatenate(segs), edge])
    planes = [_rows(np.zeros_like(y)), _rows(y), _rows(y[::-1])]
    return planes, slices


def display_planes(h=48):
    """uniform Y in [0, 1], X in [-0.03, 0.03], B in [0, 1]: many distinct in-range code values for the integer formats"""
    rng = np.random.default_rng(0xC07)
    shape = (h, WIDTH)
    return [rng.uniform(-0.03, 0.03, shape).astype(np.float32), rng.uniform(0.0, 1.0, shape).astype(np.float32),
            rng.uniform(0.0, 1.0, shape).astype(np.float32)]


# ---- parameters
IDENTITY_XYB = "identity"


def default_opsin():
    """(inverse matrix, bias) of tests/golden/reference_kat.json"""
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        k = json.load(f)["output_stage"]
    return k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3


XYB_SETS = (IDENTITY_XYB, "default_255", "default_80", "default_10000")


def xyb_param_sets(oracle):
    """name -> the 16 floats of the XybStage parameters.  "identity": identity matrix, zero biases, target 255 (then
    r = g = Y^3 with X = 0 and b = B^3); the default matrix and bias at intensity targets 255, 80 and 10000"""
    m, b = default_opsin()
    out = {IDENTITY_XYB: oracle.xyb_params(np.eye(3, dtype=np.float32).reshape(-1), [0.0, 0.0, 0.0], 255.0)}
    for target in (255.0, 80.0, 10000.0):
        out["default_%d" % target] = oracle.xyb_params(m, b, target)
    return out


# (id, colour kind, transfer, tf_param): PQ's parameter is the intensity target, HLG's the OOTF exponent (|e| < 0.1 skips
# the OOTF: 0.1 and -0.1 run it, 0.0999 and 0.05 do not), gamma's the exponent applied to the linear value
CURVES = [("linear", "xyb", "linear", 0.0), ("srgb", "xyb", "srgb", 0.0), ("bt709", "xyb", "bt709", 0.0),
          ("pq_10000", "xyb", "pq", 10000.0), ("pq_4000", "xyb", "pq", 4000.0), ("pq_255", "xyb", "pq", 255.0),
          ("hlg_-0.1667", "xyb", "hlg", -0.1667), ("hlg_0.2", "xyb", "hlg", 0.2), ("hlg_0.1", "xyb", "hlg", 0.1),
          ("hlg_-0.1", "xyb", "hlg", -0.1), ("hlg_0.0999", "xyb", "hlg", 0.0999), ("hlg_0.05", "xyb", "hlg", 0.05),
          ("gamma_0.4545", "xyb", "gamma", 0.45454545), ("gamma_1/2.6", "xyb", "gamma", 1.0 / 2.6),
          ("gamma_1", "xyb", "gamma", 1.0), ("gamma_2.4", "xyb", "gamma", 2.4),
          ("ycbcr", "ycbcr", "linear", 0.0), ("none", "none", "linear", 0.0)]
CURVE_IDS = [c[0] for c in CURVES]
# one parameter per curve, for the consumers where the dispatch and the conversion behind it are the subject
ONE_EACH = ["linear", "srgb", "bt709", "pq_4000", "hlg_0.2", "gamma_2.4", "ycbcr", "none"]


def curve(name):
    return CURVES[CURVE_IDS.index(name)]


def colour_tuples(oracle, name, sets=None):
    """[(label, colour)] with `colour` in the form save_ref.colour_stage takes: one per XYB parameter set (all of them, or
    those named) for an XYB curve, one for YCbCr and for none"""
    _, kind, transfer, param = curve(name)
    if kind != "xyb":
        return [(name, (kind,))]
    params = xyb_param_sets(oracle)
    return [(f"{name} {k}", ("xyb", transfer, params[k], param, LUM)) for k in (sets or params)]


def colour_cases(sets=XYB_SETS):
    """[(curve, XYB set or None)]: every curve with each of `sets`, YCbCr and none once; ids via case_id"""
    return [(c[0], k) for c in CURVES for k in (sets if c[1] == "xyb" else (None,))]


def case_id(case):
    return case[0] if case[1] is None else f"{case[0]}-{case[1]}"


def colour_of(oracle, case):
    """(label, colour) of one of colour_cases()"""
    return colour_tuples(oracle, case[0], None if case[1] is None else [case[1]])[0]


def is_nan_bits(bits):
    """which samples of an f32 (uint32) or f16 (uint16) bit image are NaN"""
    bits = np.asarray(bits)
    if bits.dtype == np.uint16:
        return (bits & np.uint16(0x7fff)) > np.uint16(0x7c00)
    assert bits.dtype == np.uint32, bits.dtype
    return (bits & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)


def float_bits_mismatch(got, want):
    """THE COMPARISON RULE for float outputs, on bit images (uint32 of f32, uint16 of f16) -> bool mask of samples that
    break it.  Where the wanted value is not NaN the bits are equal, the sign of zero and of inf included; where it is
    NaN the device value is NaN.  A NaN's payload and sign are free: x86 and the GPU make different default NaNs
    (inf - inf is 0xffc00000 on x86, 0x7fc00000 on the GPU) and pick different operands' payloads, and the reference's
    own scalar and SIMD back ends differ from each other in the same way.  Nothing is masked out.

    One input class is recorded where WHICH NaN an operation hands on reaches a number: fma(0, +-inf, NaN) in XybStage's
    matrix (a zero matrix entry, a channel overflowed to inf, another channel a NaN) gives the addend on an x86 FMA, a
    fresh default NaN in v_fma_f32, and in the reference's scalar (a * b) + c whichever NaN the compiler put first; gamma
    and HLG then build a number from that NaN's bits (fast_log2f works on the bit pattern, copysign takes the sign).
    The rule is not widened for it: the device follows the FMA back end there (opsin_fma, csrc/color_device.h)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    wn = is_nan_bits(want)
    return np.where(wn, ~is_nan_bits(got), got != want)
