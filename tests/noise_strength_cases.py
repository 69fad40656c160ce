"""Planes that take Noise::strength (jxl/src/features/noise.rs:21-41; noise_strength of csrc/k_noise.hip) through every
interval of its piecewise-linear LUT, its saturation branch and both clamps of its result -- from the in_g = Y - X
side and from the in_r = Y + X side of AddNoiseStage separately.

strength(v) looks up scaled = max(0, 6 v): interval floor(scaled) of 0..6, or interval 6 at fraction 1 once
scaled >= 7.  uniform(-0.2, 0.9) planes reach intervals 0..5 on one side and 0..3 on the other, and a LUT drawn from
[0, 1] never clamps; the upper half of the kernel's select chain ran unchecked.

A sample is a pair (X, Y): (-v, v) puts v on the in_g side exactly (in_g / 2 = v, in_r / 2 = 0), (v, v) on the in_r
side.  `interval` is the model of where a value lands; tests/test_noise_strength_cases_cpu.py holds it to
jxlo_noise_strength.  It never makes expected pixels.  Importing this file needs neither a GPU nor the oracle."""
import numpy as np

F = np.float32
K_SCALE = F(6.0)

LUTS = {
    "monotone": F([0.0, 0.1, 0.2, 0.35, 0.5, 0.65, 0.8, 1.0]),
    "primes": F([2, 3, 5, 7, 11, 13, 17, 19]) / F(64),                  # distinct everywhere: a wrong index cannot alias
    "clamps": F([1.5, -0.5, 2.0, -1.0, 1.25, -0.25, 3.0, -2.0]),        # every interval crosses 0 and 1
    "zero": np.zeros(8, F),                                            # AddNoiseStage leaves the planes alone
    "last_only": F([0, 0, 0, 0, 0, 0, 0, 0.75]),                        # only interval 6 and the saturation branch act
}


def interval(v):
    """the model: (index of the interval, fraction, saturated) of strength(v), binary32 in the reference's order"""
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        sv = v * K_SCALE
        scaled = np.where(sv > 0, sv, F(0.0))          # f32::max(0.0, x): a NaN gives 0
        fl = np.floor(scaled)
        sat = scaled >= K_SCALE + F(1.0)
        fi = np.where(sat, K_SCALE, fl).astype(np.int32)
        frac = np.where(sat, F(1.0), scaled - fl).astype(F)
    return fi, frac, sat


def unclamped(lut, v):
    """the model's value ahead of the clamp: tells whether a clamp fires (never an expected pixel)"""
    fi, frac, _ = interval(v)
    lut = np.asarray(lut, dtype=F)
    with np.errstate(all="ignore"):
        return (lut[fi + 1] - lut[fi]) * frac + lut[fi]


def _on_integer(k):
    """a v with 6 v == k exactly in binary32"""
    v = F(k) / K_SCALE
    for cand in (v, np.nextafter(v, F(np.inf)), np.nextafter(v, F(-np.inf))):
        if cand * K_SCALE == F(k):
            return cand
    raise AssertionError(k)


def _just_below(k):
    """the largest v whose 6 v is below k (6 v moves in steps of up to six ulps of v: not every binary32 below k is a
    product)"""
    v = _on_integer(k)
    while v * K_SCALE >= F(k):
        v = np.nextafter(v, F(-np.inf))
    return v


def values():
    """the values of v = in / 2 every side is taken through, in a fixed order"""
    rng = np.random.default_rng(0x4E53)
    out = []
    for k in range(7):                                  # inside each interval: 24 fractions
        out += [F((k + f) / 6.0) for f in rng.uniform(0.02, 0.98, 24)]
    out += [_on_integer(k) for k in range(8)]           # exactly on each integer 0..7
    out += [_just_below(k) for k in range(1, 8)]        # the last value below each, 7 among them
    out += [np.nextafter(_on_integer(7), F(np.inf))]    # the first value above 7
    out += [F(s / 6.0) for s in rng.uniform(7.0, 50.0, 20)]                              # above 7
    out += [F(2.0), F(100.0), F(65504.0), F(1e30), F(3.0e38), F(np.inf)]                 # (6 v overflows at 3e38)
    out += [F(-s) for s in rng.uniform(0.001, 2.0, 16)] + [F(-1e30), F(-np.inf)]         # below 0
    out += [F(-0.0), F(1e-42), F(-1e-42)]
    out += [F(np.nan)]
    return np.asarray(out, dtype=F)


def samples():
    """(X, Y, side): every value on the in_g side, then on the in_r side; side 0 = in_g, 1 = in_r"""
    v = values()
    x = np.concatenate([-v, v])
    y = np.concatenate([v, v])
    return x, y, np.concatenate([np.zeros(len(v), np.int8), np.ones(len(v), np.int8)])


def planes(w, h, seed=0):
    """X, Y, B planes [h, w]: the samples repeated over the plane (a frame of several 256 x 256 noise tiles holds them
    in every tile), B finite everywhere: where X or Y is not finite, B still shows the strengths that were used"""
    x, y, _ = samples()
    n = w * h
    assert n >= len(x), "the plane holds every sample"
    rng = np.random.default_rng([0x4E50, w, h, seed])
    return [np.resize(x, n).reshape(h, w).copy(), np.resize(y, n).reshape(h, w).copy(),
            rng.uniform(-0.2, 0.9, (h, w)).astype(F)]


def random_planes(w, h, seed=0):
    """what the stage hook takes as the convolved noise: anything non-zero"""
    rng = np.random.default_rng([0x4E52, w, h, seed])
    return [rng.standard_normal((h, w)).astype(F) for _ in range(3)]


def float_bits_mismatch(got, want):
    """where the wanted value is not a NaN the bits are equal; where it is, the other is a NaN (payload and sign free:
    x86 and the GPU make different default NaNs) -- the rule of tests/colour_domain_cases.py"""
    g, w = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    return np.where(np.isnan(w), ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))
