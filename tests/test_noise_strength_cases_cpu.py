"""The planes of tests/noise_strength_cases.py, checked without a GPU: on jxlo_noise_strength alone they reach every
interval of the LUT, the saturation branch and both clamps of the result, from the in_g side and from the in_r side of
AddNoiseStage, by at least 16 samples each."""
import numpy as np

import noise_strength_cases as N

F = np.float32
ONE_HOT = [np.eye(8, dtype=F)[k] for k in range(8)]


def _strength(oracle, lut, values):
    return np.asarray([oracle.noise_strength(lut, float(v)) if not np.isnan(v) else oracle.noise_strength(lut, float("nan"))
                       for v in values], dtype=F)


def _side_values():
    """per side: the values of in / 2 as AddNoiseStage computes them from the sample's X and Y"""
    x, y, side = N.samples()
    with np.errstate(all="ignore"):
        in_g, in_r = (y - x) * F(0.5), (y + x) * F(0.5)
    return {0: in_g[side == 0], 1: in_r[side == 1]}, {0: in_r[side == 0], 1: in_g[side == 1]}


def test_samples_put_each_value_on_one_side_exactly():
    v = N.values()
    own, other = _side_values()
    for s in (0, 1):
        exact = ~np.isnan(v) & ~(np.isfinite(v) & (np.abs(v) > F(1.7e38)))   # (3e38: Y - X overflows to inf itself)
        assert np.array_equal(own[s].view(np.uint32)[exact], v.view(np.uint32)[exact]), s
        assert np.isinf(own[s][~np.isnan(v) & ~exact]).all() and (~exact).sum() == 2
        assert np.isnan(own[s][np.isnan(v)]).all()
        fin = np.isfinite(v)
        assert (other[s][fin] == 0).all(), "the other side stays at 0: interval 0, fraction 0"


def test_model_is_the_oracles_strength(oracle):
    """one-hot LUTs: strength(e_k, v) is 1 - fraction where v lands in interval k, the fraction where it lands in
    interval k - 1, and 0 elsewhere -- so eight probes give the oracle's interval and fraction of every value"""
    v = N.values()
    fi, frac, sat = N.interval(v)
    for k in range(8):
        got = _strength(oracle, ONE_HOT[k], v)
        want = np.where(fi == k, (F(0.0) - F(1.0)) * frac + F(1.0), np.where(fi + 1 == k, frac, F(0.0))).astype(F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, v[got != want][:4])
    assert (fi[sat] == 6).all() and (frac[sat] == 1).all()


def test_every_interval_branch_and_clamp_is_reached_from_both_sides(oracle):
    own, _ = _side_values()
    for s, name in ((0, "in_g"), (1, "in_r")):
        v = own[s]
        fi, frac, sat = N.interval(v)
        for k in range(7):
            inside = (fi == k) & ~sat & (frac > 0)
            assert inside.sum() >= 16, (name, k, int(inside.sum()))
        on_integer = {int(i) for i in fi[(frac == 0) & ~sat]}
        assert on_integer == set(range(7)), (name, on_integer)
        seven = v * N.K_SCALE == F(7.0)
        assert seven.any() and sat[seven].all(), "exactly 7 is the first saturated value"
        below7 = v == np.nextafter(v[seven].min(), F(0))   # one ulp of the input below the first saturated value
        assert below7.any() and (fi[below7] == 6).all() and not sat[below7].any()
        assert sat.sum() >= 16 and np.isinf(v[sat]).any() and (v[sat] >= F(1e30)).sum() >= 2, name
        assert (v < 0).sum() >= 16 and (fi[v < 0] == 0).all() and (frac[v < 0] == 0).all()
        assert (np.signbit(v) & (v == 0)).any() and np.isnan(v).any()
        assert (fi[np.isnan(v)] == 0).all() and (frac[np.isnan(v)] == 0).all(), "max(0, NaN) is 0"
        # both clamps, on the oracle: it returns exactly 0 / 1 where the value ahead of the clamp is outside [0, 1]
        lut = N.LUTS["clamps"]
        raw = N.unclamped(lut, v)
        got = _strength(oracle, lut, v)
        low, high = raw < 0, raw > 1
        assert low.sum() >= 16 and high.sum() >= 16, (name, int(low.sum()), int(high.sum()))
        assert (got[low] == 0).all() and (got[high] == 1).all()
        mid = ~low & ~high
        assert np.array_equal(got[mid].view(np.uint32), raw[mid].view(np.uint32))
        for k in range(7):
            assert (low & (fi == k)).any() and (high & (fi == k)).any(), f"{name}: interval {k} crosses both clamps"
        # neither clamp can fire on the other LUTs, and the last-only LUT acts in interval 6 and saturation alone
        for other in ("monotone", "primes", "last_only"):
            r = N.unclamped(N.LUTS[other], v)
            assert ((r >= 0) & (r <= 1)).all(), other
        act = _strength(oracle, N.LUTS["last_only"], v) != 0
        assert np.array_equal(act, (fi == 6) & (frac > 0)), name
        assert (_strength(oracle, N.LUTS["last_only"], v)[sat] == F(0.75)).all()


def test_planes_hold_every_sample_in_every_noise_tile():
    """40 x 17 holds the sample list once; 300 x 258 holds it in each of its four 256 x 256 noise tiles"""
    x, y, _ = N.samples()
    n = len(x)
    assert n <= 40 * 17
    px, py, pb = N.planes(300, 258)
    assert np.isfinite(pb).all()
    fin = np.isfinite(x) & np.isfinite(y)
    want = set(zip(x[fin].view(np.uint32).tolist(), y[fin].view(np.uint32).tolist()))
    for ys, xs in ((slice(0, 256), slice(0, 256)), (slice(0, 256), slice(256, 300)), (slice(256, 258), slice(0, 256))):
        have = set(zip(px[ys, xs].view(np.uint32).ravel().tolist(), py[ys, xs].view(np.uint32).ravel().tolist()))
        assert len(want & have) >= (len(want) if (ys.stop - ys.start) * (xs.stop - xs.start) >= 2 * n else 50)
