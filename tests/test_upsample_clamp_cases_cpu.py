"""tests/upsample_clamp_cases.py proved on the CPU oracle: what every population reaches -- both sides of the clamp, every
tap as the sole owner of the acting bound, the places where the kernels' indexing changes -- and what a wrong clamp
would change on it.  The thresholds are conditions on the inputs, not tolerances: a population that misses one is
replaced, the threshold stays.  Needs no GPU."""
import numpy as np
import pytest

import upsample_clamp_cases as U

F = np.float32
_CACHE = {}


def kernels(oracle, n, ws):
    key = ("k", n, ws)
    if key not in _CACHE:
        _CACHE[key] = oracle.upsample_kernels(n, U.weights(ws, n, oracle.upsample_kernels(n)))
    return _CACHE[key]


def case(oracle, pop, shape, n, ws):
    """(plane, the oracle's result, the model), once per module and never written"""
    key = (pop, shape, n, ws)
    if key not in _CACHE:
        plane = U.POPULATIONS[pop](shape)
        want = oracle.upsample(n, plane, U.weights(ws, n, oracle.upsample_kernels(n)))
        m = U.model(plane, kernels(oracle, n, ws))
        for a in (plane, want):
            a.setflags(write=False)
        _CACHE[key] = (plane, want, m)
    return _CACHE[key]


EVERY = [(n, ws) for n in U.FACTORS for ws in U.WEIGHT_SETS]
ids = [f"x{n}-{ws}" for n, ws in EVERY]


def test_planes_are_finite_without_negative_zero():
    for shape in U.SHAPES:
        for pop, gen in U.POPULATIONS.items():
            a = gen(shape)
            assert a.dtype == F and a.shape == shape and np.isfinite(a).all(), (pop, shape)
            assert not (np.signbit(a) & (a == 0)).any(), (pop, shape)
            assert np.array_equal(a, gen(shape)), "seeded"


@pytest.mark.parametrize("n", U.FACTORS)
def test_weight_sets(oracle, n):
    """default_weights reads the defaults back; sharp and soft keep a constant plane constant (their kernels sum to 1
    as the defaults' do) and differ from the defaults"""
    dk = oracle.upsample_kernels(n)
    assert np.array_equal(oracle.upsample_kernels(n, U.default_weights(dk, n)), dk)
    rep = oracle.upsample_kernels(n, U.replicate_weights(n).astype(F)).reshape(n * n, 25)
    assert np.array_equal(rep, np.tile(np.eye(25, dtype=F)[12], (n * n, 1))), "pixel replication: 1 on each centre tap"
    sums = dk.reshape(n * n, 25).astype(np.float64).sum(-1)
    for ws in U.BLENDS:
        w = U.weights(ws, n, dk)
        assert w.dtype == F and w.shape == (U.WEIGHT_COUNT[n],)
        k = kernels(oracle, n, ws)
        assert not np.array_equal(k, dk)
        assert np.max(np.abs(k.reshape(n * n, 25).astype(np.float64).sum(-1) - sums)) < 1e-6


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_populations_reach_both_sides(oracle, n, ws, shape):
    for pop, inside in (("cells", 0.30), ("impulses", 0.10)):
        below, above, ins, uncl = U.shares(case(oracle, pop, shape, n, ws)[2])
        assert below >= 0.10 and above >= 0.10 and ins >= inside and uncl <= 0.02, (pop, below, above, ins, uncl)
    assert U.shares(case(oracle, "ramp", shape, n, ws)[2])[2] >= 0.99, "the control: the clamp stays idle on a ramp"


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_every_tap_owns_the_acting_bound_alone(oracle, n, ws, shape):
    counts = U.sole_owner_counts(case(oracle, "cells", shape, n, ws)[2])
    assert counts.shape == (2, 25) and counts.min() >= 16, counts.tolist()


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_the_oracle_equals_the_clipped_model_within_the_guard_band(oracle, n, ws, shape):
    """a population that drifts to where the model means nothing (cancellation, huge magnitudes) fails here"""
    for pop in U.POPULATIONS:
        _, want, m = case(oracle, pop, shape, n, ws)
        assert want.shape == m.clipped.shape
        assert np.max(np.abs(m.clipped - want)) <= m.guard, pop


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_every_wrong_clamp_shows_on_cells(oracle, n, ws, shape):
    plane, want, m = case(oracle, "cells", shape, n, ws)
    k = kernels(oracle, n, ws)
    assert U.told_apart(m.clipped, want, m.guard) == 0
    assert U.told_apart(U.wrong_no_clamp(plane, k), want, m.guard) >= 16
    assert U.told_apart(U.wrong_3x3(plane, k), want, m.guard) >= 16
    assert U.told_apart(U.wrong_stale_window(plane, k), want, m.guard) >= 16
    for t in range(25):
        assert U.told_apart(U.wrong_missing_tap(plane, k, t), want, m.guard) >= 16, f"tap {t}"


@pytest.mark.parametrize("n", U.FACTORS)
def test_the_gap_white_noise_leaves(oracle, n):
    """the (7, 7) standard_normal plane of test_gpu_parity.test_upsample_stage_bit_exact: extremes that skip a tap give
    the model's own clipped values on every output, within the guard band of the oracle's, for at least one tap -- that
    test cannot see such a bug"""
    plane = U.stage_test_noise_plane(n)
    k = oracle.upsample_kernels(n)
    want = oracle.upsample(n, plane)
    m = U.model(plane, k)
    blind = [t for t in range(25) if np.array_equal(U.wrong_missing_tap(plane, k, t), m.clipped)
             and U.told_apart(U.wrong_missing_tap(plane, k, t), want, m.guard) == 0]
    assert blind, "every missing tap shows on this plane: it is not blind after all, and the docstrings that say so are wrong"
    below, above, _, _ = U.shares(m)
    assert below + above < 0.05


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_clamped_outputs_of_both_sides_at_every_place(oracle, n, ws, shape):
    """the 256-column workgroup seam, the last column and row of a cut result, the first and last row of a strip of R
    rows, the four corners where the window is mirrored both ways"""
    m = case(oracle, "cells", shape, n, ws)[2]
    pl = U.places(shape, n)
    assert ("column 255, left of the seam" in pl) == (shape[1] > U.SEAM)
    cw, ch = U.cut_size(shape, n)
    assert cw % n and ch % n and -(-cw // n) == shape[1] and -(-ch // n) == shape[0]
    for name, where in pl.items():
        assert where.shape == m.regime.shape and where.any(), name
        assert ((m.regime == U.BELOW) & where).any(), f"{name}: nothing clamped up to the minimum"
        assert ((m.regime == U.ABOVE) & where).any(), f"{name}: nothing clamped down to the maximum"
    # every strip of R rows, not just some: its first and its last row, whatever R is
    assert all(U.SHAPES[1][0] % q for q in U.ROWS_PER_THREAD.values()), "the second shape ends in a partial strip"
    rows_below = (m.regime == U.BELOW).any(axis=1).reshape(shape[0], n).any(axis=1)
    rows_above = (m.regime == U.ABOVE).any(axis=1).reshape(shape[0], n).any(axis=1)
    assert rows_below.all() and rows_above.all(), "every input row has clamped outputs of both sides"


@pytest.mark.parametrize("n,ws", EVERY, ids=ids)
def test_integer_twins_reach_both_sides(oracle, n, ws):
    """what the Modular and extra-channel routes are fed: converted as the oracle converts them, at least 10 % of the
    outputs on either side; the cut result keeps clamped outputs of both sides in its last column and row"""
    k = kernels(oracle, n, ws)
    for shape in U.SHAPES:
        for bits in (8, 16):
            smp = U.cells_int(shape, bits)
            assert smp.dtype == np.int32 and smp.min() >= 0 and smp.max() < 1 << bits
            f = oracle.modular_to_f32(smp, bits)
            assert np.array_equal(f.view(np.uint32), U.to_f32(smp, bits).view(np.uint32))
            m = U.model(f, k)
            below, above, ins, uncl = U.shares(m)
            assert below >= 0.10 and above >= 0.10 and ins >= 0.30 and uncl <= 0.02, (shape, bits, below, above, ins, uncl)
            for name, where in U.places(shape, n).items():
                if "corner" not in name:  # (the corners are placed for the float plane's jitter)
                    assert ((m.regime == U.BELOW) & where).any() and ((m.regime == U.ABOVE) & where).any(), (name, bits)


@pytest.mark.parametrize("n", [2, 8])
def test_the_repaint_frame_reaches_both_sides(oracle, n):
    """the taller Modular frame tests/test_gpu_upsample_clamp.py repaints: every channel, before and after"""
    for seed in U.REPAINT_SEEDS:
        f = oracle.modular_to_f32(U.cells_int(U.REPAINT_SHAPE, 8, seed=seed), 8)
        below, above, ins, uncl = U.shares(U.model(f, oracle.upsample_kernels(n)))
        assert below >= 0.10 and above >= 0.10 and ins >= 0.30 and uncl <= 0.02, (seed, below, above, ins, uncl)


def test_describe_names_regime_and_tap(oracle):
    plane, _, m = case(oracle, "cells", U.SHAPES[0], 2, "default")
    y, x = np.argwhere((m.regime == U.BELOW) & m.sole)[0].tolist()
    text = U.describe(plane, kernels(oracle, 2, "default"), y, x)
    assert "clamped up" in text and f"tap {int(m.owner[y, x])} alone" in text
