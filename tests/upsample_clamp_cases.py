"""Planes on which the clamp of Upsample2x/4x/8x (jxl/src/render/stages/upsample.rs: compute_minmax and the
.max(minval).min(maxval) at the end of kernel_conv; ups_minmax and the end of ups_taps in csrc/upsample_device.h) ACTS
-- and a float64 numpy model that tells, per output, which regime the stage is in and which of the 25 taps owns the
bound that acts.

On white noise the 25-tap sum leaves the range of its own 5x5 window on well under 1 % of the outputs, and where it
does, the bound is rarely held by one tap alone: the (7, 7) standard_normal plane of
test_gpu_parity.test_upsample_stage_bit_exact cannot tell the window's extremes from extremes that skip a tap
(tests/test_upsample_clamp_cases_cpu.py asserts that).  The populations here are made of edges:

  cells     3 x 3-pixel cells of four levels {0, .25, .5, 1} plus +-0.03 of per-pixel jitter: the sum over- and
            undershoots at every cell edge, and the jitter makes every window's extreme belong to exactly one tap
  impulses  isolated 0 / 1 pixels, four apart each way, on a 0.5 background with +-0.002 of jitter: the kernels'
            negative lobes
  ramp      a linear ramp through zero: the control, on which the clamp must not fire

with integer twins (8-bit levels {0, 64, 128, 255}, or those times 257 at 16 bits, jitter of a few steps) for the
Modular and extra-channel routes, and two custom weight sets per factor that keep both sides of the clamp busy:
`sharp` and `soft` blend the default weights with the weights of pixel replication (1 on every kernel's centre tap),
s * default + (1 - s) * replicate with s = 1.5 and 0.7.  Either keeps a constant plane constant, so the ramp stays
inside its window.  Plain scaled copies of the defaults do not: 0.9 x leaves 5.0 - 7.0 % of the cells outputs above
the maximum and 1.1 x takes the ramp down to 89 % inside (it clamps on both sides of zero), so they would serve one
condition at the cost of another; uniform(-0.1, 0.3) weights, the only custom weights the older tests use, are
one-sided on cells and nearly idle on noise.

Measured on the CPU oracle (fused build) on the (40, 70) and (19, 300) planes, minimum - maximum over n = 2, 4, 8 and
the three weight sets; the CPU test holds the thresholds in brackets:
  cells     clamped up to the minimum 14.6 - 19.3 %, down to the maximum 15.9 - 20.8 %, inside 59.8 - 69.4 %,
            unclassified <= 0.10 %                                        (>= 10 %, >= 10 %, >= 30 %, <= 2 %)
  impulses  up to the minimum 14.2 - 20.3 %, down to the maximum 13.6 - 19.2 %, inside 61.1 - 71.6 %,
            unclassified <= 0.39 %                                        (>= 10 %, >= 10 %, >= 10 %, <= 2 %)
  ramp      inside 99.92 - 99.97 % (the rest sits on the mirrored border)                          (>= 99 %)
  integer cells, 8 and 16 bits: up 17.0 - 20.3 %, down 17.6 - 21.4 %, inside 58.3 - 65.2 %
  cells     every tap 0..24 is the sole owner, by more than the guard band, of the acting bound on at least 24
            outputs per side at (40, 70) and 48 at (19, 300); at (24, 40) the corner taps drop to 3       (>= 16)
  cells     outputs on which a wrong clamp leaves the oracle's value: no clamp 30.5 - 40.2 %, the 3x3 window
            20.8 - 27.6 %, the window one row earlier 7.6 - 11.3 %, one tap missed 0.64 - 2.92 %, at least 72
            outputs for every single tap                                                                 (>= 16)
  the (7, 7) standard_normal plane: 2 of 196 outputs clamped at n = 2, 11 of 784 at n = 4, 147 of 3136 at n = 8
The model agrees with jxlo_upsample to 2.1e-7 on cells and impulses and to 4.0e-7 on the (19, 300) ramp (largest
|model's clipped value - oracle|; the ramp reaches +-1.8); GUARD = 1e-4 of the plane's largest magnitude is the band
around either bound inside which an output stays unclassified.

Planes are finite and hold no -0.0: the reference takes min / max through its SIMD layer, whose NaN and signed-zero
behaviour differs per back-end, so there is no single right answer to hold the kernel to.

The model only proves what a case reaches and names the regime behind a failing sample.  It never makes expected
pixels: those are the oracle's.  Importing this file needs neither a GPU nor the oracle; the kernels the model takes
come from oracle.upsample_kernels."""
from collections import namedtuple

import numpy as np

F = np.float32
FACTORS = (2, 4, 8)
ROWS_PER_THREAD = {2: 8, 4: 4, 8: 2}      # kRows2 / kRows4 / kRows8 of csrc/k_upsample.hip
SEAM = 256                                # columns per workgroup of k_upsample
WEIGHT_COUNT = {2: 15, 4: 55, 8: 210}
GUARD_REL = 1e-4
BELOW, ABOVE, INSIDE, UNCLASSIFIED = 0, 1, 2, 3
REGIME_NAMES = ("below the window's minimum (clamped up)", "above the window's maximum (clamped down)",
                "inside the window's range", "within the guard band of a bound")
SHAPES = [(40, 70), (19, 300)]            # (rows, columns); the second crosses SEAM and ends every R in a partial strip
REPAINT_SHAPE = (300, 70)                 # a frame 70 wide and 300 tall: two rows of 256 x 256 cells to repaint
REPAINT_SEEDS = (None, 1, 2, 11, 12, 13)  # its three channels, and the three that replace them
LEVELS = (0.0, 0.25, 0.5, 1.0)
LEVELS_8 = (0, 64, 128, 255)
JITTER, JITTER_8 = 0.03, 7


# ---------------------------------------------------------------------------------------------------------------------
# populations
def _rng(kind, shape, seed):
    return np.random.default_rng([0x5543, kind, shape[0], shape[1], seed])


# Placement.  The seed of a shape's cells and the levels of the 2 x 2 cells in each corner (top left, top right, bottom
# left, bottom right; row-major within a corner), searched with the model so that, for every factor and weight set,
# clamped outputs of both sides fall on every place of places(): tests/test_upsample_clamp_cases_cpu.py asserts it.  A
# corner's four input samples make 16 outputs at n = 2: too few for a random seed to serve nine (n, weights) pairs.
PLACED = {
    (40, 70): dict(seed=7, corners=((1, 3, 0, 0), (0, 3, 0, 0), (0, 0, 3, 2), (0, 0, 3, 3))),
    (19, 300): dict(seed=6, corners=((2, 0, 3, 0), (0, 0, 0, 2), (0, 0, 3, 3), (0, 0, 0, 3))),
}


def _cell_index(shape, seed=None):
    """(index into the four levels per sample, the generator after the draw); seed None: the shape's PLACED entry"""
    h, w = shape
    put = PLACED.get(tuple(shape), dict(seed=0, corners=None)) if seed is None else dict(seed=seed, corners=None)
    rng = _rng(1, shape, put["seed"])
    grid = rng.integers(0, 4, size=(h // 3 + 3, w // 3 + 3))
    if put["corners"]:
        cy, cx = (h - 1) // 3 - 1, (w - 1) // 3 - 1
        for (gy, gx), lv in zip(((0, 0), (0, cx), (cy, 0), (cy, cx)), put["corners"]):
            grid[gy:gy + 2, gx:gx + 2] = np.reshape(lv, (2, 2))
    return grid[np.arange(h)[:, None] // 3, np.arange(w)[None, :] // 3], rng


def cells(shape, seed=None):
    """cells of side 3; seed None: the shape's placed plane"""
    idx, rng = _cell_index(shape, seed)
    return (F(LEVELS)[idx] + rng.uniform(-JITTER, JITTER, shape).astype(F)).astype(F)


def cells_int(shape, bits=8, seed=None):
    """the integer twin: the same cells at 8-bit levels with +-7 steps of jitter; at 16 bits those times 257 plus
    0..256 (below the top level), so that ties between taps stay as rare as in the float plane"""
    assert bits in (8, 16)
    idx, rng = _cell_index(shape, seed)
    a = np.clip(np.int32(LEVELS_8)[idx] + rng.integers(-JITTER_8, JITTER_8 + 1, shape), 0, 255).astype(np.int32)
    if bits == 16:
        a = a * 257 + rng.integers(0, 257, shape).astype(np.int32) * (a < 255)
    return np.ascontiguousarray(a, dtype=np.int32)


def _lattice(shape):
    """every fourth sample of every fourth row, the rows' phase moving by two"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + 2 * (yy // 4)) % 4 == 0) & (yy % 4 == 0)


def impulses(shape, seed=0):
    """isolated pixels of 0 or 1, four apart each way, on a background of 0.5; +-0.002 of jitter everywhere"""
    rng = _rng(2, shape, seed)
    a = np.full(shape, 0.5)
    hit = _lattice(shape)
    a[hit] = rng.integers(0, 2, size=int(hit.sum()))
    return (a + rng.uniform(-0.002, 0.002, shape)).astype(F)


def ramp(shape):
    """a plane through zero at its centre (sharp and soft keep a constant, so it stays inside under them as well)"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    a = (0.011 * (xx - (w - 1) / 2) + 0.017 * (yy - (h - 1) / 2)).astype(F)
    return a + F(0.0)  # (no -0.0)


POPULATIONS = {"cells": cells, "impulses": impulses, "ramp": ramp}


def stage_test_noise_plane(n, shape=(7, 7)):
    """the plane test_gpu_parity.test_upsample_stage_bit_exact draws for factor n"""
    return np.random.default_rng(n * 100 + shape[0]).standard_normal(shape).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# weight sets
def replicate_weights(n):
    """the weights of pixel replication: 1 where the symmetric (5 n / 2)^2 quadrant indexes a kernel's centre tap"""
    m = 5 * n // 2
    out = np.zeros(WEIGHT_COUNT[n], dtype=np.float64)
    for y in range(m):
        for x in range(y, m):
            if y % 5 == 2 and x % 5 == 2:
                out[m * y - y * (y - 1) // 2 + x - y] = 1.0
    return out


def default_weights(default_kernels, n):
    """the default weights read back from the default kernels [n, n, 5, 5] (the upper triangle of the quadrant:
    weight (y, x) sits in kernel [x // 5][y // 5] at tap [x % 5][y % 5])"""
    m = 5 * n // 2
    k = np.asarray(default_kernels, dtype=F).reshape(n, n, 5, 5)
    out = np.zeros(WEIGHT_COUNT[n], dtype=F)
    for y in range(m):
        for x in range(y, m):
            out[m * y - y * (y - 1) // 2 + x - y] = k[x // 5, y // 5, x % 5, y % 5]
    return out


BLENDS = {"sharp": 1.5, "soft": 0.7}
WEIGHT_SETS = ("default",) + tuple(BLENDS)


def weights(name, n, default_kernels):
    """None for the defaults, else the f32 weights of s * default + (1 - s) * replicate"""
    if name == "default":
        return None
    s = BLENDS[name]
    return (s * default_weights(default_kernels, n).astype(np.float64) + (1.0 - s) * replicate_weights(n)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# the model
def windows(plane, back=0):
    """float64 [h, w, 25]: the mirrored 5x5 window of every sample, tap ky * 5 + kx; back = 1: the window of the row
    above instead (mirrored like any other), i.e. a window that was not advanced"""
    a = np.asarray(plane, dtype=np.float64)
    h, w = a.shape
    p = np.pad(a, 2 + back, mode="symmetric")
    return np.stack([p[ky:ky + h, back + kx:back + kx + w] for ky in range(5) for kx in range(5)], axis=-1)


def _spread(a, n):
    """[h, w] per input sample -> [h n, w n] per output"""
    return np.repeat(np.repeat(a, n, axis=0), n, axis=1)


def raw_sums(win, kernels):
    """the 25-tap sums [h n, w n] ahead of the clamp"""
    k = np.asarray(kernels, dtype=np.float64)
    n = k.shape[0]
    h, w = win.shape[:2]
    return np.einsum("yxt,abt->yaxb", win, k.reshape(n, n, 25)).reshape(h * n, w * n)


Model = namedtuple("Model", "n guard raw mn mx regime owner sole clipped")


def model(plane, kernels):
    """Per output [h n, w n]: the raw sum, the window's minimum and maximum, the regime (BELOW / ABOVE / INSIDE /
    UNCLASSIFIED), the tap that owns the bound on the output's side (of the minimum for BELOW, the maximum for ABOVE;
    -1 elsewhere), whether that tap owns it alone by more than the guard band, and the clipped value."""
    n = np.asarray(kernels).shape[0]
    win = windows(plane)
    guard = GUARD_REL * float(np.max(np.abs(plane)))
    raw = raw_sums(win, kernels)
    srt = np.sort(win, axis=-1)
    mn, mx = _spread(srt[..., 0], n), _spread(srt[..., 24], n)
    regime = np.full(raw.shape, UNCLASSIFIED, dtype=np.int8)
    regime[raw < mn - guard] = BELOW
    regime[raw > mx + guard] = ABOVE
    regime[(raw > mn + guard) & (raw < mx - guard)] = INSIDE
    arg_mn, arg_mx = _spread(np.argmin(win, axis=-1), n), _spread(np.argmax(win, axis=-1), n)
    sole_mn, sole_mx = _spread(srt[..., 1] - srt[..., 0] > guard, n), _spread(srt[..., 24] - srt[..., 23] > guard, n)
    owner = np.where(regime == BELOW, arg_mn, np.where(regime == ABOVE, arg_mx, -1)).astype(np.int8)
    sole = np.where(regime == BELOW, sole_mn, np.where(regime == ABOVE, sole_mx, False))
    return Model(n, guard, raw, mn, mx, regime, owner, sole, np.clip(raw, mn, mx))


def shares(m, where=None):
    """(below, above, inside, unclassified) as shares of the outputs (of those under the bool map `where`)"""
    r = m.regime if where is None else m.regime[where]
    return tuple(float((r == k).mean()) for k in (BELOW, ABOVE, INSIDE, UNCLASSIFIED))


def sole_owner_counts(m):
    """[2, 25]: outputs on which the clamp acts and tap t alone owns the bound, for BELOW and for ABOVE"""
    return np.array([[int(((m.regime == side) & m.sole & (m.owner == t)).sum()) for t in range(25)]
                     for side in (BELOW, ABOVE)])


def describe(plane, kernels, y, x):
    """failure output for output (y, x)"""
    m = model(plane, kernels)
    r = int(m.regime[y, x])
    own = f", bound owned by tap {int(m.owner[y, x])}{' alone' if m.sole[y, x] else ' (shared)'}" if r in (BELOW, ABOVE) else ""
    return (f"input sample (x {x // m.n}, y {y // m.n}), phase (ox {x % m.n}, oy {y % m.n}): {REGIME_NAMES[r]}{own}; "
            f"raw sum {m.raw[y, x]:.7g}, window range [{m.mn[y, x]:.7g}, {m.mx[y, x]:.7g}]")


# ---------------------------------------------------------------------------------------------------------------------
# wrong clamps: what a broken ups_minmax / clamp would give.  CPU arrays that show what the inputs can tell apart;
# nothing here is built into or run on the device.
INNER_3X3 = [ky * 5 + kx for ky in (1, 2, 3) for kx in (1, 2, 3)]


def _clip_to(raw, lo, hi, n):
    lo, hi = _spread(lo, n), _spread(hi, n)
    return np.minimum(np.maximum(raw, lo), hi)  # .max(minval).min(maxval)


def wrong_no_clamp(plane, kernels):
    return raw_sums(windows(plane), kernels)


def wrong_3x3(plane, kernels):
    win = windows(plane)
    inner = win[..., INNER_3X3]
    return _clip_to(raw_sums(win, kernels), inner.min(-1), inner.max(-1), np.asarray(kernels).shape[0])


def wrong_missing_tap(plane, kernels, t):
    win = windows(plane)
    rest = np.delete(win, t, axis=-1)
    return _clip_to(raw_sums(win, kernels), rest.min(-1), rest.max(-1), np.asarray(kernels).shape[0])


def wrong_stale_window(plane, kernels):
    """the sum of the right window, the extremes of the window one input row earlier"""
    old = windows(plane, back=1)
    return _clip_to(raw_sums(windows(plane), kernels), old.min(-1), old.max(-1), np.asarray(kernels).shape[0])


def told_apart(wrong, oracle_out, guard):
    """the number of outputs on which a wrong clamp leaves the oracle's value by more than the guard band"""
    return int((np.abs(wrong - np.asarray(oracle_out, dtype=np.float64)) > guard).sum())


# ---------------------------------------------------------------------------------------------------------------------
# places: bool maps over the outputs [h n, w n] of a (h, w) plane
def cut_size(shape, n):
    """(out_w, out_h) of a cut result: half a patch short each way, so neither is a multiple of n"""
    h, w = shape
    return w * n - n // 2, h * n - n // 2


def places(shape, n):
    """name -> bool map of the outputs at the places where the kernels' indexing changes"""
    h, w = shape
    oy, ox = np.mgrid[0:h * n, 0:w * n]
    iy, ix = oy // n, ox // n
    r = ROWS_PER_THREAD[n]
    cw, ch = cut_size(shape, n)
    out = {
        "first row of a strip": iy % r == 0,
        "last row of a strip": (iy % r == r - 1) | (iy == h - 1),
        "last column of a cut result": (ix == w - 1) & (ox < cw) & (oy < ch),
        "last row of a cut result": (iy == h - 1) & (ox < cw) & (oy < ch),
        "corner top left": (iy < 2) & (ix < 2),
        "corner top right": (iy < 2) & (ix >= w - 2),
        "corner bottom left": (iy >= h - 2) & (ix < 2),
        "corner bottom right": (iy >= h - 2) & (ix >= w - 2),
    }
    if w > SEAM:
        out["column 255, left of the seam"] = ix == SEAM - 1
        out["column 256, right of the seam"] = ix == SEAM
    return out


def to_f32(samples, bits):
    """ConvertModularToF32 of integer samples: v * (1 / (2^bits - 1)) in binary32 (held to oracle.modular_to_f32 by
    the CPU test); the model's view of an integer twin"""
    return np.asarray(samples, dtype=np.int32).astype(F) * (F(1.0) / F((1 << bits) - 1))
