"""LF images on which adaptive LF smoothing (k0b_lf_smooth of csrc/k_lf.hip; jxl/src/frame/adaptive_lf_smoothing.rs)
ACTS -- and a numpy model that tells, per interior sample, which of its regimes the stage is in.

The stage computes gap = max(0.5, |mc - sm| / lf_factor[c]) over the three channels (sm: the 3x3 weighted mean) and
factor = max(0, 3 - 4 * gap), and writes (sm - mc) * factor + mc: it changes a sample only where every channel is
within 0.75 of a quantisation step of its mean.  uniform(0, 1) planes and synth.make_vardct's LF (+-27 steps of noise
on Y) never get there: on them the stage is an identity (tests/test_lf_smoothing_cases_cpu.py records how rarely it is
not).  The generators below stay within a few steps of a ramp, and take the header fields that make a step what it is.

The model (`classify`) returns the regime (factor == 0, 0 < factor < 1, factor == 1) and the channel that set the gap.
It only proves what a case reaches and names the regime behind a failing sample; it never makes expected pixels: those
are the oracle's.  Importing this file needs neither a GPU nor the oracle."""
import zlib
from collections import namedtuple

import numpy as np

F = np.float32
W_SIDE, W_CORNER = F(0.20345139757231578), F(0.0334829185968739)
W_CENTER = F(1.0) - F(4.0) * (W_SIDE + W_CORNER)
ZERO, PARTIAL, FULL = 0, 1, 2            # regimes: factor == 0, 0 < factor < 1, factor == 1
REGIME_NAMES = ("factor == 0", "0 < factor < 1", "factor == 1")
NONE, X, Y, B = -1, 0, 1, 2              # who set the gap (planes are X, Y, B; lf_q is coded order Y, X, B)
SETTER_NAMES = {NONE: "none", X: "X", Y: "Y", B: "B"}

# ---------------------------------------------------------------------------------------------------------------------
# headers: the fields of the frame parameters a step depends on (anything not named keeps its default)
DEFAULTS = dict(global_scale=21845, quant_lf=16, lf_quant_factors=(1.0 / 4096.0, 1.0 / 512.0, 1.0 / 256.0),
                base_correlation_x=0.0, base_correlation_b=1.0, ytox_lf=0, ytob_lf=0, color_factor=84)
HEADERS = {
    "default": {},
    # the ends test_gpu_coeff_edges.test_header_ends uses
    "gs1_qlf65536": dict(global_scale=1, quant_lf=65536),
    "gs73728_qlf65536": dict(global_scale=73728, quant_lf=65536),
    "gs73728_qlf1": dict(global_scale=73728, quant_lf=1),
    # factors 2^12 apart: one step of B is 4096 steps of X and 2^24 steps of Y (with base_correlation_b = 1, B carries
    # Y's dither: it is 2^-24 of a B step here) ...
    "factors_y_small": dict(lf_quant_factors=(2.0 ** -12, 2.0 ** -24, 1.0)),
    # ... and the other way round, without chroma from luma (Y's dither would be 2^24 steps of B)
    "factors_y_large": dict(lf_quant_factors=(2.0 ** -12, 1.0, 2.0 ** -24), base_correlation_b=0.0),
    # a step of 1.4e-40: every sample, mean and difference of the stage is a denormal
    # (no chroma from luma: with equal factors B would carry Y's dither step for step)
    "denormal_step": dict(global_scale=73728, quant_lf=65536, lf_quant_factors=(1e-35, 1e-35, 1e-35),
                          base_correlation_b=0.0),
    # chroma from luma at work in both chroma planes
    "cfl": dict(ytox_lf=7, ytob_lf=-3),
}


def header(hdr):
    h = dict(DEFAULTS)
    h.update(hdr or {})
    return h


def apply_header(p, hdr):
    """the header's fields onto a FrameParams-like ctypes struct (the oracle's or the library's)"""
    for k, v in (hdr or {}).items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(p, k)[i] = x
        else:
            setattr(p, k, v)
    return p


def lf_factors(hdr=None):
    """finalize_lf (frame/mod.rs:360-369): what the stage divides by"""
    h = header(hdr)
    inv_quant_lf = (F(65536.0) / F(h["global_scale"])) / F(h["quant_lf"])
    return [inv_quant_lf * F(f) for f in h["lf_quant_factors"]]


def dequant(lf_q, hdr=None, mul=1.0):
    """dequant_lf (frame/modular/mod.rs:837-929) in binary32, one rounding per operation: X, Y, B of the coded Y, X, B
    (tests/test_lf_smoothing_cases_cpu.py holds it to the oracle's bit for bit)"""
    h = header(hdr)
    inv_quant_lf = F(65536.0) / (F(h["global_scale"]) * F(h["quant_lf"]))
    fac = [(F(f) * inv_quant_lf) * F(mul) for f in h["lf_quant_factors"]]
    cfl_x = F(h["base_correlation_x"]) + F(h["ytox_lf"]) / F(h["color_factor"])
    cfl_b = F(h["base_correlation_b"]) + F(h["ytob_lf"]) / F(h["color_factor"])
    qy, qx, qb = [np.asarray(q, dtype=np.int32).astype(F) for q in lf_q]
    with np.errstate(all="ignore"):
        in_x, in_y, in_b = qx * fac[0], qy * fac[1], qb * fac[2]
        return [in_y * cfl_x + in_x, in_y, in_y * cfl_b + in_b]


# ---------------------------------------------------------------------------------------------------------------------
# the model
Classes = namedtuple("Classes", "regime setter gaps")


def classify(lf, hdr=None):
    """Per INTERIOR sample of the X, Y, B planes [h, w] (h, w > 2): regime [h - 2, w - 2] (ZERO / PARTIAL / FULL),
    setter [h - 2, w - 2] (NONE / X / Y / B: the channel whose |mc - sm| / lf_factor is the gap, NONE at the 0.5
    floor) and the three channels' quotients.  Binary32 in the stage's order of operations; a NaN quotient is dropped,
    as f32::max drops it."""
    fac = lf_factors(hdr)
    gs = []
    with np.errstate(all="ignore"):
        for c in range(3):
            a = np.asarray(lf[c], dtype=F)
            t, m, b = a[:-2], a[1:-1], a[2:]
            corner = ((t[:, :-2] + t[:, 2:]) + b[:, :-2]) + b[:, 2:]
            side = ((m[:, :-2] + m[:, 2:]) + t[:, 1:-1]) + b[:, 1:-1]
            mc = m[:, 1:-1]
            sm = (corner * W_CORNER + side * W_SIDE) + mc * W_CENTER
            gs.append(np.abs((mc - sm) / fac[c]))
        gap = np.full(gs[0].shape, F(0.5))
        setter = np.full(gs[0].shape, NONE, dtype=np.int8)
        for c in range(3):
            up = gs[c] > gap
            gap = np.where(up, gs[c], gap)
            setter = np.where(up, c, setter).astype(np.int8)
        factor = F(3.0) - F(4.0) * gap
        factor = np.where(factor > 0, factor, F(0.0))
    regime = np.where(factor == 0, ZERO, np.where(factor == 1, FULL, PARTIAL)).astype(np.int8)
    return Classes(regime, setter, gs)


def shares(cl):
    """(share of ZERO, PARTIAL, FULL) over the interior samples"""
    return tuple(float((cl.regime == r).mean()) for r in (ZERO, PARTIAL, FULL))


def describe(lf, hdr, c, y, x):
    """failure output for plane c, sample (y, x)"""
    h, w = np.asarray(lf[0]).shape
    if h <= 2 or w <= 2 or y in (0, h - 1) or x in (0, w - 1):
        return "a border sample (copied)"
    win = [np.asarray(a, dtype=F)[y - 1:y + 2, x - 1:x + 2] for a in lf]
    cl = classify(win, hdr)
    return (f"{REGIME_NAMES[int(cl.regime[0, 0])]}, gap set by {SETTER_NAMES[int(cl.setter[0, 0])]}, quotients "
            f"{[float(g[0, 0]) for g in cl.gaps]}, window of plane {c}: {win[c].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# quantised generators (coded order Y, X, B)
def ramp(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.round(20 + 0.3 * xx + 0.2 * yy).astype(np.int32)


def _rng(kind, w, h, channels, amp, seed):
    return np.random.default_rng([0x4C53, zlib.crc32(f"{kind}-{channels}".encode()), w, h, amp, seed])


CODED = {"Y": 0, "X": 1, "B": 2}  # position in lf_q


def dither_q(w, h, channels="XYB", amp=1, seed=0, mul=1):
    """the ramp round(20 + 0.3 x + 0.2 y) on all three channels plus iid steps 0..amp on the named ones; mul: every
    value times it (a rect delivered with extra_precision: a step stays a step)"""
    rng = _rng("dither", w, h, channels, amp, seed)
    q = [ramp(w, h) for _ in range(3)]
    for ch in "XYB":
        d = rng.integers(0, amp + 1, size=(h, w)).astype(np.int32)  # (drawn for every channel: one stream per case)
        if ch in channels:
            q[CODED[ch]] = q[CODED[ch]] + d
    return [(a * mul).astype(np.int32) for a in q]


def rows_q(w, h, mul=1):
    """terraces 16 columns wide (20 + x // 16) plus one step on every other row of Y: wherever the terrace is level,
    |mc - sm| of Y is 0.541 of a step -- 0 < factor < 1 on most of the image"""
    q = [np.broadcast_to(20 + np.arange(w) // 16, (h, w)).astype(np.int32) for _ in range(3)]
    q[0] = q[0] + (np.arange(h) % 2)[:, None].astype(np.int32)
    return [(a * mul).astype(np.int32) for a in q]


Case = namedtuple("Case", "name hdr_name hdr lf_q lf meta")


def make_case(name, hdr_name, lf_q, meta=None):
    hdr = HEADERS[hdr_name]
    lf_q = [np.ascontiguousarray(a, dtype=np.int32) for a in lf_q]
    return Case(name, hdr_name, hdr, lf_q, dequant(lf_q, hdr), meta or {})


# geometry (w, h): 2 x N and N x 2 stay untouched; 257 x 3 and 513 x 4 put interior samples on both sides of the
# 256-thread block seams of k0b_lf_smooth; 9 x 7 is the smallest with every regime populated
GEOMETRIES = [(3, 3), (3, 40), (40, 3), (2, 9), (9, 2), (9, 7), (257, 3), (513, 4), (65, 40)]
# (channels, amp): all three, each alone, and the mostly-untouched population
DITHERS = [("XYB", 1), ("X", 1), ("Y", 1), ("B", 1), ("XYB", 3)]


def is_population(w, h):
    """the sizes the 5 % conditions are stated for"""
    return w >= 9 and h >= 7


def dither_cases(hdr_name):
    out = []
    for w, h in GEOMETRIES:
        for channels, amp in DITHERS:
            out.append(make_case(f"dither-{w}x{h}-{channels}-amp{amp}", hdr_name, dither_q(w, h, channels, amp),
                                 dict(w=w, h=h, channels=channels, amp=amp)))
        out.append(make_case(f"rows-{w}x{h}", hdr_name, rows_q(w, h), dict(w=w, h=h, rows=True)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# named single-sample cases: float planes (X, Y, B) of 3 x 3, what the one interior sample must be classified as
Named = namedtuple("Named", "name lf regime setter")


def _flat(fac, steps=20.0):
    return [np.full((3, 3), F(steps) * f, dtype=F) for f in fac]


def _gap_of_centre(fac_c, centre):
    """the stage's quotient for a centre sample among zeros"""
    with np.errstate(all="ignore"):
        sm = (F(0.0) * W_CORNER + F(0.0) * W_SIDE) + centre * W_CENTER
        return np.abs((centre - sm) / fac_c)


def threshold_centres(fac_c, level=0.75):
    """centre values among zero neighbours whose quotient is the largest below `level`, exactly `level` (None when no
    binary32 input gives it) and the smallest above it: found by bisection over the bit pattern (the quotient is
    monotone in the centre), so the deviations are neighbouring floats"""
    lo, hi = F(0.0), F(4.0) * fac_c
    assert _gap_of_centre(fac_c, lo) < level < _gap_of_centre(fac_c, hi)
    lo_b, hi_b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while hi_b - lo_b > 1:
        mid = (lo_b + hi_b) // 2
        if _gap_of_centre(fac_c, np.uint32(mid).view(F)) < level:
            lo_b = mid
        else:
            hi_b = mid
    below = np.uint32(lo_b).view(F)
    at_or_above = np.uint32(hi_b).view(F)
    if _gap_of_centre(fac_c, at_or_above) == level:
        exact, b = at_or_above, hi_b + 1
        while _gap_of_centre(fac_c, np.uint32(b).view(F)) == level:
            b += 1
        above = np.uint32(b).view(F)
    else:
        exact, above = None, at_or_above
    return below, exact, above


def named_cases(hdr_name):
    hdr = HEADERS[hdr_name]
    fac = lf_factors(hdr)
    out = [Named("flat_gap_0.5", _flat(fac), FULL, NONE),
           Named("zeros", [np.zeros((3, 3), F) for _ in range(3)], FULL, NONE)]
    neg = [np.zeros((3, 3), F) for _ in range(3)]
    neg[1][1, 1] = F(-0.0)
    out.append(Named("negative_zero_centre", neg, FULL, NONE))
    for c, n in enumerate("XYB"):
        below, exact, above = threshold_centres(fac[c])
        for tag, v, regime in (("below", below, PARTIAL), ("exact", exact, ZERO), ("above", above, ZERO)):
            if v is None:
                continue
            pl = [np.zeros((3, 3), F) for _ in range(3)]
            pl[c][1, 1] = v
            out.append(Named(f"gap_0.75_{tag}_{n}", pl, regime, c))
        # just above the 0.5 floor: the first quotient that sets the gap at all
        _, _, over = threshold_centres(fac[c], level=0.5)
        pl = [np.zeros((3, 3), F) for _ in range(3)]
        pl[c][1, 1] = over
        out.append(Named(f"gap_0.5_above_{n}", pl, PARTIAL, c))
        # three side neighbours one step up (0.61 of a step), the other two channels flat
        pl = _flat(fac)
        for y, x in ((0, 1), (1, 0), (1, 2)):
            pl[c][y, x] += fac[c]
        out.append(Named(f"gap_set_by_{n}", pl, PARTIAL, c))
    # a 20-step edge in Y next to one step of dither in the others
    pl = _flat(fac)
    pl[1][:, 0] += F(20.0) * fac[1]
    pl[0][0, 1] += fac[0]
    pl[2][2, 2] += fac[2]
    out.append(Named("edge_20_steps_Y", pl, ZERO, Y))
    # denormal samples under a normal step: every quotient is tiny
    if hdr_name != "denormal_step":
        pl = [(np.arange(9, dtype=F).reshape(3, 3) * F(1e-42)) for _ in range(3)]
        out.append(Named("denormal_samples", pl, FULL, NONE))
    # corner / side overflow to inf: sm = inf, the quotient is inf, the sample's own channel comes out a NaN
    for sign, tag in ((1.0, "flt_max"), (-1.0, "minus_flt_max")):
        pl = _flat(fac)
        pl[1][:] = F(sign * 3.0e38)
        out.append(Named(f"{tag}_Y", pl, ZERO, Y))
    return out


def embed(lf3, w=300, h=5, at=(2, 256), hdr_name="default"):
    """the 3 x 3 planes inside w x h dithered planes, centre at (row, column) `at`: column 256 is the first thread of
    the kernel's second block"""
    bg = dequant(dither_q(w, h, "XYB", 1, seed=3), HEADERS[hdr_name])
    y, x = at
    out = [a.copy() for a in bg]
    for c in range(3):
        out[c][y - 1:y + 2, x - 1:x + 2] = lf3[c]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# non-finite samples: a NaN, +inf, -inf at the centre, at a side neighbour and at a corner neighbour of each channel, in
# a 3 x 3 image (one interior sample) and inside 9 x 7 (the sample sits in nine windows)
NON_FINITE = (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf))
PLACES = (("centre", 0, 0), ("side", 0, 1), ("corner", -1, -1))


def non_finite_cases(hdr_name="default"):
    """[(name, planes X, Y, B)]: the background is one step of dither on all three channels; seeds are picked so that
    the 3 x 3 image's interior sample is smoothed (factor > 0) before the sample is replaced"""
    out = []
    hdr = HEADERS[hdr_name]
    for w, h, cy, cx in ((3, 3, 1, 1), (9, 7, 3, 4)):
        seed = 0
        while True:
            bg = dequant(dither_q(w, h, "XYB", 1, seed), hdr)
            if classify(bg, hdr).regime[cy - 1, cx - 1] != ZERO:
                break
            seed += 1
        for c, n in enumerate("XYB"):
            for vn, v in NON_FINITE:
                for pn, dy, dx in PLACES:
                    pl = [a.copy() for a in bg]
                    pl[c][cy + dy, cx + dx] = F(v)
                    out.append((f"{vn}_{pn}_{n}_{w}x{h}", pl))
    return out


def float_bits_mismatch(got, want):
    """THE COMPARISON RULE where a NaN can come out (the rule of tests/colour_domain_cases.py): where the wanted value
    is not a NaN the bits are equal, sign of zero and infinities included; where it is a NaN the other is a NaN, payload
    and sign free (x86 and the GPU make different default NaNs).  Returns the bool map of samples that break it."""
    g, w = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    wn = np.isnan(w)
    return np.where(wn, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# frames: a synth workload whose lf_q is replaced
def with_lf(wl, lf_q):
    import copy
    w2 = copy.copy(wl)
    w2.lf_q = [np.ascontiguousarray(a, dtype=np.int32) for a in lf_q]
    assert all(a.shape == b.shape for a, b in zip(w2.lf_q, wl.lf_q))
    return w2


def dithered(wl, channels="XYB", amp=1, seed=None):
    """the workload with dither_q as its LF; seed None: the first seed on which the stage acts (factor > 0) on at least
    30 % of the interior samples under the default header -- on a 3 x 3 image, on its one interior sample"""
    if seed is None:
        seed = 0
        while wl.xblocks > 2 and wl.yblocks > 2:
            cl = classify(dequant(dither_q(wl.xblocks, wl.yblocks, channels, amp, seed)))
            if (cl.regime != ZERO).mean() >= 0.3:
                break
            seed += 1
    return with_lf(wl, dither_q(wl.xblocks, wl.yblocks, channels, amp, seed))
