"""The LF images of tests/lf_smoothing_cases.py, checked without a GPU: on the oracle alone they reach every regime of
adaptive LF smoothing, each channel sets the gap where its case says so, every named case lands where its name claims,
the model agrees with the oracle about which samples change, and the oracle handles non-finite samples as the
reference's f32::max chain does.  The 5 % figures are conditions on the inputs: a generator that misses one is changed,
not the figure."""
import numpy as np
import pytest

import lf_smoothing_cases as L
from helpers import bit_equal, run_oracle_frame

F = np.float32


def _params(oracle, w, h, hdr):
    return L.apply_header(oracle.default_params(w * 8, h * 8), hdr)


def _smooth(oracle, lf, hdr):
    h, w = lf[0].shape
    return oracle.adaptive_lf_smoothing(_params(oracle, w, h, hdr), lf)


def _changed(lf, out):
    """interior samples any plane of which changed its bits"""
    ch = np.zeros(lf[0].shape, bool)
    for a, b in zip(lf, out):
        ch |= np.asarray(a, F).view(np.uint32) != np.asarray(b, F).view(np.uint32)
    return ch[1:-1, 1:-1]


@pytest.mark.parametrize("hdr_name", list(L.HEADERS))
def test_dequant_model_is_the_oracles(oracle, hdr_name):
    """the float planes the generators return are the oracle's dequantisation of their integers, bit for bit"""
    for cs in L.dither_cases(hdr_name):
        h, w = cs.lf_q[0].shape
        want = oracle.dequant_lf(_params(oracle, w, h, cs.hdr), *cs.lf_q)
        assert all(bit_equal(a, b) for a, b in zip(cs.lf, want)), cs.name
    # ... and what the stage divides by is what the oracle divides by: one step up on one side neighbour in one
    # channel is |mc - sm| = 0.2035 of a step
    fac = L.lf_factors(L.HEADERS[hdr_name])
    h = L.header(L.HEADERS[hdr_name])
    for c in range(3):
        want = (F(65536.0) / F(h["global_scale"])) / F(h["quant_lf"]) * F(h["lf_quant_factors"][c])
        assert fac[c] == want


@pytest.mark.parametrize("hdr_name", list(L.HEADERS))
def test_dither_populations_reach_every_regime(oracle, hdr_name):
    """every dither case of 9 x 7 or larger: >= 5 % of the interior samples in each regime; a single-channel case has
    that channel as the gap setter on >= 5 %; dither of 0..3 steps is the mostly-untouched population; and the oracle
    changes exactly the samples the model says it can"""
    n = 0
    for cs in L.dither_cases(hdr_name):
        w, h = cs.meta["w"], cs.meta["h"]
        out = _smooth(oracle, cs.lf, cs.hdr)
        if w <= 2 or h <= 2:
            assert all(bit_equal(a, b) for a, b in zip(cs.lf, out)), f"{cs.name}: two samples across stay untouched"
            continue
        cl = L.classify(cs.lf, cs.hdr)
        changed = _changed(cs.lf, out)
        assert not changed[cl.regime == L.ZERO].any(), f"{cs.name}: the oracle changed a sample at factor == 0"
        # at factor == 1 the sample becomes its mean: it changes wherever a channel's mean differs from it
        differs = np.zeros(changed.shape, bool)
        for c in range(3):
            differs |= cl.gaps[c] > 0
        full = cl.regime == L.FULL
        assert np.array_equal(changed[full], differs[full]), f"{cs.name}: factor == 1 samples"
        # in between, a change smaller than half an ulp can round away: at least nine in ten change
        part = cl.regime == L.PARTIAL
        if part.sum() >= 10:
            assert changed[part].mean() >= 0.9, (cs.name, float(changed[part].mean()))
        if not L.is_population(w, h):
            continue
        z, p, f = L.shares(cl)
        print(f"{hdr_name} {cs.name}: factor == 0 {z:.2f}, between {p:.2f}, == 1 {f:.2f}")
        if cs.meta.get("rows"):
            assert p >= 0.85, (cs.name, p)
        elif cs.meta["amp"] == 1:
            assert min(z, p, f) >= 0.05, (cs.name, z, p, f)
            ch = cs.meta["channels"]
            if len(ch) == 1:
                share = float((cl.setter == "XYB".index(ch)).mean())
                assert share >= 0.05, (cs.name, share)
        else:
            assert z >= 0.85 and p > 0 and f > 0, (cs.name, z, p, f)
        n += 1
    assert n >= 10


def test_every_geometry_acts_where_it_can(oracle):
    """3 x 3 .. 513 x 4: each geometry with an interior has a case the oracle changes, on both sides of the 256-thread
    block seams where it has them"""
    for w, h in L.GEOMETRIES:
        if w <= 2 or h <= 2:
            continue
        cols = np.zeros(w - 2, bool)
        for cs in L.dither_cases("default"):
            if (cs.meta["w"], cs.meta["h"]) == (w, h):
                cols |= _changed(cs.lf, _smooth(oracle, cs.lf, cs.hdr)).any(axis=0)
        assert cols.any(), (w, h)
        for seam in range(256, w - 1, 256):   # interior columns are 1 .. w - 2; cols[i] is column i + 1
            assert cols[seam - 2] and cols[seam - 1], f"{w}x{h}: both sides of the block seam at column {seam}"


@pytest.mark.parametrize("hdr_name", list(L.HEADERS))
def test_named_cases_land_where_their_names_claim(oracle, hdr_name):
    names = set()
    for nm in L.named_cases(hdr_name):
        names.add(nm.name)
        for lf, (y, x) in ((nm.lf, (1, 1)), (L.embed(nm.lf, hdr_name=hdr_name), (2, 256))):
            cl = L.classify(lf, L.HEADERS[hdr_name])
            assert cl.regime[y - 1, x - 1] == nm.regime, (nm.name, L.describe(lf, L.HEADERS[hdr_name], 1, y, x))
            assert cl.setter[y - 1, x - 1] == nm.setter, (nm.name, L.describe(lf, L.HEADERS[hdr_name], 1, y, x))
            out = _smooth(oracle, lf, L.HEADERS[hdr_name])
            same = all(np.asarray(a, F).view(np.uint32)[y, x] == np.asarray(b, F).view(np.uint32)[y, x] for a, b in zip(lf, out))
            if nm.regime == L.ZERO and "flt_max" not in nm.name:
                assert same, f"{nm.name}: the oracle changed a sample at factor == 0"
            if nm.regime != L.ZERO and any(g[y - 1, x - 1] > 0 for g in cl.gaps):
                assert not same, f"{nm.name}: the oracle left the sample alone"
    for c in "XYB":
        assert {f"gap_0.75_below_{c}", f"gap_0.75_above_{c}", f"gap_set_by_{c}", f"gap_0.5_above_{c}"} <= names
        if hdr_name == "default":
            assert f"gap_0.75_exact_{c}" in names, "an input with a quotient of exactly 0.75 exists under the default header"


def test_threshold_cases_are_one_ulp_apart():
    """the deviations of the cases below and above 0.75 are neighbouring binary32 values of the centre sample"""
    for hdr_name, hdr in L.HEADERS.items():
        for fac in L.lf_factors(hdr):
            below, exact, above = L.threshold_centres(fac)
            steps = int(above.view(np.uint32)) - int(below.view(np.uint32))
            assert L._gap_of_centre(fac, below) < 0.75 < L._gap_of_centre(fac, above)
            assert steps == 1 if exact is None else steps >= 2 and L._gap_of_centre(fac, exact) == 0.75, (hdr_name, steps)


def test_the_inputs_the_suite_had_leave_the_stage_idle(oracle):
    """why these cases exist: on the stage test's uniform(0, 1) planes and on synth.make_vardct's LF the stage acts
    (factor > 0) on fewer than 1 % of the samples"""
    from jxl_rs_amd import synth
    for w, h in ((65, 40), (128, 128)):   # test_gpu_parity.test_lf_smoothing_bit_exact
        rng = np.random.default_rng(w + h)
        lf = [rng.uniform(0, 1, size=(h, w)).astype(F) * s for s in (0.02, 1.0, 1.0)]
        acting = (L.classify(lf).regime != L.ZERO).mean()
        print(f"uniform(0, 1) {w}x{h}: factor > 0 on {acting:.5f}")
        assert acting < 0.01
    wl = synth.make_vardct(520, 300)
    lf = oracle.dequant_lf(oracle.default_params(520, 300), *wl.lf_q)
    acting = (L.classify(lf).regime != L.ZERO).mean()
    print(f"synth.make_vardct(520, 300): factor > 0 on {acting:.5f}")
    assert acting < 0.01
    # the same workload with the dithered LF: the frame's luma changes on more than 5 % of its pixels
    on, _ = run_oracle_frame(oracle, L.dithered(wl), do_lf_smoothing=1)
    off, _ = run_oracle_frame(oracle, L.dithered(wl), do_lf_smoothing=0)
    assert (on[1].view(np.uint32) != off[1].view(np.uint32)).mean() > 0.05


# ---------------------------------------------------------------- non-finite samples
def reference_chain(lf, hdr, nan_adopting=False):
    """adaptive_lf_smoothing.rs:15-41 and :83-114 transcribed literally for whole planes: gap.max(abs((mc - sm) /
    dc_factor)) channel after channel, f32::max returning the other operand when one is a NaN; then
    (3.0 - 4.0 * gap).max(0.0).  nan_adopting: `gap > g ? gap : g` instead, the expression the oracle used to have."""
    fac = L.lf_factors(hdr)
    out = [np.array(a, dtype=F) for a in lf]
    with np.errstate(all="ignore"):
        mcs, sms = [], []
        gap = None
        for c in range(3):
            a = np.asarray(lf[c], dtype=F)
            t, m, b = a[:-2], a[1:-1], a[2:]
            corner = ((t[:, :-2] + t[:, 2:]) + b[:, :-2]) + b[:, 2:]
            side = ((m[:, :-2] + m[:, 2:]) + t[:, 1:-1]) + b[:, 1:-1]
            mc = m[:, 1:-1]
            sm = (corner * L.W_CORNER + side * L.W_SIDE) + mc * L.W_CENTER
            g = np.abs((mc - sm) / fac[c])
            if gap is None:
                gap = np.full(g.shape, F(0.5))
            if nan_adopting:
                gap = np.where(gap > g, gap, g)
            else:
                gap = np.where(np.isnan(g), gap, np.where(np.isnan(gap), g, np.maximum(gap, g)))
            mcs.append(mc)
            sms.append(sm)
        factor = F(3.0) - F(4.0) * gap
        factor = np.where(np.isnan(factor), F(0.0), np.maximum(factor, F(0.0)))
        for c in range(3):
            out[c][1:-1, 1:-1] = (sms[c] - mcs[c]) * factor + mcs[c]
    return out


def test_reference_chain_is_the_oracle_on_finite_cases(oracle):
    """the transcription itself, held to the oracle where nothing is in doubt"""
    for cs in L.dither_cases("default"):
        if cs.meta["w"] > 2 and cs.meta["h"] > 2:
            want = _smooth(oracle, cs.lf, cs.hdr)
            assert all(bit_equal(a, b) for a, b in zip(reference_chain(cs.lf, cs.hdr), want)), cs.name


def test_non_finite_samples_follow_the_reference_max_chain(oracle):
    """a NaN, +inf, -inf at the centre, a side and a corner neighbour of each channel: the oracle's planes are the
    transcription's (NaN where it is a NaN, the same bits elsewhere); on some of the cases the NaN-adopting maximum the
    oracle used to have gives other finite samples, so the cases tell the two apart"""
    hdr = L.HEADERS["default"]
    told_apart = 0
    cases = L.non_finite_cases()
    assert len(cases) == 2 * 27
    for name, lf in cases:
        want = reference_chain(lf, hdr)
        got = _smooth(oracle, lf, hdr)
        for c in range(3):
            bad = L.float_bits_mismatch(got[c], want[c])
            assert not bad.any(), f"{name}, plane {c}: {np.argwhere(bad)[:4].tolist()}; " \
                                  f"{L.describe(lf, hdr, c, *np.argwhere(bad)[0])}"
        old = reference_chain(lf, hdr, nan_adopting=True)
        told_apart += any(L.float_bits_mismatch(old[c], want[c]).any() for c in range(3))
    print(f"{told_apart} of {len(cases)} cases tell the NaN-adopting maximum from f32::max")
    assert told_apart >= 6
