"""Adaptive LF smoothing (k0b_lf_smooth of csrc/k_lf.hip) and everything that reads its result, held to the CPU oracle
bit for bit on LF images on which the stage ACTS (tests/lf_smoothing_cases.py; run with -m gpu on an MI355X).

On synth.make_vardct's own LF the stage is an identity, so no frame test could tell whether K1's LLF-from-LF, the LF
fill or read_lf took the smoothed image or the raw one.  Here every frame carries the dithered LF of the case file,
and before each comparison the oracle's smoothed and unsmoothed frames are shown to differ on more than 5 % of the
pixels of Y (frames two blocks across excepted: there the stage must leave the LF untouched, and the two are equal).
tests/test_lf_smoothing_cases_cpu.py proves on the oracle which regimes the cases reach; a failure of the stage test
names the regime of the first bad sample.

Non-finite samples are compared by lf_smoothing_cases.float_bits_mismatch: the bits where the oracle's value is not a
NaN, a NaN where it is."""
import numpy as np
import pytest

import lf_smoothing_cases as L
import test_gpu_coeff_edges as ce
from helpers import (bit_equal, diff_report, gpu_params_from, oracle_params_from, ragged_lf_rects, run_gpu_frame,
                     run_oracle_frame, upload_frame, upload_frame_piecewise)
from lf_fill_ref import expected_planes

pytestmark = pytest.mark.gpu
F = np.float32
STRIP = 4  # JXLH_FRAME_STRIP
K1_CLASSES = ["dct8", "dct16x8", "dct8x16", "dct16x16", "dct32x8", "dct8x32", "dct32x16", "dct16x32", "dct32x32",
              "special", "large"]
# what ran on a dithered-LF frame, over the whole module (test_k1_classes_and_forms_ran_on_dithered_lf reads it last)
SEEN = {"varblocks": {}, "forms": {}}


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 2)
    yield c
    c.close()


def assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


# ---------------------------------------------------------------- the stage hook
def _hold_stage(ctx, oracle, lf, hdr, what, finite=True):
    h, w = lf[0].shape
    pg = L.apply_header(ctx.default_params(w * 8, h * 8), hdr)
    po = L.apply_header(oracle.default_params(w * 8, h * 8), hdr)
    got = ctx.stage_lf_smooth(pg, lf)
    want = oracle.adaptive_lf_smoothing(po, lf)
    for c in range(3):
        bad = L.float_bits_mismatch(got[c], want[c]) if not finite else \
            np.asarray(got[c], F).view(np.uint32) != np.asarray(want[c], F).view(np.uint32)
        if bad.any():
            y, x = np.argwhere(bad)[0].tolist()
            pytest.fail(f"{what}, plane {c}: {int(bad.sum())} of {bad.size} samples differ; first at (x {x}, y {y}): got "
                        f"{got[c][y, x]!r} want {want[c][y, x]!r}; {L.describe(lf, hdr, c, y, x)}")
    return want


@pytest.mark.parametrize("hdr_name", list(L.HEADERS))
def test_stage_on_dither_populations(ctx, oracle, hdr_name):
    """every geometry x (all three channels, each alone, 0..3 steps, alternating rows) under one header"""
    for cs in L.dither_cases(hdr_name):
        want = _hold_stage(ctx, oracle, cs.lf, cs.hdr, f"{hdr_name} {cs.name}")
        if cs.meta["w"] > 2 and cs.meta["h"] > 2 and cs.meta.get("amp") == 1 and cs.meta["w"] * cs.meta["h"] >= 63:
            assert not all(bit_equal(a, b) for a, b in zip(want, cs.lf)), f"{cs.name}: the stage is idle on this case"


@pytest.mark.parametrize("hdr_name", list(L.HEADERS))
def test_stage_on_named_samples(ctx, oracle, hdr_name):
    """gap exactly 0.5, both sides of 0.75 one ulp apart (and exactly on it), each channel as the gap setter, a 20-step
    edge, zeros, denormals, overflow to inf: as the 3 x 3 image's one interior sample and as the first sample of the
    kernel's second block"""
    hdr = L.HEADERS[hdr_name]
    for nm in L.named_cases(hdr_name):
        finite = "flt_max" not in nm.name   # (those come out as NaN in their own channel)
        _hold_stage(ctx, oracle, nm.lf, hdr, f"{hdr_name} {nm.name} 3x3", finite)
        _hold_stage(ctx, oracle, L.embed(nm.lf, hdr_name=hdr_name), hdr, f"{hdr_name} {nm.name} at column 256", finite)


def test_stage_on_non_finite_samples(ctx, oracle):
    """a NaN, +inf, -inf at the centre and at a neighbour of each channel: fmaxf drops a NaN quotient as f32::max does,
    so the other channels' gap and the 0.5 floor survive"""
    for name, lf in L.non_finite_cases():
        _hold_stage(ctx, oracle, lf, L.HEADERS["default"], name, finite=False)


# ---------------------------------------------------------------- frames
def _mix(synth, mix):
    return {mix: 1.0} if isinstance(mix, int) else getattr(synth, mix)


def _large_size(synth, t):
    return max(24, synth.COVERED_X[t] * 8), max(24, synth.COVERED_Y[t] * 8)


FRAMES = {
    # key: (w, h, mix, options of synth.make_vardct)
    "24x24": (24, 24, "MIX_DCT8", dict(epf_iters=2)),                    # 3 x 3 blocks: one interior sample
    "16x200": (16, 200, "MIX_DCT8", dict(epf_iters=1)),                  # two blocks across: untouched
    "200x16": (200, 16, "MIX_DCT8", dict(epf_iters=1)),
    "66x34": (66, 34, "MIX_D1", dict(epf_iters=2)),
    "520x300": (520, 300, "MIX_D1", dict(epf_iters=2)),
    "512x512": (512, 512, "MIX_ALL", dict(epf_iters=0, gab=False)),
    "777x513": (777, 513, "MIX_ALL", dict(epf_iters=3)),
    "2056x40": (2056, 40, "MIX_DCT8", dict(epf_iters=1)),                # 257 blocks: across the kernel's block seam
    "200x232-aligned": (200, 232, "MIX_DCT8", dict(epf_iters=2, aligned=True)),   # the strip kernel takes it
    "420": (120, 72, "MIX_8X8", dict(epf_iters=1, hshift=(1, 0, 1), vshift=(1, 0, 1))),
}
LARGE_TYPES = list(range(18, 27))
UNTOUCHED = ("16x200", "200x16")
_CACHE = {}


def frame(oracle, key):
    """(workload with the dithered LF, oracle planes smoothed, oracle LF smoothed, oracle planes unsmoothed), once per
    module and never written; asserts that smoothing matters on it"""
    from jxl_rs_amd import synth
    if key not in _CACHE:
        if isinstance(key, int):
            w, h = _large_size(synth, key)
            mix, opts = key, dict(epf_iters=1)
        else:
            w, h, mix, opts = FRAMES[key]
        wl = L.dithered(synth.make_vardct(w, h, mix=_mix(synth, mix), seed=5, **opts))
        on, lf_on = run_oracle_frame(oracle, wl, num_threads=16, do_lf_smoothing=1)
        off, lf_off = run_oracle_frame(oracle, wl, num_threads=16, do_lf_smoothing=0)
        share = float((on[1].view(np.uint32) != off[1].view(np.uint32)).mean())
        if key in UNTOUCHED:
            assert share == 0 and all(bit_equal(a, b) for a, b in zip(lf_on, lf_off)), f"{key}: two blocks across"
        else:
            assert share > 0.05, f"{key}: smoothing changes {share:.3f} of the pixels of Y: the case is an identity again"
        for a in on + off + lf_on + lf_off:
            a.setflags(write=False)
        _CACHE[key] = (wl, on, lf_on, off)
    return _CACHE[key]


def _record(ctx, form):
    k1 = ctx.k1_counters()
    for k, v in k1["varblocks"].items():
        SEEN["varblocks"][k] = SEEN["varblocks"].get(k, 0) + v
    SEEN["forms"][form] = SEEN["forms"].get(form, 0) + sum(k1["varblocks"].values())


@pytest.mark.parametrize("key", list(FRAMES) + LARGE_TYPES, ids=lambda k: f"type{k}" if isinstance(k, int) else k)
def test_frames_vs_oracle(ctx, oracle, key):
    """planes and read_lf of the whole frame; the large varblock types 18..26 each as one uniform frame at their
    smallest size; a 4:2:0 frame, where the oracle's frame path decides what smoothing does to the corner layout"""
    wl, want, want_lf, _ = frame(oracle, key)
    got, got_lf = run_gpu_frame(ctx, wl)
    _record(ctx, "dense")
    assert_planes(got_lf, want_lf, f"{key}: read_lf")
    assert_planes(got, want, f"{key}: planes")


@pytest.mark.parametrize("key", ["520x300", "512x512"])
def test_every_transport_form(ctx, oracle, key):
    wl, want, _, _ = frame(oracle, key)
    slots = ce.pack_slots(wl.coeffs)
    assert slots is not None
    for form in ce.FORMS:
        ce._begin(ctx, wl, None, ce._flags(form), None)
        ce.submit(ctx, form, wl.coeffs, slots)
        ctx.frame_run()
        ctx.sync()
        assert_planes(ctx.read_planes(), want, f"{key}, form {form}")
        _record(ctx, form)


def test_strip_path(ctx, oracle):
    wl, want, want_lf, _ = frame(oracle, "200x232-aligned")
    upload_frame(ctx, wl, flags=STRIP)
    ctx.frame_run()
    ctx.sync()
    assert ctx.frame_path()[0], "the plan did not take the strip kernel"
    assert_planes(ctx.read_lf(), want_lf, "strip: read_lf")
    assert_planes(ctx.read_planes(), want, "strip: planes")


@pytest.mark.parametrize("key", ["520x300", "777x513"])
def test_band_run(ctx, oracle, key):
    """jxlh_frame_run(1, 2): the band's first LF row (32) is smoothed from row 31 of the band above"""
    wl, want, want_lf, _ = frame(oracle, key)
    upload_frame(ctx, wl)
    ctx.frame_run(1, 2)
    ctx.sync()
    got = ctx.read_planes()
    y0, y1 = 256, min(512, wl.ysize)
    assert_planes([g[y0:y1] for g in got], [t[y0:y1] for t in want], f"{key}: band rows {y0}..{y1}")
    assert_planes(ctx.read_lf(), want_lf, f"{key}: read_lf after a band run")


def _groups_touched(wl, rect, reach=1):
    x0, y0, w, h = rect
    gx = range(max(0, x0 - reach) // 32, min(wl.xblocks - 1, x0 + w - 1 + reach) // 32 + 1)
    gy = range(max(0, y0 - reach) // 32, min(wl.yblocks - 1, y0 + h - 1 + reach) // 32 + 1)
    return [y * wl.xgroups + x for y in gy for x in gx]


def test_rerender_after_an_lf_rect_is_replaced(ctx, oracle):
    """one LF rect replaced through set_lf_quantized (another seed of the same dither), the groups within one block of
    it re-rendered: equal to a fresh oracle frame on the new LF"""
    wl, want, want_lf, _ = frame(oracle, "777x513")
    got, _ = run_gpu_frame(ctx, wl)
    assert_planes(got, want, "before the replacement")
    x0, y0, w, h = rect = (29, 30, 9, 5)   # across a group corner
    other = L.dither_q(wl.xblocks, wl.yblocks, "XYB", 1, seed=77)
    new = L.with_lf(wl, [q.copy() for q in wl.lf_q])
    for q, o in zip(new.lf_q, other):
        q[y0:y0 + h, x0:x0 + w] = o[y0:y0 + h, x0:x0 + w]
    want2, want_lf2 = run_oracle_frame(oracle, new, num_threads=16)
    assert not bit_equal(want_lf2[1], want_lf[1])
    ctx.set_lf_quantized(*[q[y0:y0 + h, x0:x0 + w] for q in new.lf_q], x0=x0, y0=y0)
    touched = _groups_touched(wl, rect)
    assert len(touched) == 4 and len(touched) < wl.coeffs.shape[0]
    ctx.rerender_groups(touched)
    ctx.sync()
    assert_planes(ctx.read_lf(), want_lf2, "read_lf after the re-render")
    assert_planes(ctx.read_planes(), want2, "planes after the re-render")


def test_lf_only_groups_are_filled_from_the_smoothed_image(ctx, oracle):
    """jxlh_frame_set_groups_lf_only on a group whose interior is mostly in the 0 < factor < 1 regime (alternating
    rows): the fill reads the smoothed LF"""
    from jxl_rs_amd import synth
    wl = synth.make_vardct(520, 300, mix=synth.MIX_ALL, seed=5, epf_iters=2)
    wl = L.with_lf(wl, L.rows_q(wl.xblocks, wl.yblocks))
    cl = L.classify(L.dequant(wl.lf_q))
    assert (cl.regime[:31, :31] == L.PARTIAL).mean() > 0.8
    on = expected_planes(oracle, wl, [0], do_lf_smoothing=1)
    off = expected_planes(oracle, wl, [0], do_lf_smoothing=0)
    assert (on[1][:256, :256].view(np.uint32) != off[1][:256, :256].view(np.uint32)).mean() > 0.05
    for flag, want in ((1, on), (0, off)):
        p = gpu_params_from(ctx, wl, do_lf_smoothing=flag)
        ctx.frame_begin(p)
        ctx.set_dequant_tables(wl.tables)
        ctx.set_lf_quantized(*wl.lf_q)
        ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
        ctx.set_groups_lf_only([0])
        for g in range(1, wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        ctx.frame_run()
        ctx.sync()
        assert_planes(ctx.read_planes(), want, f"group 0 filled from the LF, do_lf_smoothing = {flag}")


@pytest.mark.parametrize("key", ["66x34", "520x300"])
def test_smoothing_off_and_slot_fed_frames_stay_unsmoothed(ctx, oracle, key):
    """do_lf_smoothing = 0, and jxlh_frame_set_lf_from_slot (which runs no smoothing whatever the flag says): the
    unsmoothed oracle frame, which differs from the smoothed one"""
    wl, on, _, off = frame(oracle, key)
    raw = L.dequant(wl.lf_q)
    got, got_lf = run_gpu_frame(ctx, wl, do_lf_smoothing=0)
    assert_planes(got_lf, raw, f"{key}: read_lf, smoothing off")
    assert_planes(got, off, f"{key}: smoothing off")
    ctx.set_lf_frame(0, *raw)
    p = gpu_params_from(ctx, wl, do_lf_smoothing=1)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_from_slot(0)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    assert_planes(ctx.read_lf(), raw, f"{key}: read_lf of the slot-fed frame")
    assert_planes(got, off, f"{key}: slot-fed frame")
    assert not bit_equal(got[1], on[1])
    ctx.clear_lf_frame(0)


@pytest.mark.parametrize("key", ["66x34", "520x300", "777x513"])
def test_ragged_rects_with_extra_precision(ctx, oracle, key):
    """the LF delivered in ragged rects, rect i with extra_precision i % 4 (its integers times 1 << precision: a step
    stays a step): the seams between the rects cross acting samples"""
    wl, want, want_lf, _ = frame(oracle, key)
    rects = ragged_lf_rects(wl.xblocks, wl.yblocks, 23)
    assert len({i % 4 for i in range(len(rects))}) == 4
    whole = [(0, 0, wl.xblocks, wl.yblocks)]
    _, lf = upload_frame_piecewise(ctx, wl, rects, whole, order=7, pitch_pad=3, extra_precision=lambda i, r: i % 4,
                                   oracle=oracle)
    assert_planes(lf, L.dequant(wl.lf_q), "the pieces dequantise to the whole-frame LF")
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_lf(), want_lf, f"{key}: read_lf")
    assert_planes(ctx.read_planes(), want, f"{key}: planes")


# ---------------------------------------------------------------- coverage
def test_k1_classes_and_forms_ran_on_dithered_lf():
    """over the module's frames every K1 class (through the work-list counters of the run) and every transport form
    ran on a frame whose LF the smoothing changes"""
    assert SEEN["forms"], "runs after the module's other tests"
    missing = [k for k in K1_CLASSES if SEEN["varblocks"].get(k, 0) == 0]
    assert not missing, missing
    for form in ce.FORMS:
        assert SEEN["forms"].get(form, 0) > 0, form
