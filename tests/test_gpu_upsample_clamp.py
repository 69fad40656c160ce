"""Every kernel that upsamples 2x / 4x / 8x (csrc/upsample_device.h: ups_minmax and the clamp at the end of ups_taps),
held to the CPU oracle bit for bit on inputs on which the clamp to the 5x5 window's range ACTS on both sides
(tests/upsample_clamp_cases.py; run with -m gpu on an MI355X).  tests/test_upsample_clamp_cases_cpu.py proves on the
oracle what the planes reach: 14 - 21 % of the outputs clamped up, as many clamped down, every tap the sole owner of the
acting bound, clamped outputs on the 256-column workgroup seam, in the last column and row of a cut result, in the first
and last row of every strip of R rows and in the four mirrored corners.

  k_upsample          the stage hook; Modular and VarDCT frames with frame_header.upsampling, whole and cut
  k_upsample_rows     repaint_groups on an upsampled Modular frame
  k_extra_rects       extra channels by rect, upsampled straight from their integers; the whole-plane route beside it
  the strip path      an extra channel of a JXLH_FRAME_STRIP frame
  k_lf_fill           groups filled from a cells LF image
  k_lf_preview        an LF slot that holds cells

The expected side is always oracle.upsample or a restatement that calls it (repaint_ref, lf_fill_ref, lf_preview_ref,
test_gpu_extra_rects.finished).  Where a case builds its input from decoded planes, the clamp's share on the ORACLE's
planes is asserted before the device runs.  A mismatch names regime and owning tap of the first bad outputs."""
import numpy as np
import pytest

import lf_preview_ref as lp
import lf_smoothing_cases as L
import repaint_ref as rr
import save_ref as sr
import test_gpu_extra_rects as xr
import upsample_clamp_cases as U
from helpers import bit_equal, diff_report, gpu_params_from, oracle_params_from, run_oracle_frame, upload_frame
from lf_fill_ref import expected_planes, lf_image

pytestmark = pytest.mark.gpu
F = np.float32
STRIP = 4  # JXLH_FRAME_STRIP


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def hold(got, want, what, plane=None, kernels=None):
    """bit for bit; plane / kernels: the upsampler's input and taps where the test has them -- the first bad outputs are
    then named by the model (regime, owning tap)"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if bit_equal(got, want):
        return
    bad = np.argwhere(np.ascontiguousarray(got, F).view(np.uint32) != np.ascontiguousarray(want, F).view(np.uint32))
    lines = [f"{what}: {diff_report(got, want)}"]
    if plane is not None:
        for y, x in bad[:4].tolist():
            lines.append(f"  (x {x}, y {y}) got {got[y, x]!r} want {want[y, x]!r}: {U.describe(plane, kernels, y, x)}")
    pytest.fail("\n".join(lines))


def both_sides(oracle, plane, n, least, what, weights=None):
    """the condition on an input that a case built itself: at least `least` of the outputs on either side"""
    below, above, _, _ = U.shares(U.model(plane, oracle.upsample_kernels(n, weights)))
    assert below >= least and above >= least, f"{what}: {below:.3f} clamped up, {above:.3f} clamped down: the clamp idles"


# ---------------------------------------------------------------- the stage hook
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n", U.FACTORS)
def test_stage_hook(ctx, oracle, n, shape):
    """every population under the default weights, sharp, soft, and the defaults again"""
    dk = oracle.upsample_kernels(n)
    try:
        for ws in U.WEIGHT_SETS + ("default",):
            w = U.weights(ws, n, dk)
            ctx.set_upsampling_weights(**({} if w is None else {f"w{n}": w}))
            k = oracle.upsample_kernels(n, w)
            for pop, gen in U.POPULATIONS.items():
                plane = gen(shape)
                hold(ctx.stage_upsample(n, plane), oracle.upsample(n, plane, w), f"x{n} {ws} {pop} {shape}", plane, k)
    finally:
        ctx.set_upsampling_weights()


# ---------------------------------------------------------------- the frame path
def modular_planes(shape, bits=8):
    """the placed integer cells and two more seeds of them"""
    return [U.cells_int(shape, bits)] + [U.cells_int(shape, bits, seed=s) for s in (1, 2)]


def run_modular(c, chans, n, cut=None):
    h, w = chans[0].shape
    p = c.default_params(w, h)
    p.gab, p.epf_iters, p.upsampling = 0, 0, n
    if cut:
        p.xsize_upsampled, p.ysize_upsampled = cut
    c.modular_frame_begin(p)
    c.set_modular_channels(*chans, 8)
    c.frame_run()
    c.sync()
    return p


@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n", U.FACTORS)
def test_modular_frame_whole_and_cut(ctx, oracle, n, shape):
    """k_upsample inside jxlh_frame_run: no Gaborish, EPF or noise, so the planes are the upsampled samples"""
    chans = modular_planes(shape)
    coded = [oracle.modular_to_f32(c, 8) for c in chans]
    k = oracle.upsample_kernels(n)
    want = [oracle.upsample(n, f) for f in coded]
    for cut in (None, U.cut_size(shape, n)):
        run_modular(ctx, chans, n, cut)
        got = ctx.read_planes()
        ow, oh = cut if cut else (shape[1] * n, shape[0] * n)
        for c in range(3):
            hold(got[c], want[c][:oh, :ow], f"x{n} {shape} cut {cut} plane {c}", coded[c], k)


_VARDCT = {}
VW, VH = 200, 120


def vardct_frame(oracle):
    """200 x 120, every transform of MIX_D1, no filters; the LF is cells at 32 quantisation steps per 8-bit step, so
    that the block edges stand out of the coefficients' texture: (workload, the oracle's planes), once per module"""
    from jxl_rs_amd import synth
    if not _VARDCT:
        wl = synth.make_vardct(VW, VH, mix=synth.MIX_D1, seed=5, epf_iters=0, gab=False, lf_smoothing=False)
        wl = L.with_lf(wl, [U.cells_int((wl.yblocks, wl.xblocks), seed=s) * 32 for s in (1, 2, 3)])
        planes = [np.ascontiguousarray(p) for p in run_oracle_frame(oracle, wl)[0]]
        for a in planes:
            a.setflags(write=False)
        _VARDCT["f"] = (wl, planes)
    return _VARDCT["f"]


@pytest.mark.parametrize("n,cut", [(2, None), (4, (VW * 4 - 3, VH * 4 - 1))], ids=["x2", "x4-cut"])
def test_vardct_frame(ctx, oracle, n, cut):
    wl, coded = vardct_frame(oracle)
    for c in range(3):
        both_sides(oracle, coded[c], n, 0.05, f"plane {c} of the decoded frame")
    over = dict(upsampling=n)
    if cut:
        over.update(xsize_upsampled=cut[0], ysize_upsampled=cut[1])
    upload_frame(ctx, wl, **over)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    ow, oh = cut if cut else (VW * n, VH * n)
    k = oracle.upsample_kernels(n)
    for c in range(3):
        hold(got[c], oracle.upsample(n, coded[c])[:oh, :ow], f"x{n} plane {c}", coded[c], k)


# ---------------------------------------------------------------- repaint
@pytest.mark.parametrize("n", [2, 8])
def test_repaint_of_a_modular_cell(ctx, fresh, oracle, n):
    """k_upsample_rows: the second cell's samples are replaced by another seed's and the cell repainted; the rows next to
    the cell seam (255 | 256) read both; against the oracle and against a fresh context's whole run"""
    h, w = U.REPAINT_SHAPE
    chans, other = [[U.cells_int(U.REPAINT_SHAPE, seed=s) for s in U.REPAINT_SEEDS[i:i + 3]] for i in (0, 3)]
    run_modular(ctx, chans, n)
    for c, (g, e) in enumerate(zip(ctx.read_planes(), rr.modular_result(oracle, chans, 0, 0, n))):
        hold(g, e, f"x{n} whole run, plane {c}")
    cur = [c.copy() for c in chans]
    for g in (1, 0):
        x0, y0, x1, y1 = rr.cell(w, h, g)
        for c in range(3):
            cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1]
        ctx.set_modular_channels(*[np.ascontiguousarray(c[y0:y1, x0:x1]) for c in cur], 8, x0=x0, y0=y0)
        ctx.repaint_groups([g])
        ctx.sync()
        got = ctx.read_planes()
        want = rr.modular_result(oracle, cur, 0, 0, n)
        run_modular(fresh, cur, n)
        k = oracle.upsample_kernels(n)
        for c in range(3):
            coded = oracle.modular_to_f32(cur[c], 8)
            hold(fresh.read_planes()[c], want[c], f"x{n} cell {g}: a FRESH context, plane {c}", coded, k)
            hold(got[c], want[c], f"x{n} cell {g}: repainted, plane {c}", coded, k)


# ---------------------------------------------------------------- extra channels
def feed_both_routes(ctx, plane, bits, n, seed):
    """extra channel 0 whole (jxlh_frame_set_extra_channel), extra channel 1 by rect: a ragged tiling in two calls"""
    h, w = plane.shape
    rng = np.random.default_rng(seed)
    ctx.set_extra_channel(0, plane, bits, n)
    ctx.begin_extra_channel(1, w, h, bits, n)
    pieces = [(1, x0, y0, plane[y0:y0 + rh, x0:x0 + rw]) for x0, y0, rw, rh in xr.ragged_tiling(rng, w, h)]
    order = rng.permutation(len(pieces))
    for i, part in enumerate(np.array_split(order, 2)):
        xr.hand_over(ctx, [pieces[j] for j in part], ("host", "device")[i], (0, 3)[i])


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
@pytest.mark.parametrize("n", U.FACTORS)
def test_extra_channels_whole_and_by_rect(ctx, oracle, n, shape, bits):
    """a Modular frame of the cut result's size (neither side a multiple of n) with the integer cells as two extra
    channels of factor n"""
    res_w, res_h = U.cut_size(shape, n)
    plane = U.cells_int(shape, bits)
    p = ctx.default_params(res_w, res_h)
    p.gab, p.epf_iters = 0, 0
    zeros = np.zeros((res_h, res_w), np.int32)
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(zeros, zeros, zeros, 8)
    feed_both_routes(ctx, plane, bits, n, n * 100 + bits)
    ctx.frame_run()
    ctx.sync()
    want = xr.finished(oracle, plane, bits, 0, n, res_w, res_h)
    f, k = oracle.modular_to_f32(plane, bits), oracle.upsample_kernels(n)
    for ec, route in enumerate(("whole plane", "by rect")):
        hold(ctx.read_extra_channel(ec, res_w, res_h), want, f"x{n} {shape} {bits} bits, {route}", f, k)


def test_extra_channels_of_a_strip_frame(ctx, oracle):
    """JXLH_FRAME_STRIP: the strip kernel renders the colour, the extra channels (factor 8 and 2) ride the same run"""
    from jxl_rs_amd import synth
    res_w, res_h = U.cut_size(U.SHAPES[0], 8)  # 556 x 316
    wl = synth.make_vardct(res_w, res_h, mix=synth.MIX_DCT8, seed=3, epf_iters=1, aligned=True)
    colour, _ = run_oracle_frame(oracle, wl)
    upload_frame(ctx, wl, flags=STRIP)
    plane = U.cells_int(U.SHAPES[0], 8)
    feed_both_routes(ctx, plane, 8, 8, 5)
    half = U.cells_int((-(-res_h // 2), -(-res_w // 2)), 16)
    both_sides(oracle, oracle.modular_to_f32(half, 16), 2, 0.10, "the factor-2 channel")
    ctx.set_extra_channel(2, half, 16, 2)
    ctx.frame_run()
    ctx.sync()
    assert ctx.frame_path()[0], "the plan did not take the strip kernel"
    want = xr.finished(oracle, plane, 8, 0, 8, res_w, res_h)
    f = oracle.modular_to_f32(plane, 8)
    for ec in (0, 1):
        hold(ctx.read_extra_channel(ec, res_w, res_h), want, f"strip frame, extra channel {ec}", f, oracle.upsample_kernels(8))
    hold(ctx.read_extra_channel(2, res_w, res_h), xr.finished(oracle, half, 16, 0, 2, res_w, res_h), "strip frame, x2",
         oracle.modular_to_f32(half, 16), oracle.upsample_kernels(2))
    for c, g in enumerate(ctx.read_planes()):
        hold(g, colour[c], f"strip frame, colour plane {c}")


# ---------------------------------------------------------------- LF fill
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_lf_fill_from_a_cells_lf_image(ctx, oracle, shape):
    """every group LF-only, no filters and no LF smoothing: the frame is the 8x upsampled LF image, whose three planes
    are cells (B carries Y's through the default chroma from luma)"""
    from jxl_rs_amd import synth
    yb, xb = shape
    wl = synth.make_vardct(xb * 8 - 3, yb * 8 - 5, mix=synth.MIX_DCT8, seed=9, epf_iters=0, gab=False, lf_smoothing=False)
    assert (wl.yblocks, wl.xblocks) == shape
    wl = L.with_lf(wl, modular_planes(shape))
    lf = lf_image(oracle, wl, oracle_params_from(oracle, wl))
    for c in range(3):
        both_sides(oracle, lf[c], 8, 0.10, f"plane {c} of the oracle's LF image")
    marked = list(range(wl.xgroups * wl.ygroups))
    want = expected_planes(oracle, wl, marked)
    ctx.frame_begin(gpu_params_from(ctx, wl))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.set_groups_lf_only(marked)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    k = oracle.upsample_kernels(8)
    for c in range(3):
        hold(got[c], want[c], f"LF fill {shape}, plane {c}", lf[c], k)


# ---------------------------------------------------------------- LF preview
@pytest.mark.parametrize("shape", U.SHAPES, ids=str)
def test_lf_preview_of_a_cells_slot(ctx, oracle, shape):
    """an LF slot of cells at XYB magnitudes, previewed as binary32 (the entry point always runs the colour stage: the
    samples compared are the colour stage's of the upsampled ones, as in tests/test_gpu_lf_preview.py)"""
    from test_gpu_lf_preview import check_preview, colours, SLOT
    sh, sw = shape
    iw, ih = sw * 8 - 3, sh * 8 - 5
    assert lp.slot_size(iw, ih) == (sw, sh)
    a, b, c = U.cells(shape), U.cells(shape, seed=1), U.cells(shape, seed=2)
    planes = [((b - F(0.5)) * F(0.03)).astype(F), (a * F(0.8)).astype(F), (a * F(0.8) + (c - F(0.5)) * F(0.1)).astype(F)]
    for i in range(3):
        both_sides(oracle, planes[i], 8, 0.10, f"plane {i} of the slot")
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    check_preview(ctx, oracle, sr.desc([0, 1, 2], sr.F32), planes, iw, ih, colour, what=f"cells slot {shape}")
    check_preview(ctx, oracle, sr.desc([0, 1, 2], sr.U16), planes, iw, ih, colour, rects=[(1, 1, sw - 1, sh - 1)],
                  device=True, what=f"cells slot {shape}, a rect")
    ctx.clear_lf_frame(SLOT)
