"""Frames and planes longer than 65 535 samples on one axis (run with -m gpu on an MI355X).

jxlh_frame_begin takes up to 2^20 on either axis, the Modular and stage entry points as much, yet nothing else in the
suite hands a kernel more than 16 384 rows -- and several launches put one image row (or 2 to 8) per workgroup in
gridDim.y, for which HIP reports a bound of 65 536 on earlier CDNA parts.  gfx950 launches such grids and runs every
row of them: that is what these tests pin.  Every comparison is bit-exact against the CPU oracle.

The tests must not pass by accident.  A kernel that wraps its row index modulo 65 536 writes the head of the image
where the tail belongs, and one that skips the rows above the limit leaves what the output buffer held (zeros in the
bindings, poison where a test passes the buffer).  So every expected result is first checked on the oracle side
(_tail_tells): its part at 65 536 and beyond differs from its first samples, and holds more than 16 distinct values --
or, where that part is a single pixel or one row of at most 8 samples of one channel and cannot hold 17 values, is not
all zero.  Every frame is rendered behind a flat frame of the same size (_scrub), so that the device buffers do not
hold the right pixels from an earlier case.  A build whose row kernels wrap blockIdx.y at 65 536 fails every test here
that reaches such a launch."""
import functools

import numpy as np
import pytest

from helpers import DeviceArray, bit_equal, diff_report, gpu_params_from, run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu

LONG = 65536          # one more than the largest gridDim.y earlier CDNA parts report
UNFUSED, STRIP = 1, 4  # JXLH_FRAME_UNFUSED_FILTERS, JXLH_FRAME_STRIP
GAB_W1, GAB_W2 = 0.115169525, 0.061248592
WP_DEFAULT = (16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12)
LUM = (0.2627, 0.678, 0.0593)


@pytest.fixture(scope="module")
def ctx():
    from jxl_rs_amd import Context
    c = Context(0, n_slots=1)
    yield c
    c.close()


def _tail_tells(want, axis=0, start=LONG):
    """the oracle's result tells a wrapped or skipped long axis from a right one (see the module's docstring); start:
    the first sample along `axis` that workgroup row 65 536 writes"""
    want = np.asarray(want)
    n = want.shape[axis]
    assert n > start
    tail, head = np.take(want, range(start, n), axis=axis), np.take(want, range(n - start), axis=axis)
    assert not np.array_equal(tail, head), f"the samples at {start}.. equal the first ones: a wrapped index would pass"
    if tail.size > 32:
        assert len(np.unique(tail)) > 16, f"too few distinct values at {start}..: skipped rows could pass"
    else:
        assert np.any(tail != 0), f"only zeros at {start}..: skipped rows over a zeroed buffer could pass"


def _long_axis(shape):
    return 0 if shape[0] > LONG else 1


def _frozen(arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs


# ------------------------------------------------------------------ whole frames
FRAMES = {"8x65544": (8, 65544), "1x65537": (1, 65537), "65544x8": (65544, 8), "65537x1": (65537, 1)}
TALL = ["8x65544", "1x65537"]
# seeds picked on the CPU so that _tail_tells holds for the planes and for every integer output below (with seed 1 the
# 64 pixels of 8 x 65544 at row 65 536 and beyond hold 25 distinct sRGB bytes but only 12 distinct 8-bit PQ bytes)
SEEDS = {"8x65544": 4, "1x65537": 1, "65544x8": 1, "65537x1": 1}


@functools.lru_cache(maxsize=None)
def _frame(name):
    """(workload, the oracle's planes, the oracle's smoothed LF): built once per shape, shared read-only"""
    from jxl_rs_amd import synth
    from oracle.oracle import Oracle
    w, h = FRAMES[name]
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=SEEDS[name], unique_groups=4, epf_iters=2, gab=True)
    want, want_lf = run_oracle_frame(Oracle(fused=True), wl)
    for p in want:
        _tail_tells(p, _long_axis(p.shape))
    return wl, _frozen(want), _frozen(want_lf)


def _xyb_params(oracle, kat, intensity_target=255.0):
    k = kat["output_stage"]
    return oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, intensity_target)


def _same_planes(got, want, what):
    for c in range(3):
        assert got[c].shape == want[c].shape, (what, c, got[c].shape, want[c].shape)
        assert bit_equal(got[c], want[c]), f"{what}: plane {c}: {diff_report(got[c], want[c])}"


def _same_samples(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} samples differ, first at {bad[:3].tolist()}, last at {bad[-1].tolist()}"


def _scrub(ctx, wl):
    """Renders a flat frame of the same size first (constant LF, no HF coefficients: every group an empty sparse run).
    The planes and the filters' second set of planes then hold its pixels: a test that repeats a frame on one context
    would otherwise find the right pixels already where a kernel that skips rows fails to write them."""
    ctx.frame_begin(gpu_params_from(ctx, wl))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*[np.full_like(q, 3) for q in wl.lf_q])
    ctx.set_hf_meta(np.full_like(wl.transform_map, 0x80), np.ones_like(wl.raw_quant), np.zeros_like(wl.epf_map),
                    np.zeros_like(wl.ytox), np.zeros_like(wl.ytob))
    ng = wl.coeffs.shape[0]
    ctx.submit_groups_sparse(np.arange(ng, dtype=np.uint32), np.zeros(1, np.uint32), np.zeros(3 * ng, np.uint32))
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()


def _render(ctx, wl, flags=0):
    _scrub(ctx, wl)
    upload_frame(ctx, wl, flags=flags)
    ctx.frame_run()
    ctx.sync()


@pytest.mark.parametrize("path", ["fused", "unfused", "strip"])
@pytest.mark.parametrize("name", list(FRAMES))
def test_long_frame_planes(ctx, name, path):
    """the planes after jxlh_frame_run (Gaborish + EPF1 + EPF2) through the fused filters, the per-stage kernels and the
    strip kernel, and the smoothed LF"""
    wl, want, want_lf = _frame(name)
    _render(ctx, wl, flags={"fused": 0, "unfused": UNFUSED, "strip": STRIP}[path])
    if path == "strip":
        ran = ctx.frame_path()[0]
        # one 64-pixel strip per band is always resident; the wide frames have more strips than resident workgroups
        # and are handed to the two-kernel path by the library
        assert ran or name not in TALL, "the strip kernel did not take the tall frame"
    _same_planes(ctx.read_planes(), want, f"{name} {path}")
    got_lf = ctx.read_lf()
    for c in range(3):
        assert bit_equal(got_lf[c], want_lf[c]), f"{name} {path}: LF ch{c}"


@pytest.mark.parametrize("name", list(FRAMES))
def test_long_frame_integer_outputs(ctx, oracle, kat, name):
    """jxlh_frame_read_rgb8 / _rgb16 with 3 and 4 channels, jxlh_frame_read_output with the PQ transfer function, and a
    band of rows that starts below row 65 536 and ends above it"""
    from jxl_rs_amd import lib
    wl, want, _ = _frame(name)
    w, h = FRAMES[name]
    axis = 0 if h > LONG else 1
    params, pq = _xyb_params(oracle, kat), _xyb_params(oracle, kat, 10000.0)
    want8 = {ch: oracle.xyb_to_rgb8(params, want, w, h, ch) for ch in (3, 4)}
    want16 = {ch: oracle.xyb_to_rgb16(params, want, w, h, ch) for ch in (3, 4)}
    want_pq = {(bits, ch): oracle.xyb_to_rgb_tf(pq, "pq", want, w, h, ch, bits, 10000.0, LUM) for bits, ch in ((8, 3), (16, 4))}
    for a in list(want8.values()) + list(want16.values()) + list(want_pq.values()):
        _tail_tells(a, axis)
    _render(ctx, wl)
    for ch in (3, 4):
        _same_samples(ctx.read_rgb8(params, ch), want8[ch], f"{name} rgb8 x{ch}")
        _same_samples(ctx.read_rgb16(params, ch), want16[ch], f"{name} rgb16 x{ch}")
        if h > LONG:
            y0, y1 = LONG - 6, min(h, LONG + 8)
            _same_samples(ctx.read_rgb8(params, ch, y0, y1), want8[ch][y0:y1], f"{name} rgb8 x{ch} rows {y0}:{y1}")
            _same_samples(ctx.read_rgb16(params, ch, y0, y1), want16[ch][y0:y1], f"{name} rgb16 x{ch} rows {y0}:{y1}")
    for (bits, ch), exp in want_pq.items():
        _same_samples(ctx.read_output(lib.COLOR_XYB, "pq", pq, 10000.0, LUM, bits, ch), exp, f"{name} pq {bits} bit")


@pytest.mark.parametrize("flags", [0, UNFUSED], ids=["fused", "unfused"])
def test_tall_frame_band_run_rerender_and_rect_read(ctx, oracle, flags):
    """8 x 65 544, 257 group rows: a band run over the last two group rows (the band crosses row 65 536), then the whole
    frame, jxlh_frame_rerender_groups of the last group, and jxlh_frame_read_planes_rect of the last group into a
    poisoned buffer larger than the rect"""
    from copy import copy
    wl, want, _ = _frame("8x65544")
    assert wl.ygroups == 257 and wl.xgroups == 1
    _scrub(ctx, wl)
    upload_frame(ctx, wl, flags=flags)
    ctx.frame_run(255, 257)
    ctx.sync()
    got = ctx.read_planes()
    y0 = 255 * 256
    _same_planes([g[y0:] for g in got], [p[y0:] for p in want], "band run over group rows 255..256")
    ctx.frame_run()
    ctx.sync()
    _same_planes(ctx.read_planes(), want, "whole run after the band run")
    # the last group arrives again with other coefficients (its neighbour's): only a re-render that reaches row 65 536
    # and beyond shows them
    wl2 = copy(wl)
    wl2.coeffs = wl.coeffs.copy()
    wl2.coeffs[256] = wl.coeffs[255]
    want2, _ = run_oracle_frame(oracle, wl2)
    assert not any(bit_equal(want2[c][LONG:], want[c][LONG:]) for c in range(3))
    ctx.submit_group(256, wl2.coeffs[256])
    ctx.slot_wait(0)
    ctx.rerender_groups([256])
    ctx.sync()
    _same_planes(ctx.read_planes(), want2, "after re-rendering the last group")
    out = [np.full((16, 16), np.nan, dtype=np.float32) for _ in range(3)]
    ctx.read_planes_rect(0, LONG, 16, 16, out)
    for c in range(3):
        assert bit_equal(out[c][:8, :8], want2[c][LONG:, :]), f"rect read of the last group, plane {c}"
        rest = out[c].copy()
        rest[:8, :8] = np.nan
        assert np.isnan(rest).all(), "the rect read wrote outside the frame's part of the buffer"


@pytest.mark.parametrize("name", TALL)
def test_tall_frame_slot_resident_submission(ctx, name):
    """the tall frames submitted in the slot-bucketed form: the transforms read the entries in place (direct K1 path)"""
    from jxl_rs_amd import lib as jl
    wl, want, _ = _frame(name)
    ng = wl.coeffs.shape[0]
    parts = [jl.host_pack_slots(wl.coeffs[g], group_id=g) for g in range(ng)]
    assert all(len(q[3]) == 0 for q in parts)
    _scrub(ctx, wl)
    ctx.frame_begin(gpu_params_from(ctx, wl))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.submit_groups_slots(np.arange(ng, dtype=np.uint32), np.concatenate([q[0] for q in parts]),
                            np.concatenate([q[1].reshape(-1) for q in parts]), np.concatenate([q[2] for q in parts]), None)
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()
    _same_planes(ctx.read_planes(), want, f"{name} slot-resident")


def test_tall_subsampled_frame_ycbcr_output_and_planes(ctx, oracle):
    """16 x 65 552, 4:2:0, 8x8 transforms, no filters: the integer output straight from the sub-sampled channels
    (k_ycbcr_sub_to_rgb), then the planes (the chroma upsampling kernel), then the integer output again from them"""
    from jxl_rs_amd import synth
    w, h = 16, 65552
    hs = vs = (1, 0, 1)
    wl = synth.make_vardct(w, h, mix=synth.MIX_8X8, seed=1, unique_groups=4, epf_iters=0, gab=False, lf_smoothing=False,
                           hshift=hs, vshift=vs)
    wl.lf_q[0] = wl.lf_q[0] // 3   # keep Y + 128/255 inside [0, 1] so the clamps are not the whole story
    want, _ = run_oracle_frame(oracle, wl)
    for p in want:
        _tail_tells(p)
    want8 = {ch: oracle.ycbcr_to_rgb8(want, w, h, ch) for ch in (3, 4)}
    want16 = {ch: oracle.ycbcr_to_rgb16(want, w, h, ch) for ch in (3, 4)}
    for a in list(want8.values()) + list(want16.values()):
        _tail_tells(a)
    _render(ctx, wl)
    for ch in (3, 4):
        _same_samples(ctx.read_ycbcr_rgb8(ch), want8[ch], f"ycbcr rgb8 x{ch}")
        _same_samples(ctx.read_ycbcr_rgb16(ch), want16[ch], f"ycbcr rgb16 x{ch}")
        y0, y1 = LONG - 5, h - 3
        _same_samples(ctx.read_ycbcr_rgb8(ch, y0, y1), want8[ch][y0:y1], f"ycbcr rgb8 x{ch} rows {y0}:{y1}")
    _same_planes(ctx.read_planes(), want, "4:2:0 planes")
    _same_samples(ctx.read_ycbcr_rgb8(3), want8[3], "ycbcr rgb8 from the full planes")


# ------------------------------------------------------------------ stage and Modular entry points
# (rows, columns): the long axis as the row count on planes 1, 3 and 8 samples wide, and as the row length
# ... and the full 2^20 the entry points take, on either axis
PLANES = [(65537, 1), (65537, 3), (65537, 8), (1, 65537), (1 << 20, 3), (1, 1 << 20)]
_ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def _rng(*key):
    return np.random.default_rng([0x4C4F4E47, *key])


@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_gaborish(ctx, oracle, shape):
    img = (_rng(1, *shape).random(shape, dtype=np.float32) + np.float32(0.5))
    want = oracle.gaborish(img, GAB_W1, GAB_W2)
    _tail_tells(want, _long_axis(shape))
    got = ctx.stage_gaborish(img, GAB_W1, GAB_W2)
    assert bit_equal(got, want), diff_report(got, want)


@pytest.mark.parametrize("stage", [0, 1, 2])
@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_epf(ctx, oracle, shape, stage):
    h, w = shape
    rng = _rng(2, stage, *shape)
    planes = [(rng.random(shape, dtype=np.float32) + np.float32(0.25)) * np.float32(s) for s in (0.05, 1.0, 1.0)]
    sig = -rng.uniform(0.05, 6.0, size=((h + 7) // 8, (w + 7) // 8)).astype(np.float32)  # incl. pass-through blocks
    want = oracle.epf(stage, oracle.default_params(w, h), planes, sig)
    for c in range(3):
        _tail_tells(want[c], _long_axis(shape))
    got = ctx.stage_epf(stage, ctx.default_params(w, h), planes, sig)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"epf{stage} ch{c}: {diff_report(got[c], want[c])}"


@pytest.mark.parametrize("shape", [(65537, 2), (65537, 3), (65537, 8), (3, 65537), (1, 65537)], ids=_ids)
def test_long_plane_lf_smoothing(ctx, oracle, shape):
    """k0b_lf_smooth on an LF image of 65 537 rows (a frame 524 296 pixels tall) and of 65 537 columns"""
    h, w = shape
    rng = _rng(3, *shape)
    # a slow wave plus noise small enough that the smoothing acts on part of the samples and not on others
    yy, xx = np.mgrid[0:h, 0:w]
    wave = 0.5 + 0.25 * np.sin(2 * np.pi * xx / 97) * np.cos(2 * np.pi * yy / 61)
    lf = [((wave + rng.random(shape) * a) * s).astype(np.float32) for a, s in ((0.0005, 0.02), (0.001, 1.0), (0.001, 1.0))]
    want = oracle.adaptive_lf_smoothing(oracle.default_params(w * 8, h * 8), lf)
    for c in range(3):
        _tail_tells(want[c], _long_axis(shape))
    if h > 2 and w > 2:
        changed = (want[1] != lf[1])[1:-1, 1:-1].mean()
        assert 0.05 < changed < 0.95, f"the smoothing acted on {changed:.0%} of the inner samples"
    got = ctx.stage_lf_smooth(ctx.default_params(w * 8, h * 8), lf)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"ch{c}: {diff_report(got[c], want[c])}"


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_modular_to_rgb8(ctx, oracle, shape, channels):
    planes = [_rng(4, c, *shape).integers(1, 256, size=shape).astype(np.int32) for c in range(3)]
    want = [np.asarray(oracle.i32_to_u8(planes[c], 1, 255)).reshape(shape) for c in range(3)]
    for c in range(3):
        _tail_tells(want[c], _long_axis(shape))
    got = ctx.modular_to_rgb8(planes, 1, 255, channels)
    for c in range(3):
        _same_samples(got[..., c], want[c], f"channel {c}")
    if channels == 4:
        assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("horizontal", [True, False], ids=["h", "v"])
@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_rct_row_strided(ctx, oracle, shape, horizontal, monkeypatch):
    """the RCT with a row pitch (one launch, rows strided inside the kernel) behind an unsqueeze step, on padded planes
    whose padding must survive: the route planes of 2^31 samples take, forced by JXLH_SEPARATE_RCT=1"""
    monkeypatch.setenv("JXLH_SEPARATE_RCT", "1")
    oh, ow = shape
    op, perm = 6, 1
    rng = _rng(5, horizontal, *shape)
    ah, aw = (oh, (ow + 1) // 2) if horizontal else ((oh + 1) // 2, ow)
    rh, rw = (oh, ow // 2) if horizontal else (oh // 2, ow)
    host = [(rng.integers(100, 3000, size=(ah, aw)).astype(np.int32),
             np.round(rng.laplace(0, 40, size=(rh, rw))).astype(np.int32)) for _ in range(3)]
    unsq = [oracle.unsqueeze_h(a, r, ow) if horizontal else oracle.unsqueeze_v(a, r, oh) for a, r in host]
    want = [np.asarray(p).reshape(oh, ow) for p in oracle.rct(unsq, op, perm)]
    for c in range(3):
        _tail_tells(want[c], _long_axis(shape))
    o_stride = ow + 7
    dev = [(DeviceArray(a), DeviceArray(r if r.size else np.zeros(1, np.int32)),
            DeviceArray(np.full((oh, o_stride), -55, np.int32))) for a, r in host]
    try:
        ctx.unsqueeze_rct(horizontal, [d[0].ptr for d in dev], [d[1].ptr for d in dev], [d[2].ptr for d in dev], ow, oh,
                          aw, max(rw, 1), o_stride, op, perm)
        ctx.sync()
        for c in range(3):
            got = dev[c][2].download(np.int32, oh * o_stride).reshape(oh, o_stride)
            _same_samples(got[:, :ow], want[c], f"channel {c}")
            assert (got[:, ow:] == -55).all()
    finally:
        for d in dev:
            for x in d:
                x.free()


def _palette_case(shape, nb):
    rng = _rng(6, nb, *shape)
    num_colors, num_deltas, bit_depth = 12, 5, 8
    pal = rng.integers(1, 1 << bit_depth, size=(nb, num_colors + num_deltas)).astype(np.int32)
    pal[:, :num_deltas] = rng.integers(-12, 13, size=(nb, num_deltas))   # delta entries are small steps
    idx = rng.integers(-8, num_colors + num_deltas + 100, size=shape).astype(np.int32)
    idx[rng.random(shape) < 0.5] = rng.integers(0, num_deltas + 2)       # plenty of predicted pixels
    idx[-1, -1] = num_deltas + 1   # the very last pixel is a plain colour (>= 1): never zero, see _tail_tells
    return idx, pal, num_colors, num_deltas, bit_depth


@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_delta_palette(ctx, oracle, shape):
    """257 row bands per channel (the bands sit in gridDim.y), gradient predictor"""
    idx, pal, nc, nd, bd = _palette_case(shape, 3)
    want = oracle.palette_delta(idx, pal, nc, nd, bd, 5)
    for c in range(3):
        _tail_tells(want[c], _long_axis(shape))
    _same_samples(ctx.palette_delta(idx, pal, nc, nd, bd, 5), want, "palette_delta")


@pytest.mark.parametrize("shape", PLANES, ids=_ids)
def test_long_plane_delta_palette_weighted(ctx, oracle, shape):
    idx, pal, nc, nd, bd = _palette_case(shape, 2)
    want = oracle.palette_delta_wp(idx, pal, nc, nd, 2, bd, WP_DEFAULT)
    for c in range(2):
        _tail_tells(want[c], _long_axis(shape))
    _same_samples(ctx.palette_delta_wp(idx, pal, nc, nd, bd, WP_DEFAULT), want, "palette_delta_wp")


@pytest.mark.parametrize("horizontal", [True, False], ids=["h", "v"])
@pytest.mark.parametrize("shape", PLANES + [(3, 65537), (8, 65537)], ids=_ids)
def test_long_plane_unsqueeze(ctx, oracle, shape, horizontal):
    """one squeeze step with the long axis as the line count and as the line length, in both directions"""
    h, w = shape
    rng = _rng(7, horizontal, *shape)
    ah, aw = (h, (w + 1) // 2) if horizontal else ((h + 1) // 2, w)
    rh, rw = (h, w // 2) if horizontal else (h // 2, w)
    avg = rng.integers(1000, 1256, size=(ah, aw)).astype(np.int32)
    res = np.round(rng.laplace(0, 30, size=(rh, rw))).astype(np.int32)
    want = oracle.unsqueeze_h(avg, res, w) if horizontal else oracle.unsqueeze_v(avg, res, h)
    _tail_tells(want, _long_axis(shape))
    _same_samples(ctx.unsqueeze(horizontal, avg, res, w, h), want, "unsqueeze")


# ------------------------------------------------------------------ launches that tile several rows per workgroup
# These reach workgroup row 65 536 at 2, 4 or 8 times the height: still inside the 2^20 the entry points take.
@pytest.mark.parametrize("n,rows_per_workgroup", [(8, 2), (4, 4), (2, 8)])
@pytest.mark.parametrize("w", [1, 3])
def test_long_plane_upsample(ctx, oracle, n, rows_per_workgroup, w):
    """k_upsample slides its 5x5 window down 2 (8x), 4 (4x) or 8 (2x) input rows per workgroup"""
    h = LONG * rows_per_workgroup + 3
    plane = _rng(8, n, w).standard_normal((h, w)).astype(np.float32)
    want = oracle.upsample(n, plane)
    assert want.shape == (h * n, w * n)
    _tail_tells(want, 0, LONG * rows_per_workgroup * n)
    ctx.set_upsampling_weights()
    got = ctx.stage_upsample(n, plane)
    assert bit_equal(got, want), diff_report(got, want)


@pytest.mark.parametrize("w", [1, 3])
def test_long_plane_noise_convolve(ctx, oracle, w):
    """k_noise_apply walks 8 rows per workgroup"""
    h = LONG * 8 + 1
    plane = _rng(9, w).uniform(1.0, 2.0, (h, w)).astype(np.float32)
    want = oracle.noise_convolve(plane)
    _tail_tells(want, 0, LONG * 8)
    got = ctx.stage_noise_convolve(plane)
    assert bit_equal(got, want), diff_report(got, want)


@pytest.mark.parametrize("horizontal", [True, False], ids=["h", "v"])
@pytest.mark.parametrize("w", [1, 3])
def test_long_plane_chroma_upsample(ctx, oracle, w, horizontal):
    """k_chroma_upsample takes 4 rows of the sub-sampled channel per workgroup"""
    h = LONG * 4 + 1
    plane = _rng(10, w).standard_normal((h, w)).astype(np.float32)
    want = oracle.chroma_upsample(plane, horizontal)
    _tail_tells(want, 0, LONG * 4 * (1 if horizontal else 2))
    got = ctx.stage_chroma_upsample(plane, horizontal)
    assert bit_equal(got, want), diff_report(got, want)
