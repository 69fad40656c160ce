"""Splines on the device (k_splines.hip) held bit for bit to the fused CPU restatement of the reference
(tests/splines_ref.py): through the stage hook -- the per-pixel rule's corner cases, bin edges, order of accumulation,
batches, long axes -- and inside whole VarDCT frames (after patches, before upsampling and noise; repeated, banded and
partial renders; saved references; the output stage), plus the validation of jxlh_frame_set_splines."""
import json
import os

import numpy as np
import pytest

import patches_ref as pr
import splines_ref
from helpers import bit_equal, diff_report, run_oracle_frame, upload_frame
from jxl_rs_amd import lib

pytestmark = pytest.mark.gpu

F = np.float32
BIN_W, BIN_H = lib.splines_bin_layout()  # the draw's bin (csrc/splines_host.h)


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref():
    return splines_ref.Ref(fused=True)


@pytest.fixture(scope="module")
def spline(ref):
    """the consistency test's spline as segments"""
    seg = ref.build([splines_ref.CONSISTENCY_SPLINE], **splines_ref.CONSISTENCY_ARGS)
    assert seg is not None and seg.shape[0] > 500
    return seg


def _begin(ctx, w, h):
    ctx.frame_begin(ctx.default_params(w, h))


def _base(rng, h, w, row=None):
    """three planes uniform(-0.5, 1.5) with some -0.0; with `row` > w the columns beyond w hold a poison value"""
    out = []
    for _ in range(3):
        a = rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32)
        a[rng.random((h, w)) < 0.05] = -0.0
        if row is not None:
            big = np.full((h, row), np.float32(-7.25e33), np.float32)
            big[:, :w] = a
            a = big
        out.append(a)
    return out


def _assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


def _seg(cx, cy, md, inv_sigma=0.7, s4i=0.3, color=(0.4, -0.3, 0.2)):
    return [cx, cy, md, inv_sigma, s4i, *color]


def _hand_made(w, h):
    nan = float("nan")
    segs = [
        _seg(40.0, 50.0, 0.0), _seg(41.0, 50.0, 0.4), _seg(150.0, 100.0, 90.0, 0.05, 2.0), _seg(200.5, 30.5, 7.0),
        _seg(63.5, 3.5, 2.5), _seg(64.5, 4.5, 2.5), _seg(10.0, 200.0, 12.0, -0.4, -0.5), _seg(12.0, 201.0, 12.0, -0.4, 0.5),
        # outside each of the four edges: partly, and wholly
        _seg(-3.0, 60.0, 8.0), _seg(w + 2.0, 60.0, 8.0), _seg(100.0, -3.0, 8.0), _seg(100.0, h + 2.0, 8.0),
        _seg(-50.0, 120.0, 6.0), _seg(w + 50.0, 120.0, 6.0), _seg(220.0, -50.0, 6.0), _seg(220.0, h + 50.0, 6.0),
        _seg(w - 1.0, h - 1.0, 3.0), _seg(0.0, 0.0, 3.0),
        # a distance that is not a number: pixel (0, 0) only
        _seg(120.0, 80.0, nan),
        _seg(5.0, 5.0, 20.0, 0.2, 1.0, (1e3, -1e-3, 1.0)),
    ]
    return F(segs)


# ---------------------------------------------------------------- stage hook
def test_stage_hook_rule_and_padding(ctx, ref, spline):
    w, h, row = 300, 220, 320
    rng = np.random.default_rng(300)
    base = _base(rng, h, w, row)
    segs = np.concatenate([spline, _hand_made(w, h), spline[::7]])
    _begin(ctx, w, h)
    ctx.set_splines(segs)
    got = ctx.stage_splines(base, w=w)
    want = ref.draw(base, segs, w=w)
    _assert_planes(got, want, "stage hook")
    for c in range(3):
        assert bit_equal(got[c][:, w:], base[c][:, w:]), "padding was touched"
        assert not bit_equal(got[c][:, :w], base[c][:, :w])
        # an untouched -0.0 is still one
        untouched = want[c][:, :w].view(np.uint32) == base[c][:, :w].view(np.uint32)
        assert (untouched & (base[c][:, :w].view(np.uint32) == 0x80000000)).any()
    # the rule's corner cases one by one, on planes of -0.0 (a touched pixel loses its sign or gains a value)
    zero = [np.full((h, w), -0.0, np.float32) for _ in range(3)]
    for s, cols, rows in ((_seg(-50.0, 120.0, 6.0), {0}, set(range(114, 127))), (_seg(220.0, -50.0, 6.0), set(), set()),
                          (_seg(120.0, 80.0, float("nan")), {0}, {0}), (_seg(w + 50.0, 120.0, 6.0), set(), set()),
                          (_seg(220.0, h + 50.0, 6.0), set(), set())):
        ctx.set_splines(F([s]))
        g = ctx.stage_splines(zero)
        _assert_planes(g, ref.draw(zero, F([s])), "corner case %r" % (s,))
        hit = np.argwhere(g[0].view(np.uint32) != 0x80000000)
        assert set(hit[:, 1]) == cols and set(hit[:, 0]) == rows, (s, hit)
    # no segments: nothing happens
    ctx.set_splines(np.zeros((0, 8), np.float32))
    _assert_planes(ctx.stage_splines(base, w=w), base, "no segments")


@pytest.mark.parametrize("w,h", [(1, 1)] + [(BIN_W + dx, BIN_H + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)]
                         + [(2 * BIN_W + 1, 3 * BIN_H - 1)])
def test_bin_edges(ctx, ref, w, h):
    rng = np.random.default_rng(w * 100 + h)
    base = _base(rng, h, w)
    segs = []
    for cy in (0.0, BIN_H - 1.0, BIN_H - 0.5, float(BIN_H), 2.0 * BIN_H, h - 1.0):
        for cx in (0.0, BIN_W - 1.0, BIN_W - 0.5, float(BIN_W), 2.0 * BIN_W, w - 1.0):
            for md in (0.0, 0.5, 1.0, 2.6):
                segs.append(_seg(cx, cy, md, 0.9, 0.25 * (1 + len(segs) % 3), (0.5, -0.25, 0.125)))
    segs = F(segs)
    _begin(ctx, w, h)
    ctx.set_splines(segs)
    _assert_planes(ctx.stage_splines(base), ref.draw(base, segs), "%d x %d" % (w, h))


@pytest.fixture(scope="module")
def order_case():
    rng = np.random.default_rng(16)
    n = 240
    mag = 10.0 ** rng.uniform(-3, 3, n)
    sign = np.where(np.arange(n) & 1, -1.0, 1.0)
    segs = np.zeros((n, 8), np.float32)
    segs[:, 0] = 100.0 + rng.uniform(0, 16, n)
    segs[:, 1] = 50.0 + rng.uniform(0, 16, n)
    segs[:, 2] = rng.uniform(4, 14, n)
    segs[:, 3] = rng.uniform(0.1, 0.6, n)
    segs[:, 4] = rng.uniform(0.2, 1.0, n)
    for c in range(3):
        segs[:, 5 + c] = (sign * np.roll(mag, c)).astype(np.float32)
    return segs, _base(rng, 120, 200)


def test_order_of_accumulation(ctx, ref, order_case):
    segs, base = order_case
    want = ref.draw(base, segs)
    rev = ref.draw(base, segs[::-1])
    region = (slice(50, 66), slice(100, 116))
    assert any(not bit_equal(a[region], b[region]) for a, b in zip(want, rev)), "the order does not show on the CPU"
    _begin(ctx, 200, 120)
    ctx.set_splines(segs)
    _assert_planes(ctx.stage_splines(base), want, "ascending segment index")
    ctx.set_splines(segs[::-1])
    _assert_planes(ctx.stage_splines(base), rev, "reversed list")


def test_batches_give_the_same_bits(ctx, ref, spline, order_case):
    w, h = 300, 220
    rng = np.random.default_rng(64)
    base = _base(rng, h, w)
    segs = np.concatenate([spline, _hand_made(w, h), order_case[0]])
    _begin(ctx, w, h)
    ctx.set_splines(segs)
    whole = ctx.stage_splines(base)
    _assert_planes(whole, ref.draw(base, segs), "default budget")
    try:
        for budget in (64, 1, 1000):  # (the md 90 segment alone has more than 64 entries)
            ctx.set_spline_batch_budget(budget)
            _assert_planes(ctx.stage_splines(base), whole, "budget %d" % budget)
            ctx.set_splines(segs)  # planned under the budget at the set call as well
            _assert_planes(ctx.stage_splines(base), whole, "budget %d, set again" % budget)
    finally:
        ctx.set_spline_batch_budget(0)


@pytest.mark.parametrize("w,h", [(8, 65544), (65544, 8)])
def test_long_axes(ctx, ref, w, h):
    rng = np.random.default_rng(h)
    base = _base(rng, h, w)
    segs = []
    for far in (0.0, 3.0, 9.5, 300.0):
        cx, cy = (4.0, h - 1.0 - far) if h > w else (w - 1.0 - far, 4.0)
        segs.append(_seg(cx, cy, 6.0))
    segs.append(_seg(w / 2.0, h / 2.0, 3.0))
    segs.append(_seg(2.0, 2.0, 3.0))
    segs.append(_seg(float(w), float(h), 5.0))
    segs = F(segs)
    _begin(ctx, w, h)
    ctx.set_splines(segs)
    got = ctx.stage_splines(base)
    _assert_planes(got, ref.draw(base, segs), "%d x %d" % (w, h))
    assert not bit_equal(got[0][-3:, -3:], base[0][-3:, -3:])


# ---------------------------------------------------------------- whole frames, 520 x 300 (3 x 2 groups, ragged)
W, H = 520, 300


def _frame_segments(spline):
    extra = [_seg(x, 256.0 - 3.0 + (x % 5), 9.0, 0.3, 0.4) for x in range(5, W, 37)]  # across the group-row edge
    extra += [_seg(255.5, 128.0, 30.0, -0.1, -1.0), _seg(W - 2.0, H - 2.0, 6.0), _seg(-20.0, 40.0, 5.0),
              _seg(300.0, 100.0, float("nan"))]
    return np.concatenate([spline, F(extra)])


@pytest.fixture(scope="module")
def frame(oracle, ref, spline):
    """the default-filter frame: workload, the oracle's planes, the segments, the planes with the segments drawn"""
    from jxl_rs_amd import synth
    wl = synth.make_vardct(W, H, mix=synth.MIX_D1, seed=52, epf_iters=2)
    col, _ = run_oracle_frame(oracle, wl)
    col = [np.ascontiguousarray(c) for c in col]
    segs = _frame_segments(spline)
    return wl, col, segs, ref.draw(col, segs)


def _render(ctx, wl, segs, **over):
    upload_frame(ctx, wl, **over)
    ctx.set_splines(segs)
    ctx.frame_run()
    ctx.sync()


def test_frame_default_filters_twice_and_output(ctx, oracle, frame):
    wl, col, segs, want = frame
    _render(ctx, wl, segs)
    _assert_planes(ctx.read_planes(), want, "frame with splines")
    assert any(not bit_equal(a, b) for a, b in zip(want, col))
    # jxlh_frame_read_output / _rgb8 see the drawn planes
    k = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")))["output_stage"]
    xp = oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, 255.0)
    rgb = oracle.xyb_to_rgb8(xp, want, W, H, 3)
    assert np.array_equal(ctx.read_rgb8(xp, 3), rgb)
    assert np.array_equal(ctx.read_output(xyb_params=xp), rgb)
    # a second run of the same frame adds once
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "second frame_run")


def test_frame_band_runs_and_rerender(ctx, frame):
    wl, _, segs, want = frame
    upload_frame(ctx, wl)
    ctx.set_splines(segs)
    ctx.frame_run(0, 1)
    ctx.frame_run(1, 2)
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "band runs 0..1, 1..2")
    ctx.frame_run()
    ctx.rerender_groups([0, 4, 5])
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "rerender_groups")
    ctx.rerender_groups([2])
    ctx.rerender_groups([2, 3])
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "rerender_groups again")


def test_frame_unfiltered_bands_and_rerender(ctx, oracle, ref, spline):
    """without a filter stage the result lives in the planes the transforms write: a re-render of some groups renders
    the frame again instead of adding to the other groups twice"""
    from jxl_rs_amd import synth
    wl = synth.make_vardct(W, H, mix=synth.MIX_D1, seed=53, epf_iters=0, gab=False)
    col, _ = run_oracle_frame(oracle, wl)
    segs = _frame_segments(spline)
    want = ref.draw([np.ascontiguousarray(c) for c in col], segs)
    _render(ctx, wl, segs)
    _assert_planes(ctx.read_planes(), want, "unfiltered frame")
    ctx.rerender_groups([1, 4])
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "unfiltered rerender_groups")
    upload_frame(ctx, wl)
    ctx.set_splines(segs)
    ctx.frame_run(0, 1)
    ctx.frame_run(1, 2)
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "unfiltered band runs")


def test_frame_with_patches_drawn_first(ctx, frame, ref):
    wl, col, segs, _ = frame
    rng = np.random.default_rng(9)
    refs = [[rng.uniform(-0.5, 1.5, (96, 128)).astype(np.float32) for _ in range(3)]]
    ctx.set_reference(0, refs[0])
    patches, blendings = [], []
    for _ in range(60):
        xs, ys = int(rng.integers(8, 64)), int(rng.integers(8, 48))
        patches.append((int(rng.integers(0, W - xs + 1)), int(rng.integers(0, H - ys + 1)), 0,
                        int(rng.integers(0, 128 - xs + 1)), int(rng.integers(0, 96 - ys + 1)), xs, ys))
        blendings.append((int(rng.choice([pr.REPLACE, pr.ADD, pr.MUL])), 0, False))
    patched = pr.apply_patches([c.copy() for c in col], patches, blendings, refs, [])
    want = ref.draw(patched, segs)
    # (a Replace patch over a spline would show the other order)
    other = pr.apply_patches(ref.draw(col, segs), patches, blendings, refs, [])
    assert any(not bit_equal(a, b) for a, b in zip(want, other))
    upload_frame(ctx, wl)
    ctx.set_splines(segs)
    ctx.set_patches(patches, blendings, [])
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "patches, then splines")
    ctx.clear_reference(0)


def test_frame_upsampled_with_noise(ctx, oracle, frame):
    """splines are drawn at the coded size, before Upsample2x and the noise"""
    wl, _, segs, drawn = frame
    lut = np.float32([0.02, 0.05, 0.1, 0.2, 0.15, 0.1, 0.05, 0.3])
    p = upload_frame(ctx, wl, upsampling=2, noise=1, visible_frame_index=1)
    for i in range(8):
        p.noise_lut[i] = float(lut[i])
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.set_splines(segs)
    ctx.frame_run()
    ctx.sync()
    up = [oracle.upsample(2, np.ascontiguousarray(q)) for q in drawn]
    rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(1, 0, 2 * W, 2 * H)]
    want = oracle.noise_add(lut, 0.0, 1.0, up, rnd)
    _assert_planes(ctx.read_planes(), want, "splines, upsampling, noise")


def test_frame_420_without_filters(ctx, oracle, ref, spline):
    """a sub-sampled frame with nothing but splines behind the transforms: the chroma is upsampled before the draw, and
    band runs render the whole frame (the band's halo would undo the neighbouring band's splines)"""
    from jxl_rs_amd import synth
    hs = vs = (1, 0, 1)
    wl = synth.make_vardct(W, H, mix=synth.MIX_8X8, seed=17, epf_iters=0, gab=False, hshift=hs, vshift=vs)
    col, _ = run_oracle_frame(oracle, wl)
    segs = _frame_segments(spline)
    want = ref.draw([np.ascontiguousarray(c) for c in col], segs)
    _render(ctx, wl, segs)
    _assert_planes(ctx.read_planes(), want, "4:2:0 whole frame")
    upload_frame(ctx, wl)
    ctx.set_splines(segs)
    ctx.frame_run(0, 1)
    ctx.frame_run(1, 2)
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "4:2:0 band runs")


def test_saved_reference_shows_the_spline(ctx, oracle, frame):
    from jxl_rs_amd import synth
    wl, _, segs, want = frame
    _render(ctx, wl, segs)
    ctx.save_reference(1)
    wl2 = synth.make_vardct(W, H, mix=synth.MIX_D1, seed=54, epf_iters=1)
    col2, _ = run_oracle_frame(oracle, wl2)
    patches = [(20, 200, 1, 20, 200, 400, 90), (0, 0, 1, 100, 10, 64, 64)]  # over the group-row edge's segments
    blendings = [(pr.REPLACE, 0, False), (pr.ADD, 0, False)]
    expect = pr.apply_patches([np.ascontiguousarray(c) for c in col2], patches, blendings, {1: want}, [])
    upload_frame(ctx, wl2)
    ctx.set_patches(patches, blendings, [])
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), expect, "patch from a slot saved with splines")
    ctx.clear_reference(1)


# ---------------------------------------------------------------- validation
def test_validation_and_clearing(ctx, frame):
    import ctypes as C

    import jxl_rs_amd
    from jxl_rs_amd import lib
    wl, col, segs, want = frame
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        assert fresh.try_set_splines(segs) == lib.ERR_BAD_STATE  # no frame begun
        assert fresh.try_set_splines(np.zeros((0, 8), np.float32)) == lib.ERR_BAD_STATE
    finally:
        fresh.close()
    upload_frame(ctx, wl)
    ctx.set_splines(segs)
    assert ctx.L.jxlh_frame_set_splines(ctx._ctx, None, 5) == lib.ERR_INVALID_ARGUMENT
    assert ctx.L.jxlh_frame_set_splines(None, None, 0) == lib.ERR_INVALID_ARGUMENT
    # the rejected call left the segments as they were
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "after a rejected call")
    # n = 0 clears
    ctx.set_splines(np.zeros((0, 8), np.float32))
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), col, "cleared with n = 0")
    # jxlh_frame_begin clears
    ctx.set_splines(segs)
    upload_frame(ctx, wl)
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), col, "cleared by frame_begin")
    # the stage hook's arguments
    pl = [np.zeros((4, 8), np.float32) for _ in range(3)]
    pp = (C.c_void_p * 3)(*[a.ctypes.data for a in pl])
    ctx.set_splines(segs)
    assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, 8, 4, 7) == lib.ERR_INVALID_ARGUMENT  # stride < w
    assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, 0, 4, 8) == lib.ERR_INVALID_ARGUMENT
    assert ctx.L.jxlh_stage_splines(ctx._ctx, None, 8, 4, 8) == lib.ERR_INVALID_ARGUMENT
    # an axis of 2147483520 or more (where a float bound no longer maps one to one): refused, nothing is read
    assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, 2147483520, 1, 2147483520) == lib.ERR_UNSUPPORTED
    assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, 1, 2147483520, 1) == lib.ERR_UNSUPPORTED
    pp[1] = None
    assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, 8, 4, 8) == lib.ERR_INVALID_ARGUMENT


def test_stage_hook_takes_device_planes(ctx, ref, spline):
    from jxl_rs_amd.lib import DeviceArray
    w, h = 300, 220
    rng = np.random.default_rng(301)
    base = _base(rng, h, w)
    _begin(ctx, w, h)
    ctx.set_splines(spline)
    dev = [DeviceArray(a) for a in base]
    try:
        import ctypes as C
        pp = (C.c_void_p * 3)(*[d.ptr for d in dev])
        assert ctx.L.jxlh_stage_splines(ctx._ctx, pp, w, h, w) == 0
        got = [d.download(np.float32, w * h).reshape(h, w) for d in dev]
    finally:
        for d in dev:
            d.free()
    _assert_planes(got, ref.draw(base, spline), "device planes")


def test_sharded_frame_with_splines_is_unsupported(frame):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    wl, _, segs, _ = frame
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            upload_frame(c, wl)
            c.set_splines(segs)
        with pytest.raises(lib.JxlHipError) as e:
            lib.frames_run_sharded_local(peers)
        assert e.value.status == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
