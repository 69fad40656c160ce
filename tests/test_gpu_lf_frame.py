"""LF frames on the device (run with -m gpu on an MI355X): the LF slots of the context (jxlh_ctx_set_lf_frame,
jxlh_frame_save_lf, jxlh_ctx_clear_lf_frame) and VarDCT frames that take a slot as their LF image
(jxlh_frame_set_lf_from_slot), against the host route through jxlh_frame_set_lf and against the oracle, bit for bit."""
import numpy as np
import pytest

from helpers import bit_equal, diff_report, gpu_params_from, run_oracle_frame, upload_frame
from lf_preview_ref import XYB_FACTORS, modular_xyb, render_modular_xyb

pytestmark = pytest.mark.gpu

# 8x8, 16x16, 16x8, 8x16 and the four AFV varblocks
MIX = {0: 0.40, 4: 0.15, 6: 0.10, 7: 0.10, 12: 0.06, 13: 0.06, 14: 0.06, 15: 0.07}
POISON = np.float32(np.nan)


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frame():
    """72 x 40: 9 x 5 blocks, Gaborish + two EPF iterations"""
    from jxl_rs_amd import synth
    return synth.make_vardct(72, 40, mix=MIX, seed=1, epf_iters=2)  # this seed tiles with every family of MIX


def lf_like(oracle, wl, seed):
    """LF planes (X, Y, B) at the workload's own level that adaptive LF smoothing would change: within 0.4 of a
    quantisation step around each channel's mean (the smoothing acts only where neighbours are less than a step apart),
    with one edge of 20 steps it leaves alone"""
    p = oracle.default_params(wl.xsize, wl.ysize)
    lf = oracle.dequant_lf(p, *wl.lf_q)
    step = [np.float32(65536.0 / p.global_scale / p.quant_lf * f) for f in p.lf_quant_factors]
    rng = np.random.default_rng(seed)
    out = [(np.float32(a.mean()) + rng.uniform(-0.4, 0.4, a.shape) * s).astype(np.float32) for a, s in zip(lf, step)]
    out[1][:, :3] += np.float32(20) * step[1]
    return out


@pytest.fixture(scope="module")
def lf(oracle, frame):
    return lf_like(oracle, frame, 11)


@pytest.fixture(scope="module")
def expected(oracle, frame, lf):
    """the oracle's frame on `lf` as it is, and with adaptive LF smoothing"""
    plain, _ = run_oracle_frame(oracle, frame, lf=lf, do_lf_smoothing=0)
    smoothed, _ = run_oracle_frame(oracle, frame, lf=lf, do_lf_smoothing=1)
    return plain, smoothed


def assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


def begin_from_slot(ctx, wl, slot, **over):
    """the frame with everything but its LF handed over, the LF taken from `slot`"""
    p = gpu_params_from(ctx, wl, **over)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_from_slot(slot)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)


def render_from_slot(ctx, wl, slot, **over):
    begin_from_slot(ctx, wl, slot, **over)
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes()


def render_host_route(ctx, wl, lf, **over):
    p = gpu_params_from(ctx, wl, **over)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf(*lf)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes()


# ---------------------------------------------------------------- a slot against the host route
@pytest.mark.parametrize("source", ["host", "host_strided", "device_strided"])
def test_slot_fed_frame_equals_the_host_route_and_the_oracle(ctx, oracle, frame, lf, expected, source):
    from jxl_rs_amd import lib
    if source == "host":
        ctx.set_lf_frame(2, *lf)
    else:
        big = [np.full((a.shape[0], a.shape[1] + 7), POISON, np.float32) for a in lf]
        for b, a in zip(big, lf):
            b[:, 3:3 + a.shape[1]] = a
        if source == "host_strided":
            ctx.set_lf_frame(2, *[b[:, 3:3 + lf[0].shape[1]] for b in big])
        else:
            dev = [lib.DeviceArray(b) for b in big]
            ctx.set_lf_frame(2, *[d.ptr + 3 * 4 for d in dev], w=lf[0].shape[1], h=lf[0].shape[0], stride=big[0].shape[1])
            for d in dev:
                d.free()
    begin_from_slot(ctx, frame, 2, do_lf_smoothing=0)
    assert_planes(ctx.read_lf(), lf, f"{source}: read_lf before the run")
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    assert_planes(ctx.read_lf(), lf, f"{source}: read_lf after the run")
    assert_planes(got, render_host_route(ctx, frame, lf, do_lf_smoothing=0), f"{source}: against jxlh_frame_set_lf")
    assert_planes(got, expected[0], f"{source}: against the oracle")
    ctx.clear_lf_frame(2)


def test_adaptive_lf_smoothing_is_not_run(ctx, frame, lf, expected):
    plain, smoothed = expected
    assert any(not bit_equal(a, b) for a, b in zip(plain, smoothed)), "smoothing changes nothing on this input"
    ctx.set_lf_frame(0, *lf)
    got = render_from_slot(ctx, frame, 0, do_lf_smoothing=1)
    assert_planes(got, plain, "do_lf_smoothing = 1 in the parameters")
    assert_planes(ctx.read_lf(), lf, "read_lf")
    # the host route with the same parameters does smooth: the flag is what tells the two apart
    assert_planes(render_host_route(ctx, frame, lf, do_lf_smoothing=1), smoothed, "host route, smoothed")
    ctx.clear_lf_frame(0)


def test_the_frame_keeps_a_copy_and_the_slot_survives_frame_begin(ctx, oracle, frame, lf, expected):
    from jxl_rs_amd import synth
    ctx.set_lf_frame(1, *lf)
    other = synth.make_vardct(40, 24, seed=3, epf_iters=1)
    upload_frame(ctx, other)  # another frame in between: jxlh_frame_begin leaves the slot alone
    ctx.frame_run()
    begin_from_slot(ctx, frame, 1)
    ctx.set_lf_frame(1, *[np.full_like(a, 1e6) for a in lf])  # overwritten ...
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_planes(), expected[0], "slot overwritten after set_lf_from_slot")
    ctx.clear_lf_frame(1)  # ... and cleared
    ctx.frame_run()
    ctx.sync()
    assert_planes(ctx.read_planes(), expected[0], "slot cleared, frame run again")
    assert_planes(ctx.read_lf(), lf, "read_lf")


# ---------------------------------------------------------------- chains on one context
def test_modular_lf_frame_feeds_the_vardct_frame(ctx, oracle, frame):
    chans = modular_xyb(np.random.default_rng(21), 9, 5)
    lf = oracle.modular_xyb_to_f32(*chans, np.float32(XYB_FACTORS))
    render_modular_xyb(ctx, chans)
    ctx.save_lf(0)  # lf_level 1
    got = render_from_slot(ctx, frame, 0)
    want, _ = run_oracle_frame(oracle, frame, lf=lf, do_lf_smoothing=0)
    assert_planes(ctx.read_lf(), lf, "the slot holds the Modular frame's planes")
    assert_planes(got, want, "Modular XYB frame -> slot 0 -> VarDCT frame")
    ctx.clear_lf_frame(0)


def test_two_level_chain(ctx, oracle, frame):
    from jxl_rs_amd import synth
    chans = modular_xyb(np.random.default_rng(22), 2, 1)
    lf2 = oracle.modular_xyb_to_f32(*chans, np.float32(XYB_FACTORS))
    mid = synth.make_vardct(9, 5, mix=synth.MIX_DCT8, seed=6, epf_iters=2)  # 2 x 1 blocks
    render_modular_xyb(ctx, chans)
    ctx.save_lf(1)  # lf_level 2
    got_mid = render_from_slot(ctx, mid, 1)  # lf_level 1 reads slot 1 ...
    want_mid, _ = run_oracle_frame(oracle, mid, lf=lf2, do_lf_smoothing=0)
    assert_planes(got_mid, want_mid, "the 9 x 5 VarDCT LF frame")
    ctx.save_lf(0)  # ... and saves into slot 0
    got = render_from_slot(ctx, frame, 0)
    want, _ = run_oracle_frame(oracle, frame, lf=want_mid, do_lf_smoothing=0)
    assert_planes(got, want, "2 x 1 -> slot 1 -> 9 x 5 -> slot 0 -> 72 x 40")
    for s in (0, 1):
        ctx.clear_lf_frame(s)


def test_bands_and_rerender_of_a_slot_fed_frame(ctx, oracle):
    """300 x 260 from a 38 x 33 slot: two group rows and columns"""
    from jxl_rs_amd import synth
    wl = synth.make_vardct(300, 260, mix=synth.MIX_D1, seed=42, epf_iters=2)
    lf = lf_like(oracle, wl, 12)
    want, _ = run_oracle_frame(oracle, wl, lf=lf, do_lf_smoothing=0)
    ctx.set_lf_frame(3, *lf)
    assert_planes(render_from_slot(ctx, wl, 3), want, "whole frame")
    ctx.rerender_groups([3, 0])
    ctx.rerender_groups([1, 2])
    ctx.sync()
    assert_planes(ctx.read_planes(), want, "after rerender_groups")
    for order in ((0, 1), (1, 0)):
        begin_from_slot(ctx, wl, 3)
        for r in order:
            ctx.frame_run(r, r + 1)
        ctx.sync()
        assert_planes(ctx.read_planes(), want, f"bands in order {order}")
    ctx.clear_lf_frame(3)


# ---------------------------------------------------------------- the post stages are part of what is saved
def test_save_lf_saves_the_post_stage_result(ctx):
    """patches, splines and Upsample2x in front of jxlh_frame_save_lf: the slot holds what read_planes returns (read back
    through the LF image of a frame begun at the slot's size in blocks)"""
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(31)
    wl = synth.make_vardct(20, 12, mix=synth.MIX_DCT8, seed=8, epf_iters=1)
    upload_frame(ctx, wl)
    ctx.frame_run()
    plain = ctx.read_planes()
    ctx.set_reference(0, [rng.uniform(-0.5, 1.5, (16, 32)).astype(np.float32) for _ in range(3)])
    upload_frame(ctx, wl, upsampling=2)
    ctx.set_patches([(3, 2, 0, 1, 1, 9, 7)], [(lib.PATCH_ADD, 0, 0)])
    ctx.set_splines(np.array([[12.0, 6.0, 6.0, 0.4, 0.5, 0.3, 0.2, 0.1], [5.0, 9.0, 4.0, 0.6, 0.4, 0.1, 0.3, 0.2]], np.float32))
    ctx.frame_run()
    ctx.sync()
    assert ctx.out_size == (40, 24)
    planes = ctx.read_planes()
    assert planes[0].shape == (24, 40) and plain[0].shape == (12, 20)
    ctx.save_lf(1)
    big = ctx.default_params(320, 192)  # 40 x 24 blocks
    ctx.frame_begin(big)
    ctx.set_lf_from_slot(1)
    assert_planes(ctx.read_lf(), planes, "slot against read_planes")
    ctx.clear_lf_frame(1)
    ctx.clear_reference(0)


# ---------------------------------------------------------------- state and argument errors
def test_state_and_argument_errors(ctx, frame, lf):
    from jxl_rs_amd import lib, synth
    INV, BAD, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_BAD_STATE, lib.ERR_UNSUPPORTED
    L = ctx.L
    h, w = lf[0].shape
    # jxlh_ctx_set_lf_frame
    assert ctx.try_set_lf_frame(4, *lf) == INV
    p = [a.ctypes.data for a in lf]
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, w, h, None, p[1], p[2], w) == INV
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, w, h, p[0], p[1], None, w) == INV
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, w, h, p[0], p[1], p[2], w - 1) == INV
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, 0, h, p[0], p[1], p[2], w) == INV
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, w, 0, p[0], p[1], p[2], w) == INV
    assert L.jxlh_ctx_set_lf_frame(ctx._ctx, 0, (1 << 20) + 1, 1, p[0], p[1], p[2], (1 << 20) + 1) == INV
    assert L.jxlh_ctx_clear_lf_frame(ctx._ctx, 4) == INV
    # jxlh_frame_set_lf_from_slot
    p0 = gpu_params_from(ctx, frame)
    ctx.frame_begin(p0)
    assert ctx.try_set_lf_from_slot(4) == INV
    assert ctx.try_set_lf_from_slot(0) == INV  # an unset slot (none of the refused calls above set it)
    ctx.set_lf_frame(0, *[a[:, :-1] for a in lf])
    assert ctx.try_set_lf_from_slot(0) == INV  # 8 x 5 against 9 x 5 blocks
    ctx.set_lf_frame(0, *lf)
    ctx.set_lf(*lf)
    assert ctx.try_set_lf_from_slot(0) == BAD  # after jxlh_frame_set_lf in the same frame
    ctx.frame_begin(p0)
    ctx.set_lf_quantized(*frame.lf_q)
    assert ctx.try_set_lf_from_slot(0) == BAD  # ... or jxlh_frame_set_lf_quantized
    ctx.frame_begin(p0)
    assert L.jxlh_frame_set_lf(ctx._ctx, 2, 1, 0, 3, p[0], p[1], p[2], w) == lib.OK  # a zero-sized rect writes nothing ...
    assert L.jxlh_frame_set_lf_quantized(ctx._ctx, 2, 1, 3, 0, p[0], p[1], p[2], w, 0) == lib.OK
    assert ctx.try_set_lf_from_slot(0) == lib.OK  # ... and does not lock the slot out
    assert L.jxlh_frame_set_lf(ctx._ctx, 0, 0, w, h, p[0], p[1], p[2], w) == BAD
    q = [np.ascontiguousarray(a, dtype=np.int32) for a in frame.lf_q]
    assert L.jxlh_frame_set_lf_quantized(ctx._ctx, 0, 0, w, h, q[0].ctypes.data, q[1].ctypes.data, q[2].ctypes.data, w, 0) == BAD
    assert all(bit_equal(a, b) for a, b in zip(ctx.read_lf(), lf))  # the refused calls changed nothing
    # a Modular frame, a chroma-subsampled frame
    mp = ctx.default_params(w, h)
    mp.gab, mp.epf_iters = 0, 0
    ctx.modular_frame_begin(mp)
    assert ctx.try_set_lf_from_slot(0) == BAD
    assert ctx.try_save_lf(1) == BAD  # before a render
    sub = synth.make_vardct(72, 40, mix=synth.MIX_8X8, seed=7, epf_iters=0, hshift=(1, 0, 1), vshift=(1, 0, 1))
    ctx.frame_begin(gpu_params_from(ctx, sub))
    assert ctx.try_set_lf_from_slot(0) == UNS
    # jxlh_frame_save_lf: before a render, after a band only, after a blend
    wl = synth.make_vardct(300, 260, mix=synth.MIX_D1, seed=42, epf_iters=2)
    upload_frame(ctx, wl)
    assert ctx.try_save_lf(4) == INV
    assert ctx.try_save_lf(1) == BAD
    ctx.frame_run(0, 1)
    assert ctx.try_save_lf(1) == BAD  # one band is no whole-frame render
    ctx.frame_run()
    assert ctx.try_save_lf(1) == lib.OK
    ctx.set_reference(0, [np.zeros((260, 300), np.float32) for _ in range(3)])
    ctx.blend(lib.blend_desc(0, 0, 300, 260, (lib.BLEND_REPLACE, 0, 0, 0)))
    assert ctx.try_save_lf(2) == BAD
    ctx.clear_reference(0)
    # outside a frame
    import jxl_rs_amd
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        fresh.set_lf_frame(0, *lf)
        assert fresh.try_set_lf_from_slot(0) == BAD
        assert fresh.try_save_lf(0) == BAD
    finally:
        fresh.close()
    for s in range(4):
        ctx.clear_lf_frame(s)


def test_sharded_context_is_unsupported(lf):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            assert c.try_set_lf_frame(0, *lf) == lib.ERR_UNSUPPORTED
            assert c.try_save_lf(0) == lib.ERR_UNSUPPORTED
            assert c.try_set_lf_from_slot(0) == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
