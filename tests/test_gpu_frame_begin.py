"""jxlh_frame_begin as check, plan, commit (csrc/frame_plan.h, csrc/abi_frame.hip; run with -m gpu on an MI355X).

A begin the plan refuses must leave the context exactly as it was: the previous frame stays readable and can be run
again.  A begin that succeeds must start the per-frame state (FrameState, jxlh_ctx.h) from nothing, whatever the frames
before it used: a frame rendered behind frames that used every per-frame feature equals the same frame on a fresh
context, bit for bit and launch for launch.

The frames "A" that use every per-frame feature are a series of four on one context, not one frame: the library refuses
LF-only groups in a chroma-subsampled frame (jxlh_frame_set_groups_lf_only), patches and splines are drawn in place and so
rule out the deferred chroma upsampling, and the strip kernel needs a filter (run_plan.h)."""
import ctypes as C

import numpy as np
import pytest

import blending_ref as br
import patches_ref as pr
from helpers import bit_equal, diff_report, gpu_params_from, run_gpu_frame, run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu

STRIP = 4  # JXLH_FRAME_STRIP
W, H = 72, 40


def _assert_planes(got, want, what):
    assert len(got) == len(want), what
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


@pytest.fixture(scope="module")
def small():
    from jxl_rs_amd import synth
    return synth.make_vardct(W, H, mix=synth.MIX_D1, seed=3, epf_iters=2)


@pytest.fixture(scope="module")
def small_want(oracle, small):
    return run_oracle_frame(oracle, small)


@pytest.fixture(scope="module")
def frame_b():
    from jxl_rs_amd import synth
    return synth.make_vardct(264, 264, mix=synth.MIX_D1, seed=5, epf_iters=2)  # 2 x 2 groups


@pytest.fixture(scope="module")
def frame_b_want(oracle, frame_b):
    return run_oracle_frame(oracle, frame_b)


# ---------------------------------------------------------------- a refused begin changes nothing
def _refused(ctx, small):
    """(name, params, expected status) of begins the plan refuses: nothing is allocated for any of them"""
    from jxl_rs_amd import lib
    out = []
    p = ctx.default_params(8448, 84736)  # 33 x 331 = 10 923 groups: 32-bit coefficient indices
    out.append(("8448 x 84736 VarDCT", p, lib.ERR_UNSUPPORTED))
    p = ctx.default_params(32768, 32768)  # plane_elems = 2^30: 32-bit byte offsets
    p.flags |= lib.FRAME_MODULAR
    out.append(("32768 x 32768 Modular", p, lib.ERR_UNSUPPORTED))
    p = gpu_params_from(ctx, small)
    p.hshift[0] = 2
    out.append(("hshift[0] = 2", p, lib.ERR_INVALID_ARGUMENT))
    p = gpu_params_from(ctx, small)
    p.epf_iters = 4
    out.append(("epf_iters = 4", p, lib.ERR_INVALID_ARGUMENT))
    return out


def test_refused_begin_changes_nothing(small, small_want):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    want, want_lf = small_want
    ctx = jxl_rs_amd.Context(0, 1)
    try:
        planes, lf = run_gpu_frame(ctx, small)
        _assert_planes(planes, want, "the frame itself")
        _assert_planes(lf, want_lf, "the frame's LF image")
        for name, p, status in _refused(ctx, small):
            # (the C entry point directly: the wrapper's frame_begin keeps the new geometry for its read-outs)
            assert ctx.L.jxlh_frame_begin(ctx._ctx, C.byref(p)) == status, name
            # copies only, and the stride check fails if the geometry was overwritten
            got_lf = [np.zeros((small.yblocks, small.xblocks), np.float32) for _ in range(3)]
            st = ctx.L.jxlh_frame_read_lf(ctx._ctx, got_lf[0].ctypes.data, got_lf[1].ctypes.data, got_lf[2].ctypes.data,
                                          small.xblocks)
            assert st == lib.OK, f"read_lf after {name}: status {st}"
            _assert_planes(got_lf, lf, f"LF image after {name}")
            _assert_planes(ctx.read_planes(), planes, f"planes after {name}")
            ctx.frame_run()
            ctx.sync()
            _assert_planes(ctx.read_planes(), want, f"run again after {name}")
            _assert_planes(ctx.read_lf(), want_lf, f"LF image of the run after {name}")
    finally:
        ctx.close()


# ---------------------------------------------------------------- a frame starts from nothing
def _render_a_series(ctx):
    """Four 72 x 40 frames that between them use every per-frame feature; -> their read-outs, by name"""
    from jxl_rs_amd import synth
    out = {}
    rng = np.random.default_rng(72)
    # 4:2:0, no filter, nothing drawn: the chroma upsampling is deferred -- and left pending by the last run
    sub = (1, 0, 1)
    wl = synth.make_vardct(W, H, mix=synth.MIX_8X8, seed=7, epf_iters=0, gab=False, hshift=sub, vshift=sub)
    upload_frame(ctx, wl)
    ctx.frame_run()
    ctx.sync()
    out["lazy_rgb8"] = [ctx.read_ycbcr_rgb8(3)]
    out["lazy_planes"] = ctx.read_planes()
    ctx.frame_run()
    ctx.sync()
    # one patch from a reference slot, one spline, an extra channel upsampled 2x, the group marked LF-only, the strip
    # flag (no filter: not eligible), then blended onto a canvas
    iw, ih = 100, 60
    ref = [rng.uniform(-0.5, 1.5, (ih, iw)).astype(np.float32) for _ in range(4)]
    ctx.set_reference(1, ref)
    wl = synth.make_vardct(W, H, mix=synth.MIX_D1, seed=8, epf_iters=0, gab=False)
    upload_frame(ctx, wl, flags=STRIP)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(H // 2, W // 2)).astype(np.int32), 16, ec_upsampling=2)
    ctx.set_patches([(10, 5, 1, 3, 2, 24, 16)], [(pr.BLEND_ABOVE, 0, 1), (pr.ADD, 0, 0)], [pr.EC_ALPHA])
    ctx.set_splines(np.float32([[30.0, 20.0, 6.0, 0.7, 0.3, 0.4, -0.3, 0.2]]))
    ctx.set_groups_lf_only([0])
    ctx.frame_run()
    ctx.sync()
    out["drawn_planes"] = ctx.read_planes()
    out["drawn_ec"] = [ctx.read_extra_channel(0, W, H)]
    from jxl_rs_amd import lib
    ctx.blend(lib.blend_desc(11, 7, iw, ih, (br.BLEND, 0, True, 1), [(br.BLEND, 0, False, 1)], [pr.EC_ALPHA]))
    out["canvas"] = ctx.read_planes() + [ctx.read_extra_channel(0, iw, ih)]
    assert out["canvas"][0].shape == (ih, iw)
    # the strip kernel
    wl = synth.make_vardct(W, H, mix=synth.MIX_D1, seed=9, epf_iters=2, aligned=True)
    out["strip_planes"], _ = run_gpu_frame(ctx, wl, flags=STRIP)
    assert ctx.frame_path()[0], "the strip kernel did not run"
    # A': a Modular frame
    p = ctx.default_params(W, H)
    p.gab, p.epf_iters = 0, 0
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*[rng.integers(0, 256, size=(H, W)).astype(np.int32) for _ in range(3)], 8)
    ctx.frame_run()
    ctx.sync()
    out["modular_planes"] = ctx.read_planes()
    ctx.clear_reference(1)
    return out


def _render_b(ctx, wl):
    """-> (planes, launches per kernel timer)"""
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    planes, _ = run_gpu_frame(ctx, wl)
    counts = {k: n for k, (_, n) in ctx.kernel_times().items()}
    ctx.kernel_timing(False)
    return planes, counts


def test_frame_starts_from_nothing(frame_b, frame_b_want):
    import jxl_rs_amd
    want_b, _ = frame_b_want
    first, second = jxl_rs_amd.Context(0, 1), jxl_rs_amd.Context(0, 1)
    try:
        # A, A', then B: every buffer grows (72 x 40 -> 2 x 2 groups)
        a_fresh = _render_a_series(first)
        b_behind, counts_behind = _render_b(first, frame_b)
        _assert_planes(b_behind, want_b, "B behind A and A'")
        # B on a fresh context, then A and A' behind it
        b_fresh, counts_fresh = _render_b(second, frame_b)
        _assert_planes(b_fresh, want_b, "B on a fresh context")
        assert counts_fresh and counts_behind == counts_fresh
        a_behind = _render_a_series(second)
        assert sorted(a_behind) == sorted(a_fresh)
        for name in sorted(a_fresh):
            _assert_planes(a_behind[name], a_fresh[name], f"A behind B: {name}")
    finally:
        first.close()
        second.close()
