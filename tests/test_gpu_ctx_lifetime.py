"""What a context holds goes with it (run with -m gpu on an MI355X): jxlh_live_resources counts the device buffers,
pinned blocks, events and streams the library holds through the owners of csrc/device_owned.h.  One context with three
slots is driven through everything that allocates lazily -- every coefficient transport, re-renders and LF-only groups,
marks, hand-overs and kernel timing, reference slots with a patch, a spline, a blend, an extra channel, an LF slot with
its preview, upsampling, a save and a read-out to the host, a Modular frame of group-local transforms and a squeeze
chain -- and after jxlh_ctx_destroy the four counts are back where they were.  Twice.

Frames are 264 x 264 (2 x 2 groups, a whole and a partial one on both axes).  The squeeze chain is 640 x 641, the
smallest size of tests/test_gpu_parity.py::test_unsqueeze_chain_dataflow_launch with levels in both directions: the
dataflow launch needs two streamed levels in a row, which a 264 x 264 image does not have; that it was taken shows in
the pinned block of its error word."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 264
LUM = (0.2627, 0.678, 0.0593)
_cache = {}


def _workload():
    from jxl_rs_amd import synth
    if "wl" not in _cache:
        _cache["wl"] = synth.make_vardct(W, H, mix=synth.MIX_ALL, seed=264, epf_iters=2)
    return _cache["wl"]


def _begin(ctx, wl, **over):
    from helpers import gpu_params_from
    ctx.frame_begin(gpu_params_from(ctx, wl, **over))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)


def _submit_slots(ctx, wl, groups, slot):
    from jxl_rs_amd import lib
    parts = [lib.host_pack_slots(wl.coeffs[g], group_id=g) for g in groups]
    assert all(len(q[3]) == 0 for q in parts)
    ctx.submit_groups_slots(np.asarray(groups, np.uint32), np.concatenate([q[0] for q in parts]),
                            np.concatenate([q[1].reshape(-1) for q in parts]), np.concatenate([q[2] for q in parts]), None,
                            slot=slot)
    ctx.slot_wait(slot)


def _submit_sparse8(ctx, wl, slot):
    from jxl_rs_amd import synth
    ng = wl.coeffs.shape[0]
    parts = [synth.to_sparse8(wl.coeffs[g]) for g in range(ng)]
    wide = []
    for g, q in enumerate(parts):  # the batched form addresses wide entries frame-wide
        if len(q[3]):
            e = q[3].copy()
            e[:, 0] += np.uint32(g * 3 * 65536)
            wide.append(e)
    ctx.submit_groups_sparse8(np.arange(ng, dtype=np.uint32), np.concatenate([q[0] for q in parts]),
                              np.concatenate([q[1] for q in parts]), np.concatenate([q[2] for q in parts]),
                              np.concatenate(wide) if wide else None, slot=slot)
    ctx.slot_wait(slot)


def drive(ctx, oracle, kat, at=lambda what: None):
    """everything that allocates lazily, on a context with three slots; at(what): called at the points the test looks
    at the counters"""
    from jxl_rs_amd import lib
    from jxl_rs_amd.modular import ModularChain
    wl = _workload()
    rng = np.random.default_rng(264)
    ng = wl.coeffs.shape[0]
    assert (wl.xgroups, wl.ygroups) == (2, 2)
    k = kat["output_stage"]
    xyb = oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, 255.0)
    # ---- dense slabs on slot 0, kernel timing on (its event pairs stay pending until the context goes): a reference
    # slot with a patch across the group edge, an extra channel, a spline; a whole run, then a re-render
    ctx.kernel_timing(True)
    ctx.set_reference(0, [rng.uniform(0, 1, (40, 50)).astype(np.float32) for _ in range(4)])
    _begin(ctx, wl)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(H, W)).astype(np.int32), 16)
    ctx.set_patches([(236, 250, 0, 3, 2, 26, 12)], [(lib.BLEND_ADD, 0, False), (lib.BLEND_ADD, 0, False)], [lib.EC_ALPHA])
    ctx.set_splines(np.float32([[250.0, 255.0, 6.0, 0.7, 0.3, 0.4, -0.3, 0.2]]))
    for g in range(ng):
        ctx.submit_group(g, wl.coeffs[g], slot=0)
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.rerender_groups([3])
    ctx.sync()
    assert ctx.read_extra_channel(0, W, H).shape == (H, W)
    ctx.kernel_timing(False)
    at("after the dense frame")  # (a pinned block by now: jxlh_ctx_sync's error word)
    # ---- sparse8 on slot 1 (the slot's staging), upsampling 2; a save and the 8-bit read-out to host memory
    _begin(ctx, wl, upsampling=2)
    _submit_sparse8(ctx, wl, 1)
    ctx.frame_run()
    ctx.sync()
    assert ctx.out_size == (2 * W, 2 * H)
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb, 0.0, LUM)
    assert ctx.frame_save(lib.save_desc([0, 1, 2], lib.SAVE_U16), colour).shape == (2 * H, 2 * W * 3)
    assert ctx.read_rgb8(xyb, 3).shape == (2 * H, 2 * W, 3)
    # ---- slot-bucketed on slot 2 in two consecutive frames (both entry sets and their fences); the first with an
    # LF-only group, a hand-over and a mark, blended onto a reference slot
    ctx.set_reference(1, [rng.uniform(0, 1, (280, 300)).astype(np.float32) for _ in range(3)])
    _begin(ctx, wl)
    ctx.set_groups_lf_only([3])
    _submit_slots(ctx, wl, [0, 1, 2], 2)
    ctx.wait_stream(None)
    ctx.frame_run()
    ctx.wait_mark(ctx.mark())
    ctx.rerender_groups([0])
    ctx.blend(lib.blend_desc(8, 4, 300, 280, (lib.BLEND_ADD, 0, False, 1)))
    ctx.sync()
    assert ctx.out_size == (300, 280)
    _begin(ctx, wl)
    _submit_slots(ctx, wl, list(range(ng)), 2)
    ctx.frame_run()
    ctx.sync()
    # ---- an LF slot and its preview
    ctx.set_lf_frame(0, *[rng.uniform(0, 0.5, (33, 33)).astype(np.float32) for _ in range(3)])
    assert ctx.lf_preview(0, W, H, lib.save_desc([0, 1, 2], lib.SAVE_U8), colour).shape == (H, W * 3)
    # ---- a Modular frame of group-local transforms from a host arena
    specs = [dict(x0=x0, y0=y0, n_channels=3, steps=[lib.local_rct(0, 7 + i)],
                  coded=[rng.integers(0, 64, size=(min(256, H - y0), min(256, W - x0))).astype(np.int32) for _ in range(3)])
             for i, (x0, y0) in enumerate([(0, 0), (256, 0), (0, 256), (256, 256)])]
    arena, groups = lib.pack_local_groups(specs)
    ctx.modular_frame_begin(ctx.default_params(W, H))
    ctx.set_modular_groups(arena, groups, 8, n=len(specs))
    ctx.frame_run()
    ctx.sync()
    assert len(ctx.read_planes()) == 3
    # ---- a squeeze chain long enough for the dataflow launch (its pinned error word appears)
    at("before the chain")
    ch = ModularChain(ctx, 640, 641, seed=3)
    try:
        ch.run_chain()
        ctx.sync()
    finally:
        ch.free()
    at("after the chain")


def test_context_releases_everything_it_held(oracle, kat):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    gc.collect()
    baseline = lib.live_resources()
    for cycle in range(2):
        seen = {}

        def at(what):
            seen[what] = now = lib.live_resources()
            assert all(n > b for n, b in zip(now, baseline)), (cycle, what, now, baseline)

        ctx = jxl_rs_amd.Context(0, 3)
        try:
            now = lib.live_resources()
            assert now[2] > baseline[2] and now[3] == baseline[3] + 4, (now, baseline)  # the main stream + three slots
            drive(ctx, oracle, kat, at)
            assert len(seen) == 3
            assert seen["after the chain"][1] == seen["before the chain"][1] + 1, "the chain did not take the dataflow launch"
        finally:
            ctx.close()
        gc.collect()
        assert lib.live_resources() == baseline, cycle
