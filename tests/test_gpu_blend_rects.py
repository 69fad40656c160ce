"""Blend rectangles on the device (include/jxl_hip_blend_rects.h, k_blend_rects.hip; run with -m gpu on an MI355X):
jxlh_stage_blend_rects' exact write set on poisoned planes, and jxlh_frame_blend_rects after every kind of re-render.
Every comparison is bit for bit; what is expected inside the rects is blending_ref.blend_frame of the oracle's NEW frame,
what is expected outside them is the OLD composition (or the poison).  The cases are tests/blend_rects_cases.py's, which
tests/test_blend_rects_cpu.py holds to the non-vacuity rules: none of these tests can pass by writing nothing."""
import ctypes as C

import numpy as np
import pytest

import blend_rects_cases as bc
import blending_ref as br
import repaint_ref as rr
import test_gpu_blending as tb
from helpers import upload_frame
from test_gpu_patches import EC_SETS

pytestmark = pytest.mark.gpu

ASSOC = bc.ALPHA | tb.ASSOC
# test_gpu_blending's sets hold up to two extra channels: with these every instantiation of the kernel (0..8) runs
MORE_EC_SETS = [[0, bc.ALPHA, 0], [bc.ALPHA, 0, ASSOC, 0], [0, 0, bc.ALPHA, 0, ASSOC], [bc.ALPHA, 0, 0, ASSOC, 0, 0],
                [0, ASSOC, 0, 0, 0, bc.ALPHA, 0], [0, bc.ALPHA, 0, ASSOC, 0, 0, bc.ALPHA, 0]]
ALL_EC_SETS = EC_SETS + MORE_EC_SETS


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits(got, want, what):
    assert len(got) == len(want), what
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        bad = np.argwhere(bits(g) != bits(e))
        assert not len(bad), f"{what}: channel {c}: {len(bad)} samples differ, first (y, x) {bad[:4].tolist()}"


def patched(old, new, rects):
    """the old planes with the pixels of the rects' union taken from the new ones"""
    h, w = old[0].shape
    m = bc.union_mask(rects, w, h)
    return [np.where(m, n, o) for o, n in zip(old, new)]


# ---------------------------------------------------------------- the stage hook: the exact write set
def _stage_case(ctx, flags, device):
    from jxl_rs_amd import lib
    num_ec = len(flags)
    nch = 3 + num_ec
    rng = np.random.default_rng(211 + 7 * num_ec + sum(flags))
    (iw, ih), (fw, fh) = bc.STAGE_IMAGE, bc.STAGE_FRAME
    refs = {s: tb._planes(rng, nch, ih + s, iw + 3 * s) for s in range(3)}  # slot 3 is never set
    for r in refs.values():
        tb._zero_alpha_patch(r, num_ec)
    tb._set_slots(ctx, refs)
    stride = 520 if device else iw  # device rows must be 16-byte aligned to be written in place
    pois = bc.poison(nch, ih, stride)
    dev = [lib.DeviceArray(p) for p in pois] if device else None
    try:
        for k, (color, ec) in enumerate(tb._mode_grid(num_ec)):
            x0, y0 = bc.STAGE_ORIGINS[k % len(bc.STAGE_ORIGINS)]
            frame = tb._planes(rng, nch, fh, fw)
            tb._zero_alpha_patch(frame, num_ec)
            d = br.BlendDesc(x0, y0, iw, ih, color, ec, flags)
            want = br.blend_frame(frame, refs, d)
            tb._assert_finite(want)
            rects = bc.stage_rects(x0, y0)
            mask = bc.union_mask(rects, iw, ih)
            if device:
                for a, p in zip(dev, pois):
                    a.upload(p)
                ctx.stage_blend_rects(tb._lib_desc(d), frame, rects, [a.ptr for a in dev], out_stride=stride)
                got = [a.download(np.float32, ih * stride).reshape(ih, stride) for a in dev]
            else:
                got = ctx.stage_blend_rects(tb._lib_desc(d), frame, rects, [p.copy() for p in pois])
            exp = [p.copy() for p in pois]
            for c in range(nch):
                exp[c][:, :iw][mask] = want[c][mask]
            assert_bits(got, exp, f"{'device' if device else 'host'} planes, {color} {ec} at {(x0, y0)}")
    finally:
        for a in dev or []:
            a.free()


@pytest.mark.parametrize("flags", ALL_EC_SETS, ids=["ec%d_%s" % (len(f), "_".join(map(str, f))) for f in ALL_EC_SETS])
def test_stage_hook_writes_exactly_the_union_device_planes(ctx, flags):
    _stage_case(ctx, flags, True)


@pytest.mark.parametrize("flags", ALL_EC_SETS, ids=["ec%d_%s" % (len(f), "_".join(map(str, f))) for f in ALL_EC_SETS])
def test_stage_hook_writes_exactly_the_union_host_planes(ctx, flags):
    _stage_case(ctx, flags, False)


def test_stage_hook_4096_rects_of_one_pixel(ctx):
    from jxl_rs_amd import lib
    rng = np.random.default_rng(4096)
    (iw, ih), (fw, fh) = bc.STAGE_IMAGE, bc.STAGE_FRAME
    refs = {0: tb._planes(rng, 4, ih, iw)}
    tb._set_slots(ctx, refs)
    frame = tb._planes(rng, 4, fh, fw)
    d = br.BlendDesc(1, 1, iw, ih, (br.BLEND, 0, True, 0), [(br.BLEND, 0, False, 0)], [bc.ALPHA])
    want = br.blend_frame(frame, refs, d)
    rects = [(k % iw, k // iw, 1, 1) for k in ((i * 1381) % (iw * ih) for i in range(lib.MAX_SAVE_RECTS))]  # all distinct
    pois = bc.poison(4, ih, iw)
    got = ctx.stage_blend_rects(tb._lib_desc(d), frame, rects, [p.copy() for p in pois])
    mask = bc.union_mask(rects, iw, ih)
    assert mask.sum() == lib.MAX_SAVE_RECTS < iw * ih
    assert_bits(got, [np.where(mask, w, p) for w, p in zip(want, pois)], "4096 rects of 1 x 1")


# ---------------------------------------------------------------- frames
def render(ctx, wl, desc, ec_seed=5, **over):
    upload_frame(ctx, wl, **over)
    for i in range(len(desc.ec)):
        ctx.set_extra_channel(i, bc.ec_samples(ec_seed + i, wl.xsize, wl.ysize), 16)
    ctx.frame_run()


def save_desc(desc):
    from jxl_rs_amd import lib
    return lib.save_desc([0, 1, 2] + ([3] if desc.ec else []), lib.SAVE_U8)


@pytest.mark.parametrize("case", list(bc.DESCS))
def test_vardct_rerender_then_blend_rects(ctx, oracle, case):
    """render, blend, one group arrives again, rerender_groups, changed_rects, blend_image_rects, blend_rects: the whole
    image is the composition of the oracle's new frame; save_rects of the same list repaints the first paint"""
    from jxl_rs_amd import lib
    d = bc.DESCS[case]
    ld = tb._lib_desc(d)
    a, b = bc.workloads()
    fa, fab, _ = bc.frames(oracle)
    refs = {0: bc.slot_planes(11, 3 + len(d.ec))}
    tb._set_slots(ctx, refs)
    render(ctx, a, d)
    ctx.blend(ld)
    first = br.blend_frame(bc.with_ec(oracle, fa, d), refs, d)
    assert_bits(tb._read_all(ctx, len(d.ec)), first, "the first composition")
    paint = ctx.frame_save(save_desc(d))
    ctx.submit_group(bc.GROUP, b.coeffs[bc.GROUP])
    ctx.slot_wait(0)
    ctx.rerender_groups([bc.GROUP])
    assert ctx.out_size == bc.FRAME  # the render points the result back at the frame's own planes
    rects = ctx.changed_rects([bc.GROUP])
    image_rects = lib.blend_image_rects(ld, *bc.FRAME, rects)
    assert image_rects.tolist() == [list(r) for r in bc.frame_rects(d, *bc.FRAME, rects)] and len(image_rects) == 1
    ctx.blend_rects(ld, image_rects)
    assert ctx.out_size == bc.IMAGE
    want = br.blend_frame(bc.with_ec(oracle, fab, d), refs, d)
    tb._assert_finite(want)
    assert_bits(tb._read_all(ctx, len(d.ec)), want, "after blend_rects")
    before = paint.copy()
    ctx.frame_save_rects(save_desc(d), image_rects, out=paint)
    assert not np.array_equal(paint, before)
    assert np.array_equal(paint, ctx.frame_save(save_desc(d)))
    # idempotence: again, then the whole blend: the same canvas; save_reference copies the recomposed canvas
    ctx.blend_rects(ld, image_rects)
    assert_bits(tb._read_all(ctx, len(d.ec)), want, "blend_rects twice")
    ctx.blend(ld)
    assert_bits(tb._read_all(ctx, len(d.ec)), want, "a whole blend after blend_rects")
    ctx.blend_rects(ld, image_rects)
    ctx.save_reference(3)
    assert_bits(tb._slot_contents(ctx, 3, 3 + len(d.ec), *bc.IMAGE), want, "save_reference after blend_rects")
    ctx.clear_reference(3)


def test_stale_outside_the_rects(ctx, oracle):
    """after a blend the whole frame runs on other coefficients and the source slot is replaced (so that both sides of the
    frame's edge change): inside the union of the hand-picked rects the new composition, outside it the old one"""
    d = bc.DESCS["blend_alpha"]
    ld = tb._lib_desc(d)
    a, b = bc.workloads()
    fa, _, fb = bc.frames(oracle)
    s1, s2 = bc.slot_planes(11, 4), bc.slot_planes(12, 4)
    tb._set_slots(ctx, {0: s1})
    render(ctx, a, d)
    ctx.blend(ld)
    old = br.blend_frame(bc.with_ec(oracle, fa, d), {0: s1}, d)
    for g in range(b.coeffs.shape[0]):
        ctx.submit_group(g, b.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.set_reference(0, s2)
    ctx.blend_rects(ld, bc.STALE_RECTS)
    new = br.blend_frame(bc.with_ec(oracle, fb, d), {0: s2}, d)
    tb._assert_finite(new)
    assert_bits(tb._read_all(ctx, 1), patched(old, new, bc.STALE_RECTS), "new inside the union, old outside")


def test_stale_outside_extend_only_rects(ctx, oracle):
    """only the source slot is replaced, and only rects outside the frame are composed again"""
    d = bc.DESCS["blend_alpha"]
    ld = tb._lib_desc(d)
    a, _ = bc.workloads()
    fa, _, _ = bc.frames(oracle)
    s1, s2 = bc.slot_planes(11, 4), bc.slot_planes(12, 4)
    tb._set_slots(ctx, {0: s1})
    render(ctx, a, d)
    ctx.blend(ld)
    old = br.blend_frame(bc.with_ec(oracle, fa, d), {0: s1}, d)
    ctx.set_reference(0, s2)
    ctx.blend_rects(ld, bc.EXTEND_RECTS)  # the canvas is still the result: no render in between
    new = br.blend_frame(bc.with_ec(oracle, fa, d), {0: s2}, d)
    assert_bits(tb._read_all(ctx, 1), patched(old, new, bc.EXTEND_RECTS), "the new slot inside the union only")


def test_upsampled_frame_repaint_groups(ctx, oracle):
    from jxl_rs_amd import lib
    d, n = bc.UPS_DESC, bc.UPS_N
    ld = tb._lib_desc(d)
    a, b = bc.ups_workloads()
    before, after = bc.ups_frames(oracle)
    fw, fh = bc.UPS_CODED[0] * n, bc.UPS_CODED[1] * n
    refs = {2: bc.slot_planes(13, 3, (d.image_w, d.image_h))}
    tb._set_slots(ctx, refs)
    upload_frame(ctx, a, upsampling=n)
    ctx.frame_run()
    ctx.blend(ld)
    old = br.blend_frame(before, refs, d)
    assert_bits(tb._read_all(ctx, 0), old, "the first composition")
    ctx.submit_group(bc.UPS_GROUP, b.coeffs[bc.UPS_GROUP])
    ctx.slot_wait(0)
    ctx.repaint_groups([bc.UPS_GROUP])
    image_rects = lib.blend_image_rects(ld, fw, fh, ctx.repaint_changed_rects([bc.UPS_GROUP]))
    assert len(image_rects) == 1
    ctx.blend_rects(ld, image_rects)
    assert_bits(tb._read_all(ctx, 0), br.blend_frame(after, refs, d), "upsampled frame after blend_rects")


def test_modular_frame_by_cell(ctx, oracle):
    from jxl_rs_amd import lib
    d = bc.MOD_DESC
    ld = tb._lib_desc(d)
    w, h = bc.MOD_SIZE
    chans, cur, (x0, y0, x1, y1) = bc.mod_samples()
    before, after = bc.mod_frames(oracle)
    refs = {1: [p + np.float32(0.25) for p in bc.slot_planes(14, 3, (d.image_w, d.image_h))]}
    tb._set_slots(ctx, refs)
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters, p.upsampling, p.epf_sigma_for_modular = 1, 2, 1, rr.SIGMA_FOR_MODULAR
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*chans, 8)
    ctx.frame_run()
    ctx.blend(ld)
    assert_bits(tb._read_all(ctx, 0), br.blend_frame(before, refs, d), "the first composition")
    ctx.set_modular_channels(*[np.ascontiguousarray(c[y0:y1, x0:x1]) for c in cur], 8, x0=x0, y0=y0)
    ctx.repaint_groups([bc.MOD_CELL])
    image_rects = lib.blend_image_rects(ld, w, h, ctx.repaint_changed_rects([bc.MOD_CELL]))
    ctx.blend_rects(ld, image_rects)
    assert_bits(tb._read_all(ctx, 0), br.blend_frame(after, refs, d), "Modular frame after blend_rects")


def test_alpha_channel_delivered_by_rects(ctx, oracle):
    from jxl_rs_amd import lib
    d = bc.DESCS["blend_alpha"]
    ld = tb._lib_desc(d)
    a, _ = bc.workloads()
    fa, _, _ = bc.frames(oracle)
    w, h = bc.FRAME
    first, new = bc.ec_planes()
    refs = {0: bc.slot_planes(11, 4)}
    tb._set_slots(ctx, refs)
    upload_frame(ctx, a)
    ctx.begin_extra_channel(0, w, h, 16, 1)
    ctx.set_extra_channel_rects([(0, 0, 0, first)])
    ctx.frame_run()
    ctx.blend(ld)
    assert_bits(tb._read_all(ctx, 1), br.blend_frame(list(fa) + [oracle.modular_to_f32(first, 16, 0)], refs, d), "first")
    x0, y0, rw, rh = bc.EC_UPDATE
    ctx.set_extra_channel_rects([(0, x0, y0, new[y0:y0 + rh, x0:x0 + rw])])
    ctx.rerender_groups([0])  # finishes the channel's dirty tiles
    image_rects = lib.blend_image_rects(ld, w, h, lib.extra_channel_changed_rects(w, h, 1, w, h, [bc.EC_UPDATE]))
    assert len(image_rects) == 1
    ctx.blend_rects(ld, image_rects)
    assert_bits(tb._read_all(ctx, 1), br.blend_frame(list(fa) + [oracle.modular_to_f32(new, 16, 0)], refs, d),
                "after the alpha rect and blend_rects")


def test_colour_stage_in_front(ctx, oracle):
    """XYB to sRGB in f32 in front of the blend, against the oracle's colour stage, as
    test_gpu_blending.test_frame_colour_stage_in_front does"""
    from jxl_rs_amd import lib
    d = br.BlendDesc(*bc.ORIGIN, *bc.IMAGE, (br.ADD, 0, True, 0), [], [])
    ld = tb._lib_desc(d)
    a, b = bc.workloads()
    fa, fab, _ = bc.frames(oracle)
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", tb._xyb_params(oracle), 0.0, tb.LUM)
    refs = {0: bc.slot_planes(15, 3)}
    tb._set_slots(ctx, refs)
    upload_frame(ctx, a)
    ctx.frame_run()
    ctx.blend(ld, colour)
    assert_bits(tb._read_all(ctx, 0), br.blend_frame(tb._oracle_colour(oracle, fa, "xyb", "srgb", 0.0), refs, d), "first")
    ctx.submit_group(bc.GROUP, b.coeffs[bc.GROUP])
    ctx.slot_wait(0)
    ctx.rerender_groups([bc.GROUP])
    ctx.blend_rects(ld, lib.blend_image_rects(ld, *bc.FRAME, ctx.changed_rects([bc.GROUP])), colour)
    want = br.blend_frame(tb._oracle_colour(oracle, fab, "xyb", "srgb", 0.0), refs, d)
    tb._assert_finite(want)
    assert_bits(tb._read_all(ctx, 0), want, "sRGB in front, after blend_rects")


# ---------------------------------------------------------------- states and statuses
def test_states_and_statuses_leave_canvas_and_result(ctx, oracle):
    from jxl_rs_amd import lib
    BAD, INV = lib.ERR_BAD_STATE, lib.ERR_INVALID_ARGUMENT
    d = bc.DESCS["blend_alpha"]
    ld = tb._lib_desc(d)
    a, b = bc.workloads()
    fa, fab, _ = bc.frames(oracle)
    refs = {0: bc.slot_planes(11, 4)}
    tb._set_slots(ctx, refs)
    whole = [(0, 0, *bc.IMAGE)]
    frame_a = bc.with_ec(oracle, fa, d)
    old = br.blend_frame(frame_a, refs, d)
    # before any blend
    render(ctx, a, d)
    assert ctx.try_blend_rects(ld, whole) == BAD
    assert ctx.try_blend_rects(ld, []) == BAD
    assert ctx.out_size == bc.FRAME
    assert_bits(ctx.read_planes(), fa, "the frame's own planes are still the result")
    ctx.blend(ld)
    # jxlh_frame_begin forgets the composition
    render(ctx, a, d)
    assert ctx.try_blend_rects(ld, whole) == BAD
    ctx.blend(ld)
    assert_bits(tb._read_all(ctx, 1), old, "composed")

    def refused(st, status, what):
        assert st == status, (what, st)
        assert ctx.out_size == bc.IMAGE
        assert_bits(tb._read_all(ctx, 1), old, f"after the refused call ({what})")

    # a descriptor that differs in a field the blend reads
    for what, change in (("x0", dict(x0=d.x0 + 1)), ("y0", dict(y0=d.y0 - 1)), ("image_w", dict(image_w=d.image_w - 1)),
                         ("image_h", dict(image_h=d.image_h - 4)), ("a larger image", dict(image_w=d.image_w + 64, image_h=d.image_h + 9)),
                         ("mode", dict(color=(br.ADD, 0, True, 0))),
                         ("clamp", dict(color=(br.BLEND, 0, False, 0))), ("source", dict(color=(br.BLEND, 0, True, 3))),
                         ("ec mode", dict(ec=[(br.MUL, 0, False, 0)])), ("ec flags", dict(ec_flags=[0]))):
        refused(ctx.try_blend_rects(tb._lib_desc(d._replace(**change)), whole), INV, what)
    # ... and the colour stage
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", tb._xyb_params(oracle), 0.0, tb.LUM)
    refused(ctx.try_blend_rects(ld, whole, colour), INV, "a colour stage the composition was not made with")
    # what jxlh_frame_blend checks comes first, with its status
    refused(ctx.try_blend_rects(tb._lib_desc(d._replace(color=(5, 0, True, 0))), whole), INV, "mode > 4")
    refused(ctx.try_blend_rects(tb._lib_desc(d._replace(ec=[], ec_flags=[])), whole), INV, "num_ec != handed over")
    # the list's errors
    iw, ih = bc.IMAGE
    for what, rects in (("x0 outside", [(iw, 0, 1, 1)]), ("y0 outside", [(0, ih, 1, 1)]),
                        ("outside behind a good one", [(0, 0, 1, 1), (iw + 3, ih + 3, 2, 2)]),
                        ("x overflow", [(1, 1, 0xffffffff, 1)]), ("y overflow", [(1, 1, 1, 0xffffffff)]),
                        ("4097 rects", [(0, 0, 1, 1)] * (lib.MAX_SAVE_RECTS + 1))):
        refused(ctx.try_blend_rects(ld, rects), INV, what)
    refused(ctx.L.jxlh_frame_blend_rects(ctx._ctx, C.byref(ld), None, None, 1), INV, "rects == NULL with n > 0")
    assert ctx.L.jxlh_frame_blend_rects(None, C.byref(ld), None, None, 0) == INV
    assert ctx.L.jxlh_frame_blend_rects(ctx._ctx, None, None, None, 0) == INV
    # the same refusals while the result is the frame's own planes: canvas and result stay as they were
    ctx.submit_group(bc.GROUP, b.coeffs[bc.GROUP])
    ctx.slot_wait(0)
    ctx.rerender_groups([bc.GROUP])
    for st in (ctx.try_blend_rects(tb._lib_desc(d._replace(x0=d.x0 + 1)), whole), ctx.try_blend_rects(ld, [(iw, 0, 1, 1)])):
        assert st == INV and ctx.out_size == bc.FRAME
        assert_bits(ctx.read_planes(), fab, "the re-rendered frame is still the result")
    # n == 0 and a list of empty rects: nothing launched, the (stale) canvas is the result again
    for rects in ([], [(5, 5, 0, 3), (iw + 9, ih + 9, 0, 0)]):
        ctx.rerender_groups([bc.GROUP])
        assert ctx.out_size == bc.FRAME
        assert ctx.try_blend_rects(ld, rects) == lib.OK
        assert ctx.out_size == bc.IMAGE
        assert_bits(tb._read_all(ctx, 1), old, "the kept composition, untouched")
    # ... and the rects then bring it up to date
    ctx.blend_rects(ld, lib.blend_image_rects(ld, *bc.FRAME, ctx.changed_rects([bc.GROUP])))
    assert_bits(tb._read_all(ctx, 1), br.blend_frame(bc.with_ec(oracle, fab, d), refs, d), "brought up to date")


def test_stage_hook_statuses(ctx):
    from jxl_rs_amd import lib
    INV = lib.ERR_INVALID_ARGUMENT
    rng = np.random.default_rng(3)
    (iw, ih), (fw, fh) = bc.STAGE_IMAGE, bc.STAGE_FRAME
    tb._set_slots(ctx, {})
    frame = tb._planes(rng, 3, fh, fw)
    ld = tb._lib_desc(br.BlendDesc(1, 1, iw, ih, (br.ADD, 0, False, 0), [], []))
    pois = bc.poison(3, ih, iw)
    out = [p.copy() for p in pois]
    for rects in ([(iw, 0, 1, 1)], [(0, ih, 1, 1)], [(1, 1, 0xffffffff, 1)], [(0, 0, 1, 1)] * (lib.MAX_SAVE_RECTS + 1)):
        assert ctx.try_stage_blend_rects(ld, frame, rects, out) == INV
    assert ctx.try_stage_blend_rects(ld, frame + frame[:1], [(0, 0, 1, 1)], out) == INV  # n_channels != 3 + num_ec
    assert ctx.try_stage_blend_rects(ld, frame, [], out) == lib.OK
    assert ctx.try_stage_blend_rects(ld, frame, [(9, 9, 0, 0), (iw + 1, 0, 0, 5)], out) == lib.OK
    ctx.sync()
    assert_bits(out, pois, "refused and empty calls write nothing")


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        d = lib.blend_desc(0, 0, 300, 600, (lib.BLEND_REPLACE, 0, 0, 0))
        for c in peers:
            upload_frame(c, wl)
            assert c.try_blend_rects(d, [(0, 0, 10, 10)]) == lib.ERR_UNSUPPORTED
            assert c.try_blend_rects(d, []) == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
