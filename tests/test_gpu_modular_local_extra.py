"""Group-local transforms with extra channels on the device (run with -m gpu on an MI355X):
jxlh_frame_set_modular_groups_extra[_async].  The inputs are tests/modular_local_extra_cases.py's (proved to tell mistakes
apart by tests/test_modular_local_extra_cpu.py); expected values are the committed oracle's transforms per group, fed
through the whole-plane setters jxlh_frame_set_modular_channels / jxlh_frame_set_extra_channel on a second context, and
the three-call route (jxlh_modular_local_transforms_squeeze into caller planes, jxlh_frame_set_modular_channels,
jxlh_frame_set_extra_channel_rects).  Every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import modular_local_extra_cases as ec
from helpers import bit_equal, diff_report, upload_frame

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other():
    """the context of the whole-plane route"""
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def pattern(w, h, k):
    """the canary: 8-bit samples that differ per plane"""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 7 + y * 13 + 31 * k + 5) % 251).astype(np.int32)


def _params(c, w, h):
    p = c.default_params(w, h)
    p.gab, p.epf_iters = 0, 0
    return p


def _dest(n_colour, ecs):
    from jxl_rs_amd import lib
    return lib.local_dest(n_colour, ecs, bit_depth=0 if n_colour else 8)


def _begin_modular(c, w, h, fmt, ecs, prefill, n_colour):
    """a Modular frame whose planes and extra channels hold the pattern (through the whole-plane setters) or nothing"""
    c.modular_frame_begin(_params(c, w, h))
    if prefill:
        if n_colour:
            c.set_modular_channels(*[pattern(w, h, 0 if n_colour == 1 else k) for k in range(3)], fmt)
        for e in ecs:
            c.set_extra_channel(e, pattern(w, h, 3 + e), 8)
    else:
        for e in ecs:
            c.begin_extra_channel(e, w, h, 8, 1)


def _call(c, specs, n_colour, ecs, fmt, device_arena=False, wait=True, mark=False):
    from jxl_rs_amd import lib
    arena, batch = lib.pack_local_squeeze_groups(specs)
    wp = [sp["wp"] for sp in specs]
    keep = lib.DeviceArray(arena) if device_arena else None
    try:
        c.set_modular_groups_extra(keep if keep else arena, batch, fmt if n_colour else 0, _dest(n_colour, ecs), wp=wp,
                                   n=len(specs), arena_samples=arena.size, wait=wait)
        if mark:
            c.wait_mark(c.mark())
        elif not wait:
            c.sync()
    finally:
        if keep:
            c.sync()
            keep.free()


def _full_planes(oracle, specs, w, h, n_colour, ecs, prefill, bits=8):
    """what the planes hold after the call: the pattern (or zero) outside the rects, the oracle's channels inside"""
    n = n_colour + len(ecs)
    ids = ([0] if n_colour == 1 else list(range(n_colour))) + [3 + e for e in ecs]
    full = [pattern(w, h, k) if prefill else np.zeros((h, w), np.int32) for k in ids]
    assert len(full) == n
    for sp in specs:
        for c, f in enumerate(ec.finished(oracle, sp, bits)):
            full[c][sp["y0"]:sp["y0"] + sp["h"], sp["x0"]:sp["x0"] + sp["w"]] = f
    return full


def _read(c, w, h, ecs, colour=True):
    return (c.read_planes() if colour else []) + [c.read_extra_channel(e, w, h) for e in ecs]


def _reference(other, oracle, specs, w, h, n_colour, ecs, fmt, prefill, bits=8):
    """the oracle's finished planes through jxlh_frame_set_modular_channels and jxlh_frame_set_extra_channel"""
    full = _full_planes(oracle, specs, w, h, n_colour, ecs, prefill, bits)
    other.modular_frame_begin(_params(other, w, h))
    if n_colour:
        colour = full[:n_colour] * 3 if n_colour == 1 else full[:3]
        other.set_modular_channels(*colour, fmt)
    else:  # the colour of an extra-only call is whatever the frame holds: the pattern
        other.set_modular_channels(*[pattern(w, h, k) for k in range(3)], fmt)
    for e, plane in zip(ecs, full[n_colour:]):
        other.set_extra_channel(e, plane, 8)
    other.frame_run()
    other.sync()
    return _read(other, w, h, ecs)


def _assert_planes(got, want, what):
    assert len(got) == len(want)
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: plane {c}: {diff_report(g, e)}"


def _new_route(ctx, specs, w, h, n_colour, ecs, fmt, prefill, **how):
    _begin_modular(ctx, w, h, fmt, ecs, prefill, n_colour)
    if not n_colour:
        ctx.set_modular_channels(*[pattern(w, h, k) for k in range(3)], fmt)
    _call(ctx, specs, n_colour, ecs, fmt, **how)
    ctx.frame_run()
    ctx.sync()
    return _read(ctx, w, h, ecs)


def _three_call_route(ctx, specs, w, h, ecs, fmt, prefill):
    """today's route for an RGBA frame: the stage-level call into four caller planes, a copy of three into the frame, a
    scatter of the fourth into the extra channel"""
    from jxl_rs_amd import lib
    arena, batch = lib.pack_local_squeeze_groups(specs)
    ids = [0, 1, 2, 3 + ecs[0]]
    outs = [lib.DeviceArray(pattern(w, h, k) if prefill else np.zeros((h, w), np.int32)) for k in ids]
    try:
        ctx.modular_local_transforms_squeeze(arena, batch, 8, outs, w, h, w, wp=[sp["wp"] for sp in specs], n=len(specs))
        _begin_modular(ctx, w, h, fmt, ecs, prefill, 3)
        ctx.set_modular_channels(outs[0], outs[1], outs[2], fmt, w=w, h=h, stride=w)
        descs = np.zeros(len(specs), dtype=lib.EC_RECT_DTYPE)
        for d, sp in zip(descs, specs):
            d["ec"], d["x0"], d["y0"], d["w"], d["h"] = ecs[0], sp["x0"], sp["y0"], sp["w"], sp["h"]
            d["offset"], d["stride"] = sp["y0"] * w + sp["x0"], w
        ctx.set_extra_channel_rects(descs, block=outs[3], n_samples=w * h)
        ctx.frame_run()
        ctx.sync()
        return _read(ctx, w, h, ecs)
    finally:
        for o in outs:
            o.free()


# ---------------------------------------------------------------- RGBA on both frames, every step list
_REFERENCE = {}


def _rgba_case(other, oracle, name, frame_name):
    """specs, and the reference's planes: computed once per (list, frame), shared and never modified"""
    key = (name, frame_name)
    if key not in _REFERENCE:
        frame = ec.ALIGNED if frame_name == "aligned" else ec.RAGGED
        w, h, _ = frame
        specs = ec.frame_specs(name, frame, 4)
        if frame_name == "ragged":
            specs = [sp for i, sp in enumerate(specs) if i != 5]  # one cell stays the pattern: a canary inside the frame too
        _REFERENCE[key] = (specs, _reference(other, oracle, specs, w, h, 3, [1], 8, frame_name == "ragged"))
    return _REFERENCE[key]


@pytest.mark.parametrize("frame_name", ["aligned", "ragged"])
@pytest.mark.parametrize("name", ec.lists_for(4))
def test_rgba_equals_the_whole_plane_route(ctx, other, oracle, name, frame_name):
    """aligned: 256 x 128 in two 128 x 128 groups, every destination row 16-byte aligned (the vector path on every
    plane); ragged: 203 x 137 in cells of 64 with an 11-wide last column and a 9-high last row, the extra channel's stride
    203 (the 4-byte path), every sample outside the rects a canary of the pattern"""
    w, h, _ = ec.ALIGNED if frame_name == "aligned" else ec.RAGGED
    specs, want = _rgba_case(other, oracle, name, frame_name)
    got = _new_route(ctx, specs, w, h, 3, [1], 8, frame_name == "ragged")
    _assert_planes(got, want, f"{name} {frame_name}")
    assert len(np.unique(want[3])) > 20


@pytest.mark.parametrize("frame_name", ["aligned", "ragged"])
@pytest.mark.parametrize("name", ec.lists_for(4))
def test_rgba_equals_the_three_call_route(ctx, other, oracle, name, frame_name):
    w, h, _ = ec.ALIGNED if frame_name == "aligned" else ec.RAGGED
    specs, want = _rgba_case(other, oracle, name, frame_name)
    _assert_planes(_three_call_route(ctx, specs, w, h, [1], 8, frame_name == "ragged"), want, f"three calls, {name} {frame_name}")


def test_one_large_group_has_streamed_levels(ctx, other, oracle):
    """300 x 200 in one group: levels beyond the LDS tile run as streamed launches whose last one writes the planes"""
    specs = [ec.spec("squeeze", 3, 0, 0, 300, 200, 4)]
    want = _reference(other, oracle, specs, 300, 200, 3, [0], 8, False)
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    got = _new_route(ctx, specs, 300, 200, 3, [0], 8, False)
    seen = ctx.kernel_times()
    ctx.kernel_timing(False)
    _assert_planes(got, want, "300x200")
    assert seen["k_modular_local_squeeze_level"][1] >= 1 and seen["k_modular_local_squeeze_lds"][1] == 1


# ---------------------------------------------------------------- further layouts
@pytest.mark.parametrize("layout", ["grey_alpha", "grey_three"])
@pytest.mark.parametrize("name", ["none", "palette_all", "general_p5", "squeeze", "palette_squeeze"])
def test_grey_layouts(ctx, other, oracle, layout, name):
    n_colour, n_ec = ec.LAYOUTS[layout]
    ecs = [2, 0, 1][:n_ec]
    w, h, _ = ec.GREY
    specs = ec.frame_specs(name, ec.GREY, n_colour + n_ec)
    want = _reference(other, oracle, specs, w, h, 1, ecs, 8, True)
    got = _new_route(ctx, specs, w, h, 1, ecs, 8, True)
    _assert_planes(got, want, f"{layout} {name}")
    assert bit_equal(got[0], got[1]) and bit_equal(got[0], got[2]), "grey is fanned out"


@pytest.mark.parametrize("n_colour,name", [(n, name) for n in (3, 1) for name in
                                           ("none", "rct", "palette_all", "general_p5", "squeeze", "palette_squeeze")
                                           if name in ec.lists_for(n)])
def test_colour_only_is_the_frame_form(ctx, other, oracle, n_colour, name):
    """3 + 0 and 1 + 0: no extra channel named.  Grey alone takes the plain launch of the frame form, whose fan-out
    stores through planes 1 and 2; the result is also what jxlh_frame_set_modular_groups_squeeze gives"""
    from jxl_rs_amd import lib
    w, h, _ = ec.RAGGED
    specs = ec.frame_specs(name, ec.RAGGED, n_colour, seed=12)
    want = _reference(other, oracle, specs, w, h, n_colour, [], 8, True)
    got = _new_route(ctx, specs, w, h, n_colour, [], 8, True)
    _assert_planes(got, want, f"{n_colour} + 0 {name}")
    _begin_modular(ctx, w, h, 8, [], True, n_colour)
    arena, batch = lib.pack_local_squeeze_groups(specs)
    ctx.set_modular_groups_squeeze(arena, batch, 8, wp=[sp["wp"] for sp in specs], n=len(specs))
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, f"squeeze form, {n_colour} channels {name}")
    if n_colour == 1:
        assert bit_equal(got[0], got[1]) and bit_equal(got[0], got[2]), "grey is fanned out"


def test_xyb_format_with_alpha(ctx, other, oracle):
    from jxl_rs_amd import lib
    fmt = 16 | lib.MODULAR_XYB
    w, h, _ = ec.RAGGED
    specs = ec.frame_specs("rct", ec.RAGGED, 4, seed=5)
    want = _reference(other, oracle, specs, w, h, 3, [0], fmt, True, bits=16)
    got = _new_route(ctx, specs, w, h, 3, [0], fmt, True)
    _assert_planes(got, want, "xyb")


@pytest.mark.parametrize("layout", ["extra_1", "extra_2", "extra_4"])
def test_extra_only_on_a_modular_frame(ctx, other, oracle, layout):
    n_ec = ec.LAYOUTS[layout][1]
    ecs = [3, 1, 0, 2][:n_ec]
    w, h, _ = ec.RAGGED
    for name in ("palette_all", "squeeze") + (("rct",) if n_ec >= 3 else ()):
        specs = ec.frame_specs(name, ec.RAGGED, n_ec, seed=9)
        want = _reference(other, oracle, specs, w, h, 0, ecs, 8, True)
        got = _new_route(ctx, specs, w, h, 0, ecs, 8, True)
        _assert_planes(got, want, f"{layout} {name}")


@pytest.fixture(scope="module")
def vardct():
    from jxl_rs_amd import synth
    return synth.make_vardct(256, 256, mix=synth.MIX_DCT8, seed=77, epf_iters=1)


def _vardct_channels(oracle, rng_seed):
    """(ec, up, specs, full plane): channels 0, 1 (one call of two), 2..5 (one call of four) at 256 x 256, channel 6 at
    128 x 128 with ec_upsampling 2 in a call of its own"""
    calls = []
    for ecs, size, up, name in (([0], 256, 1, "palette_all"), ([1, 2], 256, 1, "squeeze"), ([3, 4, 5, 6], 256, 1, "rct"),
                                ([7], 128, 2, "general_p13")):
        specs = ec.frame_specs(name, (size, size, 128), len(ecs), seed=rng_seed)
        calls.append((ecs, size, up, specs))
    return calls


def test_vardct_frame_extra_channels(ctx, other, oracle, vardct):
    calls = _vardct_channels(oracle, 21)
    upload_frame(ctx, vardct)
    upload_frame(other, vardct)
    for ecs, size, up, specs in calls:
        for e in ecs:
            ctx.begin_extra_channel(e, size, size, 8, up)
        _call(ctx, specs, 0, ecs, 0, wait=(ecs[0] % 2 == 0), device_arena=(len(ecs) == 2))
        full = _full_planes(oracle, specs, size, size, 0, ecs, False)
        for e, plane in zip(ecs, full):
            other.set_extra_channel(e, plane, 8, up)
    for c in (ctx, other):
        c.frame_run()
        c.sync()
    all_ecs = [e for ecs, _, _, _ in calls for e in ecs]
    _assert_planes(_read(ctx, 256, 256, all_ecs), _read(other, 256, 256, all_ecs), "vardct")
    # a group replaced after the run, then only its groups rendered again
    ecs, size, up, specs = calls[2]
    repl = [ec.spec("palette_last", 99, 128, 0, 128, 128, 4)]
    _call(ctx, repl, 0, ecs, 0)
    from jxl_rs_amd import lib
    with pytest.raises(lib.JxlHipError) as e:
        ctx.read_extra_channel(ecs[0], 256, 256)
    assert e.value.status == lib.ERR_BAD_STATE, "not rendered between the call and the run"
    ctx.rerender_groups([0])
    ctx.sync()
    full = _full_planes(oracle, specs + repl, size, size, 0, ecs, False)
    upload_frame(other, vardct)
    for e2, plane in zip(ecs, full):
        other.set_extra_channel(e2, plane, 8, up)
    other.frame_run()
    other.sync()
    _assert_planes(_read(ctx, 256, 256, ecs), _read(other, 256, 256, ecs), "vardct, rerendered")


# ---------------------------------------------------------------- behaviour
@pytest.mark.parametrize("how", ["device", "async_sync", "async_mark", "device_async"])
def test_arenas_and_async(ctx, other, oracle, how):
    w, h, _ = ec.RAGGED
    specs, want = _rgba_case(other, oracle, "rct_palette", "ragged")
    got = _new_route(ctx, specs, w, h, 3, [1], 8, True, device_arena=how.startswith("device"), wait=(how == "device"),
                     mark=(how == "async_mark"))
    _assert_planes(got, want, how)


def test_replaced_after_a_run_repainted_and_saved(ctx, other, oracle):
    from jxl_rs_amd import lib
    w, h, _ = ec.ALIGNED
    specs, _ = _rgba_case(other, oracle, "palette_all", "aligned")
    _new_route(ctx, specs, w, h, 3, [1], 8, False)
    repl = [ec.spec("rct", 41, 128, 0, 128, 128, 4)]
    _call(ctx, repl, 3, [1], 8)
    with pytest.raises(lib.JxlHipError) as e:
        ctx.read_extra_channel(1, w, h)
    assert e.value.status == lib.ERR_BAD_STATE, "the channel is not rendered between the call and the repaint"
    ctx.repaint_groups([0])
    ctx.sync()
    got = _read(ctx, w, h, [1])
    desc = lib.save_desc([0, 1, 2, 4], lib.SAVE_U8)
    saved = ctx.frame_save(desc)
    want = _reference(other, oracle, specs + repl, w, h, 3, [1], 8, False)
    _assert_planes(got, want, "repainted")
    assert np.array_equal(saved, other.frame_save(desc)) and len(np.unique(saved)) > 50


def test_patches_over_the_alpha_are_rebuilt(ctx, other, oracle, vardct):
    """a patch dictionary that draws into the alpha: the patched copy of a run is stale after the call and rebuilt by the
    next rerender"""
    from jxl_rs_amd import lib
    rng = np.random.default_rng(8)
    ref = [rng.uniform(-0.5, 1.5, (64, 96)).astype(np.float32) for _ in range(4)]
    patches, blendings = [], []
    for _ in range(30):
        xs, ys = int(rng.integers(8, 48)), int(rng.integers(8, 40))
        patches.append((int(rng.integers(0, 256 - xs + 1)), int(rng.integers(0, 256 - ys + 1)), 0,
                        int(rng.integers(0, 96 - xs + 1)), int(rng.integers(0, 64 - ys + 1)), xs, ys))
        blendings += [(int(rng.integers(0, 8)), 0, bool(rng.integers(0, 2))) for _ in range(2)]
    first = ec.frame_specs("general_p0", (256, 256, 128), 1, seed=31)
    repl = [ec.spec("squeeze", 32, 0, 128, 128, 128, 1)]
    got = []
    for c in (ctx, other):
        c.set_reference(0, ref)
        upload_frame(c, vardct)
        if c is ctx:
            c.begin_extra_channel(0, 256, 256, 8, 1)
            _call(c, first, 0, [0], 0)
        else:
            c.set_extra_channel(0, _full_planes(oracle, first + repl, 256, 256, 0, [0], False)[0], 8)
        c.set_patches(patches, blendings, [lib.EC_ALPHA])
        c.frame_run()
        c.sync()
        if c is ctx:
            before = c.read_extra_channel(0, 256, 256)
            _call(c, repl, 0, [0], 0)
            c.rerender_groups([0])
            c.sync()
        got.append(c.read_planes() + [c.read_extra_channel(0, 256, 256)])
        c.clear_reference(0)
    _assert_planes(got[0], got[1], "patched alpha")
    assert not bit_equal(before, got[0][3])
    plain = np.float32(_full_planes(oracle, first + repl, 256, 256, 0, [0], False)[0]) * np.float32(1.0 / 255.0)
    assert not bit_equal(got[0][3], plain), "the patches did reach the channel"


# ---------------------------------------------------------------- accounting
def _times(ctx, fn):
    ctx.sync()
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    try:
        fn()
        ctx.sync()
        return {k: v[1] for k, v in ctx.kernel_times().items() if v[1]}
    finally:
        ctx.kernel_timing(False)


def test_launch_accounting(ctx):
    """the labels and counts of the squeeze-form call for the same groups (its stage-level form: the frame form takes no
    fourth channel), and no k_ec_scatter"""
    from jxl_rs_amd import lib
    w, h, _ = ec.RAGGED
    specs = []
    for i, (x0, y0, gw, gh) in enumerate(ec.grid(w, h, 64)):
        specs.append(ec.spec(ec.lists_for(4)[i % len(ec.lists_for(4))], 2, x0, y0, gw, gh, 4))
    arena, batch = lib.pack_local_squeeze_groups(specs)
    wp = [sp["wp"] for sp in specs]
    outs = [lib.DeviceArray(np.zeros((h, w), np.int32)) for _ in range(4)]
    try:
        stage = _times(ctx, lambda: ctx.modular_local_transforms_squeeze(arena, batch, 8, outs, w, h, w, wp=wp, n=len(specs)))
    finally:
        for o in outs:
            o.free()
    _begin_modular(ctx, w, h, 8, [0], False, 3)
    frame = _times(ctx, lambda: _call(ctx, specs, 3, [0], 8, wait=False))
    assert frame == stage, (frame, stage)
    assert "k_ec_scatter" not in frame and set(frame) == {"k_modular_local", "k_modular_local_squeeze_lds", "k_modular_local_phase",
                                                          "k_modular_local_palette"}
    assert frame["k_modular_local"] == 1 and frame["k_modular_local_squeeze_lds"] == 1


def test_refusals_enqueue_nothing_and_change_nothing(ctx, other, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    INV, BAD, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_BAD_STATE, lib.ERR_UNSUPPORTED
    w, h, _ = ec.ALIGNED
    specs, want = _rgba_case(other, oracle, "rct", "aligned")
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups(specs)

    def status(c, dest, fmt=8, n=len(specs), fn="jxlh_frame_set_modular_groups_extra", arena_ptr=arena.ctypes.data):
        bad = C.c_size_t(777)
        st = getattr(c.L, fn)(c._ctx, arena_ptr, arena.size, groups, n, coded, len(coded), params, len(params), None, fmt,
                              None if dest is None else C.byref(dest), C.byref(bad))
        return st, bad.value

    fresh = jxl_rs_amd.Context(0, 1)
    try:
        for fn in ("jxlh_frame_set_modular_groups_extra", "jxlh_frame_set_modular_groups_extra_async"):
            assert status(fresh, _dest(3, [1]), fn=fn) == (BAD, 777), "outside a frame"
    finally:
        fresh.close()
    got = _new_route(ctx, specs, w, h, 3, [1], 8, False)  # ... and ec 0 set at another size below
    _assert_planes(got, want, "before")

    def refusals():
        d = lib.local_dest
        assert status(ctx, None) == (INV, 777)
        assert status(ctx, d(3, [1]), arena_ptr=None) == (INV, 777)
        for dest in (d(2, [1]), d(4, []), d(3, [0, 1]), d(0, []), d(3, [lib.MAX_EXTRA_CHANNELS]), d(0, [1, 1]),
                     d(3, [1], bit_depth=8), d(0, [1], bit_depth=32)):
            fmt = 0 if dest.n_colour == 0 else 8
            assert status(ctx, dest, fmt) == (INV, 777), (dest.n_colour, dest.n_ec, list(dest.ec), dest.bit_depth)
        assert status(ctx, d(0, [1], bit_depth=8), 8) == (INV, 777), "sample_format without colour"
        assert status(ctx, d(3, [1]), 0) == (INV, 777) and status(ctx, d(3, [1]), 12) == (INV, 777), "the frame's format is 8"
        assert status(ctx, d(3, [2])) == (BAD, 777), "a channel that is not set"
        assert status(ctx, d(3, [0])) == (UNS, 777), "a channel of another size"
        assert status(ctx, d(0, [0, 1]), 0) == (UNS, 777)
        groups[1].n_channels = 3
        assert status(ctx, d(3, [1])) == (INV, 1), "a group whose n_channels differs"
        groups[1].n_channels = 4
        groups[1].x0 = 129
        assert status(ctx, d(3, [1])) == (INV, 1), "a rect that leaves the planes"
        assert b"group 1" in ctx.L.jxlh_last_error(ctx._ctx)
        groups[1].x0 = 128
        rct_type = groups[1].steps[0].rct_type
        groups[1].steps[0].rct_type = 42
        assert status(ctx, d(3, [1])) == (INV, 1), "what the lowering rejects"
        groups[1].steps[0].rct_type = rct_type
        # a transform behind the squeeze: what the squeeze-form lowering answers JXLH_ERR_UNSUPPORTED
        st = L2(ctx._ctx, arena2.ctypes.data, arena2.size, groups2, len(specs2), coded2, len(coded2), params2, len(params2), None, 8,
                C.byref(d(3, [1])), C.byref(bad2))
        assert (st, bad2.value) == (UNS, 1)

    specs2 = ec.frame_specs("palette_squeeze", ec.ALIGNED, 4)
    arena2, (groups2, coded2, params2) = lib.pack_local_squeeze_groups(specs2)
    groups2[1].squeeze_pos = 0
    bad2 = C.c_size_t(777)
    L2 = ctx.L.jxlh_frame_set_modular_groups_extra
    ctx.begin_extra_channel(0, 64, 64, 8, 2)
    assert _times(ctx, refusals) == {}, "a refusal enqueues nothing"
    # planes and channel state as they were: the channel is still rendered, nothing was stored
    _assert_planes(_read(ctx, w, h, [1]), want, "after the refusals")
    # a VarDCT frame takes no colour; a chroma-subsampled Modular frame neither
    upload_frame(ctx, synth.make_vardct(64, 64, mix=synth.MIX_DCT8, seed=1, epf_iters=0))
    ctx.begin_extra_channel(1, w, h, 8, 1)
    assert status(ctx, _dest(3, [1])) == (BAD, 777)
    p = _params(ctx, w, h)
    for c in (0, 2):
        p.hshift[c] = p.vshift[c] = 1
    ctx.modular_frame_begin(p)
    ctx.begin_extra_channel(1, w, h, 8, 1)
    assert status(ctx, _dest(3, [1])) == (UNS, 777)
    # the extra channels of such a frame are not subsampled: the call gets as far as the groups (which hold four channels)
    assert status(ctx, _dest(0, [1]), 0) == (INV, 0)


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    sp = ec.spec("none", 1, 0, 0, 8, 8, 1)
    arena, batch = lib.pack_local_squeeze_groups([sp])
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            upload_frame(c, wl)
            c.set_extra_channel(0, np.zeros((8, 8), np.int32), 8)
            for wait in (True, False):
                assert c.try_set_modular_groups_extra(arena, batch, 0, lib.local_dest(0, [0], bit_depth=8), wait=wait) == \
                    (lib.ERR_UNSUPPORTED, None)
    finally:
        for c in peers:
            c.close()
