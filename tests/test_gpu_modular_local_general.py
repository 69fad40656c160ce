"""Group-local palettes with delta entries and all 14 predictors on the device (run with -m gpu on an MI355X):
jxlh_modular_local_transforms_general (the stage-level form, exact i32 read-back) and
jxlh_frame_set_modular_groups_general* (the frame form, against the rect-by-rect route).  Expected samples are the
committed oracle's palette_delta / palette_delta_wp run on each group's own h x w arrays, composed in the reference's
order by tests/modular_local_general_ref.py; every comparison is exact equality.  Inputs follow the recipe of that
module, which tests/test_modular_local_general_cpu.py proves not to be vacuous."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import modular_local_general_ref as gr
import modular_local_ref as mr
from helpers import bit_equal, diff_report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = np.int32(0x5ca1ab1e)
POISON = 0x0badf00d
# the kernel's tile constants, pinned to its source below: rows a workgroup walks at a time, steps per chunk, entries of
# one palette row that fit LDS
LP_ROWS, LP_CHUNK, LP_LDS_ENTRIES = 64, 32, 2048
# predictor (and header) cases: every predictor, and for the weighted one the three headers
CASES = [(p, gr.WP_DEFAULT) for p in range(14)] + [(6, gr.WP_A), (6, gr.WP_B)]
CASE_IDS = [f"p{p}" for p in range(14)] + ["p6_hdrA", "p6_hdrB"]


def test_tile_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "jxl_rs_amd", "csrc", "jxlh_internal.h")).read()
    assert int(re.search(r"constexpr int kLpRows = (\d+);", src).group(1)) == LP_ROWS
    assert int(re.search(r"constexpr int kLpChunk = (\d+);", src).group(1)) == LP_CHUNK
    assert int(re.search(r"constexpr uint32_t kLpLdsEntries = (\d+);", src).group(1)) == LP_LDS_ENTRIES


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def _lib_steps(steps):
    from jxl_rs_amd import lib
    return [lib.local_rct(s["begin_c"], s["rct_type"]) if s["kind"] == mr.RCT else
            lib.local_palette(s["begin_c"], s["num_c"], s["table"], s["num_deltas"], s["predictor"]) for s in steps]


def _spec(x0, y0, n_channels, steps, coded, wp=gr.WP_DEFAULT):
    return {"x0": x0, "y0": y0, "n_channels": n_channels, "steps": _lib_steps(steps), "ref_steps": steps, "coded": coded,
            "wp": wp}


def _delta_spec(rng, x0, y0, shape, predictor, wp=gr.WP_DEFAULT, num_c=3, num_colors=11, num_deltas=5, bit_depth=8):
    n_channels = max(num_c, 3) if num_c > 1 else 1
    steps = [gr.delta_palette(rng, 0, num_c, predictor, num_colors, num_deltas, bit_depth)]
    return _spec(x0, y0, n_channels, steps, gr.coded_for(n_channels, steps, shape, rng), wp)


_EXPECTED = {}


def _finished(oracle, sp, bit_depth):
    """a group's finished channels; computed once per spec object"""
    key = id(sp)
    if key not in _EXPECTED:
        _EXPECTED[key] = (sp, gr.local_apply(oracle, sp["n_channels"], sp["ref_steps"], sp["coded"], bit_depth, sp["wp"]))
    return _EXPECTED[key][1]


def _expected(oracle, specs, n_out, h, stride, bit_depth, fan=False):
    """the out planes after the call: canaries everywhere but in the rects"""
    want = [np.full((h, stride), CANARY, dtype=np.int32) for _ in range(n_out)]
    for sp in specs:
        gh, gw = sp["coded"][0].shape
        fin = _finished(oracle, sp, bit_depth)
        if fan and len(fin) == 1:
            fin = fin * 3
        for c, f in enumerate(fin):
            want[c][sp["y0"]:sp["y0"] + gh, sp["x0"]:sp["x0"] + gw] = f
    return want


def _run_stage(ctx, specs, n_out, w, h, stride, bit_depth, device_arena=False, **pack):
    """jxlh_modular_local_transforms_general into canary-filled device planes; -> the planes, whole.  The arena's gaps
    and row padding hold POISON."""
    from jxl_rs_amd import lib
    arena, groups = lib.pack_local_groups(specs, fill=POISON, **pack)
    wp = lib.wp_headers([sp["wp"] for sp in specs])
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(n_out)]
    keep = None
    try:
        if device_arena:
            keep = lib.DeviceArray(arena)
            ctx.modular_local_transforms_general(keep, groups, bit_depth, outs, w, h, stride, wp=wp, n=len(specs),
                                                 arena_samples=arena.size)
        else:
            ctx.modular_local_transforms_general(arena, groups, bit_depth, outs, w, h, stride, wp=wp, n=len(specs))
        return [o.download(np.int32, h * stride).reshape(h, stride) for o in outs]
    finally:
        for o in outs + ([keep] if keep else []):
            o.free()


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for c, (g, e) in enumerate(zip(got, want)):
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{what}: plane {c}: {len(bad)} samples differ, first at {bad[:4].tolist()}"


# ---------------------------------------------------------------- stage-level form
# (h, w) of the groups: the issue's sizes, then widths on both sides of the chunk length (and of two chunks, where the
# window of the rows above is refilled) and heights on both sides of the rows a workgroup walks at a time
SIZES = [(1, 1), (1, 40), (50, 1), (9, 2), (37, 53), (257, 3), (300, 258),
         (LP_ROWS - 1, LP_CHUNK - 1), (LP_ROWS, LP_CHUNK), (LP_ROWS + 1, LP_CHUNK + 1), (2 * LP_ROWS + 1, 2 * LP_CHUNK + 3)]


def _place(sizes, x_odd=1):
    """rects in one row at odd origins, a gap of canaries between them; -> (rects, w, h)"""
    x, rects = x_odd, []
    for gh, gw in sizes:
        rects.append((x, 1 + 2 * (len(rects) % 3), gw, gh))
        x += gw + 3
    return rects, x, max(y + gh for (_, y, _, gh) in rects) + 2


@pytest.mark.parametrize("predictor,wp", CASES, ids=CASE_IDS)
def test_every_predictor_on_every_size(ctx, oracle, predictor, wp):
    """one call per predictor / header: a delta palette of three channels on every size, at odd origins, with
    coded_stride = w + 1 (no vector path, POISON in the padding) and canaries around every rect and between rows"""
    rng = np.random.default_rng([500, predictor, wp[0]])
    rects, w, h = _place(SIZES)
    specs = [_delta_spec(rng, x0, y0, (gh, gw), predictor, wp) for x0, y0, gw, gh in rects]
    stride = w + 5
    got = _run_stage(ctx, specs, 3, w, h, stride, 8, align=1, stride_pad=1)
    want = _expected(oracle, specs, 3, h, stride, 8)
    assert sum(int((p == CANARY).sum()) for p in want) > 3 * h * 5, "canaries exist"
    _assert_same(got, want, f"predictor {predictor}")


@pytest.mark.parametrize("predictor,wp", [(5, gr.WP_DEFAULT), (13, gr.WP_DEFAULT), (6, gr.WP_A)], ids=["p5", "p13", "p6"])
def test_one_1024_group(ctx, oracle, predictor, wp):
    """16 bands of one workgroup per channel; 12-bit samples"""
    rng = np.random.default_rng([1024, predictor])
    specs = [_delta_spec(rng, 4, 2, (1024, 1024), predictor, wp, num_colors=200, num_deltas=7, bit_depth=12)]
    got = _run_stage(ctx, specs, 3, 1030, 1028, 1032, 12)
    _assert_same(got, _expected(oracle, specs, 3, 1028, 1032, 12), f"1024 x 1024, predictor {predictor}")


def _mixed_specs(rng, n, cols=8, cell=48):
    """n groups of mixed kinds on a grid of cells: copy, RCT, look-up palette, delta palettes, weighted; sizes 1..cell - 3"""
    specs = []
    headers = (gr.WP_DEFAULT, gr.WP_A, gr.WP_B)
    for k in range(n):
        gw, gh = int(rng.integers(1, cell - 2)), int(rng.integers(1, cell - 2))
        x0, y0 = cell * (k % cols) + int(rng.integers(0, 3)), cell * (k // cols) + int(rng.integers(0, 3))
        kind = k % 5
        if kind == 0:
            steps = []
        elif kind == 1:
            steps = [mr.rct(0, (5 * k + 3) % 42)]
        elif kind == 2:
            steps = [mr.palette(0, 3, rng.integers(0, 256, size=(3, 19), dtype=np.int64).astype(np.int32))]
        elif kind == 3:
            steps = [gr.delta_palette(rng, 0, 3, (1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13)[(k // 5) % 12])]
        else:
            steps = [gr.delta_palette(rng, 0, 3, 6)]
        specs.append(_spec(x0, y0, 3, steps, gr.coded_for(3, steps, (gh, gw), rng, 0, 200), headers[k % 3]))
    return specs


@pytest.mark.parametrize("device_arena", [False, True], ids=["host_arena", "device_arena"])
def test_mixed_batch_host_and_device_arena(ctx, oracle, device_arena):
    specs = _mixed_specs(np.random.default_rng(77), 60)
    w, h = 8 * 48 + 2, 8 * 48 + 2
    got = _run_stage(ctx, specs, 3, w, h, w + 2, 8, device_arena=device_arena)
    _assert_same(got, _expected(oracle, specs, 3, h, w + 2, 8), "mixed batch")


def test_palette_rows_inside_and_beyond_lds(ctx, oracle):
    """palette rows of kLpLdsEntries - 1, kLpLdsEntries and kLpLdsEntries + 1 values (the last one is read from global
    memory), with and without the weighted predictor, indices all over the table"""
    rng = np.random.default_rng(2048)
    specs = []
    for k, size in enumerate((LP_LDS_ENTRIES - 1, LP_LDS_ENTRIES, LP_LDS_ENTRIES + 1)):
        for j, predictor in enumerate((4, 6)):
            nd = 9
            steps = [mr.palette(0, 3, gr.recipe_table(rng, 3, size - nd, nd, 10), nd, predictor)]
            idx = gr.recipe_index(rng, (70, 45), size - nd, nd)
            far = rng.random(idx.shape) < 0.3
            idx[far] = rng.integers(0, size, size=int(far.sum()))
            idx[0, :4] = (size - 1, size, size - 2, 0)
            specs.append(_spec(1 + 50 * k, 1 + 75 * j, 3, steps, [idx], gr.WP_A))
    got = _run_stage(ctx, specs, 3, 152, 152, 156, 10)
    _assert_same(got, _expected(oracle, specs, 3, 152, 156, 10), "palette sizes around the LDS limit")


def test_phase_composition(ctx, oracle):
    """every list of the ref module side by side in one call: RCT / delta palette / RCT with the index PRODUCED by an RCT
    (kept in scratch while the palette overwrites its slot), a palette whose index is another general palette's output,
    two general palettes, look-up next to general, predictor 0 with deltas, and the plain lists"""
    rng = np.random.default_rng(909)
    lists = dict(mr.LISTS)
    lists.update(gr.GENERAL_LISTS)
    specs = []
    for i, (name, (n_channels, steps)) in enumerate(lists.items()):
        specs.append(_spec(1 + 100 * (i % 6), 1 + 75 * (i // 6), n_channels, steps,
                           gr.coded_for(n_channels, steps, (70, 97), rng, -9, 40), gr.WP_B))
    w, h = 602, 75 * 4 + 2
    got = _run_stage(ctx, specs, 4, w, h, w + 3, 8)
    _assert_same(got, _expected(oracle, specs, 4, h, w + 3, 8), "phase composition")


def _launches(ctx, fn):
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    try:
        fn()
        ctx.sync()
        return {k: n for k, (_, n) in ctx.kernel_times().items() if k.startswith("k_modular_local")}
    finally:
        ctx.kernel_timing(False)


def test_launch_accounting(ctx, oracle):
    rng = np.random.default_rng(31)
    plain = [sp for sp in _mixed_specs(rng, 40) if all(s["kind"] == mr.RCT or s["predictor"] == 0 for s in sp["ref_steps"])]
    assert len(plain) >= 20
    n = _launches(ctx, lambda: _run_stage(ctx, plain, 3, 386, 386, 388, 8))
    assert n == {"k_modular_local": 1}, n
    one = [_delta_spec(rng, 0, 0, (20, 30), 5)]
    many = [_delta_spec(rng, 32 * (k % 20), 24 * (k // 20), (20, 30), 5) for k in range(200)]
    a = _launches(ctx, lambda: _run_stage(ctx, one, 3, 640, 240, 640, 8))
    b = _launches(ctx, lambda: _run_stage(ctx, many, 3, 640, 240, 640, 8))
    assert a == b == {"k_modular_local_palette": 1}, (a, b)
    # the deepest group decides: two general palettes with a copy between them, next to plain groups
    deep = _spec(0, 0, *gr.GENERAL_LISTS["general_of_general"], gr.coded_for(*gr.GENERAL_LISTS["general_of_general"], (20, 30), rng))
    c = _launches(ctx, lambda: _run_stage(ctx, [deep] + many[1:50] + plain[:3], 3, 640, 386, 640, 8))
    assert c == {"k_modular_local": 1, "k_modular_local_palette": 2, "k_modular_local_phase": 1}, c


def test_refusals_launch_nothing(ctx):
    from jxl_rs_amd import lib
    rng = np.random.default_rng(1)
    w, h, stride = 64, 40, 64
    INV, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED

    def batch(third, **over):
        specs = [_delta_spec(rng, 0, 0, (20, 20), 5), _spec(20, 0, 3, [], [np.ones((20, 20), np.int32)] * 3), third]
        arena, groups = lib.pack_local_groups(specs)
        for k, v in over.items():
            setattr(groups[2].steps[0], k, v)
        return arena, groups

    good = _delta_spec(rng, 40, 0, (20, 20), 6)
    hdr = lib.wp_headers([gr.WP_DEFAULT] * 3)
    wide = lib.wp_headers([gr.WP_DEFAULT, gr.WP_DEFAULT, (32,) + gr.WP_DEFAULT[1:]])
    wide2 = lib.wp_headers([gr.WP_DEFAULT, gr.WP_DEFAULT, gr.WP_DEFAULT[:10] + (16,)])
    cases = [(batch(good, predictor=14), hdr, INV), (batch(good), None, INV), (batch(good), wide, INV),
             (batch(good), wide2, INV), (batch(good, num_colors=2 ** 31 - 3), hdr, INV),
             (batch(good, num_colors=12), hdr, INV),  # one entry per row more than the arena holds behind the table
             (batch(good, kind=2), hdr, UNS)]
    cases[5][0][1][2].steps[0].palette_offset = cases[5][0][0].size - 3 * 16
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ptr for o in outs])
    try:
        for i, ((arena, groups), wp, want) in enumerate(cases):
            bad, res = C.c_size_t(99), []
            n = _launches(ctx, lambda: res.append(ctx.L.jxlh_modular_local_transforms_general(
                ctx._ctx, arena.ctypes.data, arena.size, groups, wp, 3, 8, ptrs, 3, w, h, stride, C.byref(bad))))
            assert res[0] == want and bad.value == 2, (i, res[0], bad.value)
            assert b"group 2" in ctx.L.jxlh_last_error(ctx._ctx)
            assert n == {}
        ctx.sync()
        for o in outs:
            assert np.all(o.download(np.int32, h * stride) == CANARY)
        arena, groups = batch(good)
        assert ctx.L.jxlh_modular_local_transforms_general(ctx._ctx, arena.ctypes.data, arena.size, groups, hdr, 3, 8, ptrs, 3,
                                                           w, h, stride, None) == lib.OK
        assert not np.all(outs[0].download(np.int32, h * stride) == CANARY)
        # the plain call still refuses the same batch
        bad = C.c_size_t(99)
        assert ctx.L.jxlh_modular_local_transforms(ctx._ctx, arena.ctypes.data, arena.size, groups, 3, 8, ptrs, 3, w, h, stride,
                                                   C.byref(bad)) == UNS and bad.value == 0
    finally:
        for o in outs:
            o.free()


# ---------------------------------------------------------------- frame form
def _frame_specs(w, h, rng, grid=128, n_channels=3, bits=8):
    specs = []
    headers = (gr.WP_DEFAULT, gr.WP_A, gr.WP_B)
    for gy in range(0, h, grid):
        for gx in range(0, w, grid):
            gw, gh = min(grid, w - gx), min(grid, h - gy)
            k = len(specs)
            if n_channels == 1:
                steps = [gr.delta_palette(rng, 0, 1, (5, 6, 0)[k % 3], 40, 6, bits)] if k % 4 else []
            elif k % 3 == 1:
                steps = [mr.rct(0, (7 * k + 1) % 42)]
            else:
                steps = [gr.delta_palette(rng, 0, 3, (5, 6, 13, 2)[k % 4], 100, 8, bits)]
            coded = gr.coded_for(n_channels, steps, (gh, gw), rng, 0, (1 << bits) // 4)
            specs.append(_spec(gx, gy, n_channels, steps, coded, headers[k % 3]))
    return specs


def _params(ctx, w, h, gab, epf):
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = gab, epf
    return p


def _route_b(ctx, oracle, p, specs, fmt, bits):
    """the rect route: the oracle's transforms per group on the host, one jxlh_frame_set_modular_channels each"""
    ctx.modular_frame_begin(p)
    for sp in specs:
        fin = _finished(oracle, sp, bits)
        fin = fin * 3 if len(fin) == 1 else fin
        ctx.set_modular_channels(*fin, fmt, x0=sp["x0"], y0=sp["y0"])
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes()


def _set_groups(ctx, specs, fmt, wait=True):
    from jxl_rs_amd import lib
    arena, groups = lib.pack_local_groups(specs)
    ctx.set_modular_groups_general(arena, groups, fmt, wp=[sp["wp"] for sp in specs], n=len(specs), wait=wait)


def _assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 2)], ids=["plain", "gab_epf"])
def test_frame_groups_equal_the_rect_route(ctx, oracle, gab, epf):
    from jxl_rs_amd import lib
    w, h = 600, 420
    specs = _frame_specs(w, h, np.random.default_rng(600))
    p = _params(ctx, w, h, gab, epf)
    want = _route_b(ctx, oracle, p, specs, 8, 8)
    desc = lib.save_desc([0, 1, 2], lib.SAVE_U8)
    want_saved = ctx.frame_save(desc)
    ctx.modular_frame_begin(p)
    _set_groups(ctx, specs, 8)
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "groups vs rects")
    assert np.array_equal(ctx.frame_save(desc), want_saved)
    assert len(np.unique(want[0])) > 50


@pytest.mark.parametrize("kind", ["grey", "xyb"])
def test_frame_grey_fans_out_and_xyb_format(ctx, oracle, kind):
    from jxl_rs_amd import lib
    w, h = 300, 200
    fmt = 16 | lib.MODULAR_XYB if kind == "xyb" else 8
    bits = 16 if kind == "xyb" else 8
    specs = _frame_specs(w, h, np.random.default_rng(5), n_channels=1 if kind == "grey" else 3, bits=bits)
    p = _params(ctx, w, h, 0, 0)
    want = _route_b(ctx, oracle, p, specs, fmt, bits)
    ctx.modular_frame_begin(p)
    _set_groups(ctx, specs, fmt)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    _assert_planes(got, want, kind)
    if kind == "grey":
        assert bit_equal(got[0], got[1]) and bit_equal(got[0], got[2])


def test_frame_mixed_with_the_other_setters_replaced_and_async(ctx, oracle):
    """a third of the rects by jxlh_frame_set_modular_channels, a third by jxlh_frame_set_modular_groups (plain lists),
    the rest by the general call; after a run one rect is replaced through the _async form and the frame runs again"""
    from jxl_rs_amd import lib
    w, h = 384, 256
    specs = _frame_specs(w, h, np.random.default_rng(11))
    p = _params(ctx, w, h, 1, 1)
    by_rect, general = specs[::3], specs[2::3]
    plain = [sp for sp in specs[1::3]]
    assert all(s["kind"] == mr.RCT for sp in plain for s in sp["ref_steps"])

    def fill():
        ctx.modular_frame_begin(p)
        for sp in by_rect:
            ctx.set_modular_channels(*_finished(oracle, sp, 8), 8, x0=sp["x0"], y0=sp["y0"])
        arena, groups = lib.pack_local_groups(plain)
        ctx.set_modular_groups(arena, groups, 8, n=len(plain))
        _set_groups(ctx, general, 8)
        ctx.frame_run()

    fill()
    ctx.sync()
    _assert_planes(ctx.read_planes(), _route_b(ctx, oracle, p, specs, 8, 8), "mixed")
    fill()
    rng = np.random.default_rng(12)
    repl = [_delta_spec(rng, specs[0]["x0"], specs[0]["y0"], specs[0]["coded"][0].shape, 6, gr.WP_B)]
    _set_groups(ctx, repl, 8, wait=False)
    ctx.sync()
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), _route_b(ctx, oracle, p, repl + specs[1:], 8, 8), "replaced")
    with pytest.raises(lib.JxlHipError) as e:  # one sample_format per frame
        _set_groups(ctx, repl, 12)
    assert e.value.status == lib.ERR_INVALID_ARGUMENT


def test_frame_states(ctx):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    rng = np.random.default_rng(3)
    arena, groups = lib.pack_local_groups([_delta_spec(rng, 0, 0, (8, 8), 5)])

    def status(c, fn="jxlh_frame_set_modular_groups_general"):
        return getattr(c.L, fn)(c._ctx, arena.ctypes.data, arena.size, groups, None, 1, 8, None)

    fresh = jxl_rs_amd.Context(0, 1)
    try:
        assert status(fresh) == lib.ERR_BAD_STATE and status(fresh, "jxlh_frame_set_modular_groups_general_async") == lib.ERR_BAD_STATE
    finally:
        fresh.close()
    ctx.frame_begin(ctx.default_params(64, 64))  # a VarDCT frame
    assert status(ctx) == lib.ERR_BAD_STATE
    p = ctx.default_params(64, 64)
    p.gab, p.epf_iters = 0, 0
    for c in (0, 2):
        p.hshift[c] = p.vshift[c] = 1
    ctx.modular_frame_begin(p)
    assert status(ctx) == lib.ERR_UNSUPPORTED
    ctx.modular_frame_begin(_params(ctx, 64, 64, 0, 0))
    groups[0].x0 = 60  # the rect leaves the coded size
    assert status(ctx) == lib.ERR_INVALID_ARGUMENT
    groups[0].x0 = 0
    assert status(ctx) == lib.OK
