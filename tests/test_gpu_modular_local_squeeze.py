"""Group-local squeeze on the device (run with -m gpu on an MI355X): jxlh_modular_local_transforms_squeeze (the
stage-level form, exact i32 read-back) and jxlh_frame_set_modular_groups_squeeze* (the frame form, against the
rect-by-rect route).  Expected samples are the committed oracle's unsqueeze_h / unsqueeze_v, RCT and palettes run on each
group's own arrays, composed in the reference's order by tests/modular_local_squeeze_ref.py; every comparison is exact
equality.  The plane recipe is the one tests/test_modular_local_squeeze_cpu.py proves to reach every tendency regime."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import modular_local_general_ref as gr
import modular_local_ref as mr
import modular_local_squeeze_ref as sr
from helpers import bit_equal, diff_report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = np.int32(0x5ca1ab1e)
POISON = 0x0badf00d
LS_TILE, LS_LINES = 128, 64  # the kernels' constants, pinned to their source below


def test_tile_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "jxl_rs_amd", "csrc", "jxlh_internal.h")).read()
    assert int(re.search(r"constexpr int kLsTile = (\d+);", src).group(1)) == LS_TILE
    assert int(re.search(r"constexpr int kLsLines = (\d+);", src).group(1)) == LS_LINES


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


def _spec(rng, x0, y0, w, h, n_channels, steps, squeeze, data="plane", wp=gr.WP_DEFAULT, scale=500):
    """data: "plane" -- the channels that reach the squeeze are the recipe plane (palette lists: gr.coded_for's index
    recipe), forward-squeezed; "random" -- every coded channel holds random samples in [-scale, scale)"""
    if data == "random":
        coded = sr.random_coded(rng, n_channels, steps, squeeze, w, h, -scale, scale)
    else:
        if any(s["kind"] == mr.PALETTE for s in steps):
            planes = gr.coded_for(n_channels, steps, (h, w), rng, 0, 64)
        else:
            planes = [sr.recipe_plane(rng, h, w) + 9 * k for k in range(len(gr.coded_for(n_channels, steps, (1, 1), rng)))]
        coded = sr.forward(n_channels, steps, squeeze, planes) if squeeze is not None else planes
    return {"x0": x0, "y0": y0, "w": w, "h": h, "n_channels": n_channels, "steps": _lib_steps(steps), "ref_steps": steps,
            "squeeze": squeeze, "coded": coded, "wp": wp}


_EXPECTED = {}


def _finished(oracle, sp, bit_depth):
    """a group's finished channels; computed once per spec object"""
    key = id(sp)
    if key not in _EXPECTED:
        _EXPECTED[key] = (sp, sr.local_apply(oracle, sp["n_channels"], sp["ref_steps"], sp["squeeze"], sp["w"], sp["h"],
                                             sp["coded"], bit_depth, sp["wp"]))
    return _EXPECTED[key][1]


def _expected(oracle, specs, n_out, h, stride, bit_depth):
    """the out planes after the call: canaries everywhere but in the rects"""
    want = [np.full((h, stride), CANARY, dtype=np.int32) for _ in range(n_out)]
    for sp in specs:
        for c, f in enumerate(_finished(oracle, sp, bit_depth)):
            want[c][sp["y0"]:sp["y0"] + sp["h"], sp["x0"]:sp["x0"] + sp["w"]] = f
    return want


def _run_stage(ctx, specs, n_out, w, h, stride, bit_depth, device_arena=False, **pack):
    """jxlh_modular_local_transforms_squeeze into canary-filled device planes; -> the planes, whole.  The arena's gaps
    and row padding hold POISON."""
    from jxl_rs_amd import lib
    arena, batch = lib.pack_local_squeeze_groups(specs, fill=POISON, **pack)
    wp = lib.wp_headers([sp["wp"] for sp in specs])
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(n_out)]
    keep = None
    try:
        if device_arena:
            keep = lib.DeviceArray(arena)
            ctx.modular_local_transforms_squeeze(keep, batch, bit_depth, outs, w, h, stride, wp=wp, n=len(specs),
                                                 arena_samples=arena.size)
        else:
            ctx.modular_local_transforms_squeeze(arena, batch, bit_depth, outs, w, h, stride, wp=wp, n=len(specs))
        return [o.download(np.int32, h * stride).reshape(h, stride) for o in outs]
    finally:
        for o in outs + ([keep] if keep else []):
            o.free()


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for c, (g, e) in enumerate(zip(got, want)):
        bad = np.argwhere(g != e)
        assert len(bad) == 0, f"{what}: plane {c}: {len(bad)} samples differ, first at {bad[:4].tolist()}"


def _place(rects, x_odd=1):
    """the rects (w, h) in one row at odd origins, a gap of canaries between them; -> ((x0, y0, w, h) list, w, h)"""
    x, out = x_odd, []
    for gw, gh in rects:
        out.append((x, 1 + 2 * (len(out) % 3), gw, gh))
        x += gw + 3
    return out, x, max(y + gh for (_, y, _, gh) in out) + 2


# ---------------------------------------------------------------- stage-level form
# no level (1 x 1, 8 x 8 with one channel), odd tails, one-sample axes, one axis across the tile limit (17 x 130), both
# (129 x 127 is inside on one), two streamed levels (255 x 257, 256 x 256)
RECTS = [r for r in sr.RECTS if r != (1024, 1024)]


@pytest.mark.parametrize("data", ["plane", "random"])
@pytest.mark.parametrize("n_channels", [1, 2, 3, 4])
def test_default_squeeze_on_every_rect(ctx, oracle, n_channels, data):
    """one call per channel count (the preview branch fires for 3 and 4): a default squeeze on every rect, at odd origins,
    with strides of w + 1 at unaligned offsets (POISON in the padding) and canaries around every rect and between rows"""
    rng = np.random.default_rng([700, n_channels, data == "plane"])
    rects, w, h = _place(RECTS)
    specs = [_spec(rng, x0, y0, gw, gh, n_channels, [], [], data) for x0, y0, gw, gh in rects]
    stride = w + 5
    got = _run_stage(ctx, specs, n_channels, w, h, stride, 8, align=1, stride_pad=1)
    want = _expected(oracle, specs, n_channels, h, stride, 8)
    assert sum(int((p == CANARY).sum()) for p in want) > n_channels * h * 5, "canaries exist"
    _assert_same(got, want, f"{n_channels} channels, {data}")


def test_512x384_one_channel(ctx, oracle):
    """the streamed levels behind the LDS launch with several workgroups per level"""
    rng = np.random.default_rng(512)
    specs = [_spec(rng, 4, 2, 512, 384, 1, [], [])]
    got = _run_stage(ctx, specs, 1, 520, 388, 520, 8)
    _assert_same(got, _expected(oracle, specs, 1, 388, 520, 8), "512 x 384")


def test_one_1024_group_at_the_level_limit(ctx, oracle):
    """three channels of 1024 x 1024: 16 levels on channels 1 and 2 (the most a chain may hold), six of them streamed"""
    rng = np.random.default_rng(1024)
    specs = [_spec(rng, 3, 2, 1024, 1024, 3, [], [], "random", scale=300)]
    _, _, chains = sr.expected_program(3, [], [], 1024, 1024)
    assert [len(c["levels"]) for c in chains] == [14, 16, 16]
    got = _run_stage(ctx, specs, 3, 1030, 1028, 1032, 8)
    _assert_same(got, _expected(oracle, specs, 3, 1028, 1032, 8), "1024 x 1024")


@pytest.mark.parametrize("name", list(sr.EXPLICIT))
def test_explicit_lists(ctx, oracle, name):
    """not in place, one axis only (a 256-wide plane squeezed horizontally three times never enters the LDS launch), a
    sub-range of channels (channels 0 and 3 stay coded and are copied); 1 x 300 and 300 x 1 give zero-side residuals"""
    n_channels, squeeze = sr.EXPLICIT[name]
    rng = np.random.default_rng([len(name), n_channels])
    rects, w, h = _place([(9, 9), (1, 300), (300, 1), (17, 130), (256, 256), (2, 3)])
    specs = [_spec(rng, x0, y0, gw, gh, n_channels, [], squeeze, "plane" if i % 2 else "random")
             for i, (x0, y0, gw, gh) in enumerate(rects)]
    assert any(0 in c.shape for sp in specs for c in sp["coded"]), "zero-side residuals exist"
    got = _run_stage(ctx, specs, n_channels, w, h, w + 1, 8, align=1)
    _assert_same(got, _expected(oracle, specs, n_channels, h, w + 1, 8), name)


def test_large_magnitudes(ctx, oracle):
    """single levels on samples up to +-2^28, inside the LDS launch and streamed, both axes"""
    rng = np.random.default_rng(28)
    h1, v1 = [sr.params(1, 1, 0, 1)], [sr.params(0, 1, 0, 1)]
    rects, w, h = _place([(100, 37), (130, 37), (37, 100), (37, 130)])
    specs = [_spec(rng, x0, y0, gw, gh, 1, [], sq, "random", scale=2 ** 28)
             for (x0, y0, gw, gh), sq in zip(rects, (h1, h1, v1, v1))]
    for sp in specs:
        sp["coded"][0][2::5, 1:] = sp["coded"][0][2::5, :-1]  # equal neighbours: zero differences
    got = _run_stage(ctx, specs, 1, w, h, w, 31)
    want = _expected(oracle, specs, 1, h, w, 31)
    assert max(int(np.abs(p[p != CANARY].astype(np.int64)).max()) for p in want) > 2 ** 27
    _assert_same(got, want, "+-2^28")


FRONTS = {
    "rct": (3, [mr.rct(0, 17)]),
    "lookup": (3, [mr.palette(0, 3, np.arange(3 * 300, dtype=np.int32).reshape(3, 300) % 251)]),
    "predicted": (3, [gr.delta_palette(np.random.default_rng(4), 0, 3, 5)]),
    "weighted": (3, [gr.delta_palette(np.random.default_rng(5), 0, 3, 6)]),
    "rct_palette_1_1": (3, [mr.rct(0, 40), mr.palette(1, 1, mr.small_palette(1, 90))]),
    "delta_palette_rct": (4, [gr.delta_palette(np.random.default_rng(3), 3, 1, 5), mr.rct(1, 10)]),
}


def _mixed_specs(rng, n, cols=6, cell=150):
    """n groups of mixed kinds on a grid of cells: copy, RCT, look-up and predicted palettes without a squeeze; pure
    squeezes (default and explicit); squeezes behind an RCT and behind palettes; ragged sizes 1 .. cell - 3"""
    specs = []
    headers = (gr.WP_DEFAULT, gr.WP_A, gr.WP_B)
    fronts = list(FRONTS.values())
    for k in range(n):
        gw, gh = int(rng.integers(1, cell - 2)), int(rng.integers(1, cell - 2))
        x0, y0 = cell * (k % cols) + int(rng.integers(0, 3)), cell * (k // cols) + int(rng.integers(0, 3))
        kind = k % 8
        if kind == 0:
            nc, steps, sq = 3, [], None
        elif kind in (1, 2):
            (nc, steps), sq = fronts[(k // 8 + kind) % len(fronts)], None
        elif kind == 3:
            nc, steps, sq = 1 + (k // 8) % 4, [], []
        elif kind == 4:
            (nc, sq), steps = list(sr.EXPLICIT.values())[(k // 8) % len(sr.EXPLICIT)], []
        else:
            (nc, steps), sq = fronts[(k // 8 + kind) % len(fronts)], []
        specs.append(_spec(rng, x0, y0, gw, gh, nc, steps, sq, "plane" if k % 3 else "random", headers[k % 3], scale=60))
    return specs


@pytest.mark.parametrize("device_arena", [False, True], ids=["host_arena", "device_arena"])
def test_mixed_batch_host_and_device_arena(ctx, oracle, device_arena):
    specs = _mixed_specs(np.random.default_rng(78), 36)
    w, h = 6 * 150 + 2, 6 * 150 + 2
    got = _run_stage(ctx, specs, 4, w, h, w + 2, 8, device_arena=device_arena)
    _assert_same(got, _expected(oracle, specs, 4, h, w + 2, 8), "mixed batch")


@pytest.mark.parametrize("skew", [1, 3])
def test_unaligned_offsets_strides_and_origins(ctx, oracle, skew):
    """every block starts `skew` samples behind a multiple of 4, rows are 4k + 1 long, x0 is odd: the 4-byte path on
    every side, for the plain groups of the batch too"""
    specs = _mixed_specs(np.random.default_rng(79), 16)
    for sp in specs:
        sp["x0"] |= 1
    w, h = 6 * 150 + 3, 3 * 150 + 2
    got = _run_stage(ctx, specs, 4, w, h, w + 2, 8, align=4, skew=skew, stride_pad=1)
    _assert_same(got, _expected(oracle, specs, 4, h, w + 2, 8), f"skew {skew}")


@pytest.mark.parametrize("name", list(FRONTS))
def test_steps_in_front_of_a_squeeze(ctx, oracle, name):
    """a default squeeze of 130 x 131 (LDS launch and two streamed levels) behind every front list: the chains end in the
    rect, the phases run on it; a predicted palette's index is moved to scratch first"""
    n_channels, steps = FRONTS[name]
    rng = np.random.default_rng([41, len(name)])
    specs = [_spec(rng, 3, 1, 130, 131, n_channels, steps, [], wp=gr.WP_A), _spec(rng, 141, 2, 40, 9, n_channels, steps, [], wp=gr.WP_B)]
    got = _run_stage(ctx, specs, 4, 190, 135, 192, 8)
    _assert_same(got, _expected(oracle, specs, 4, 135, 192, 8), name)


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
    from jxl_rs_amd import lib
    rng = np.random.default_rng(32)
    one = [_spec(rng, 0, 0, 130, 130, 3, [], [], "random")]
    many = [_spec(rng, 132 * (k % 8), 132 * (k // 8), 130, 130, 3, [], [], "random") for k in range(40)]
    a = _launches(ctx, lambda: _run_stage(ctx, one, 3, 1056, 660, 1056, 8))
    b = _launches(ctx, lambda: _run_stage(ctx, many, 3, 1056, 660, 1056, 8))
    # 130 x 130: every level up to 65 x 65 runs in the LDS launch; the last two of each chain (130 x 65 or 65 x 130, then
    # 130 x 130) have a side above the tile and are streamed
    assert a == b == {"k_modular_local_squeeze_lds": 1, "k_modular_local_squeeze_level": 2}, (a, b)
    # the deepest group decides: an RCT behind the chains adds its phase; plain groups their one launch
    deep = _spec(rng, 0, 0, 130, 130, 3, [mr.rct(0, 5)], [], "random")
    plain = _spec(rng, 0, 140, 30, 30, 3, [mr.rct(0, 6)], None, "random")
    c = _launches(ctx, lambda: _run_stage(ctx, [deep, plain] + many[1:8], 3, 1056, 660, 1056, 8))
    assert c == {"k_modular_local": 1, "k_modular_local_squeeze_lds": 1, "k_modular_local_squeeze_level": 2,
                 "k_modular_local_phase": 1}, c
    # a batch without a squeeze group: exactly the launches of the _general call on the same groups
    nosq = [sp for sp in _mixed_specs(rng, 40) if sp["squeeze"] is None]
    assert len(nosq) >= 12
    d = _launches(ctx, lambda: _run_stage(ctx, nosq, 4, 902, 1052, 904, 8))
    general = [{"x0": sp["x0"], "y0": sp["y0"], "n_channels": sp["n_channels"], "steps": sp["steps"], "coded": sp["coded"]} for sp in nosq]
    arena, groups = lib.pack_local_groups(general)
    outs = [lib.DeviceArray(np.zeros((1052, 904), dtype=np.int32)) for _ in range(4)]
    try:
        e = _launches(ctx, lambda: ctx.modular_local_transforms_general(arena, groups, 8, outs, 902, 1052, 904,
                                                                        wp=[sp["wp"] for sp in nosq], n=len(nosq)))
    finally:
        for o in outs:
            o.free()
    assert d == e and "k_modular_local" in d and not any("squeeze" in k for k in d), (d, e)


def test_refusals_launch_nothing(ctx):
    from jxl_rs_amd import lib
    rng = np.random.default_rng(2)
    w, h, stride = 96, 40, 96
    INV, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED

    def batch(mutate=None, third_squeeze=()):
        specs = [_spec(rng, 0, 0, 30, 30, 3, [], [], "random"), _spec(rng, 32, 0, 30, 30, 3, [mr.rct(0, 1)], None, "random"),
                 _spec(rng, 64, 0, 30, 30, 3, [mr.rct(0, 2)], list(third_squeeze), "random")]
        arena, b = lib.pack_local_squeeze_groups(specs)
        if mutate:
            mutate(*b)
        return arena, b

    cases = [(batch(lambda g, c, p: setattr(g[2], "squeeze_pos", 0)), UNS),
             (batch(lambda g, c, p: setattr(g[2].steps[0], "kind", 2)), UNS),
             (batch(lambda g, c, p: setattr(g[2], "n_coded", g[2].n_coded - 1)), UNS),
             (batch(lambda g, c, p: setattr(p[0], "num_c", 4), third_squeeze=[(1, 1, 0, 3)]), INV),
             (batch(lambda g, c, p: setattr(p[1], "begin_c", 1), third_squeeze=[(1, 1, 0, 1), (0, 1, 0, 1)]), UNS),  # a residual
             (batch(lambda g, c, p: setattr(c[len(c) - 1], "stride", 1)), INV),
             (batch(lambda g, c, p: setattr(c[len(c) - 1], "offset", 2 ** 63)), INV),
             (batch(lambda g, c, p: setattr(c[len(c) - 1], "w", c[len(c) - 1].w + 1)), INV),
             (batch(lambda g, c, p: setattr(g[2], "x0", 70)), INV)]  # the rect leaves the planes
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ptr for o in outs])

    def call(arena, b, bad=None):
        groups, coded, params = b
        return ctx.L.jxlh_modular_local_transforms_squeeze(ctx._ctx, arena.ctypes.data, arena.size, groups, 3, coded, len(coded),
                                                           params, len(params), None, 8, ptrs, 3, w, h, stride, bad)

    try:
        for i, ((arena, b), want) in enumerate(cases):
            bad, res = C.c_size_t(99), []
            n = _launches(ctx, lambda: res.append(call(arena, b, C.byref(bad))))
            assert res[0] == want and bad.value == 2, (i, res[0], bad.value)
            assert b"group 2" in ctx.L.jxlh_last_error(ctx._ctx)
            assert n == {}
        ctx.sync()
        for o in outs:
            assert np.all(o.download(np.int32, h * stride) == CANARY)
        arena, b = batch()
        assert call(arena, b) == lib.OK
        assert not np.all(outs[0].download(np.int32, h * stride) == CANARY)
    finally:
        for o in outs:
            o.free()


# ---------------------------------------------------------------- frame form
def _frame_specs(w, h, rng, grid=200, n_channels=3):
    specs = []
    headers = (gr.WP_DEFAULT, gr.WP_A, gr.WP_B)
    for gy in range(0, h, grid):
        for gx in range(0, w, grid):
            gw, gh = min(grid, w - gx), min(grid, h - gy)
            k = len(specs)
            if n_channels == 1:
                steps, sq = [], ([] if k % 3 else None)
            elif k % 4 == 0:
                steps, sq = [], []
            elif k % 4 == 1:
                steps, sq = [mr.rct(0, (7 * k + 1) % 42)], []
            elif k % 4 == 2:
                steps, sq = [mr.rct(0, (5 * k + 2) % 42)], None
            else:
                steps, sq = [gr.delta_palette(rng, 0, 3, (5, 6)[k % 2], 100, 8, 8)], []
            specs.append(_spec(rng, gx, gy, gw, gh, n_channels, steps, sq, wp=headers[k % 3]))
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
    arena, batch = lib.pack_local_squeeze_groups(specs)
    ctx.set_modular_groups_squeeze(arena, batch, fmt, wp=[sp["wp"] for sp in specs], n=len(specs), wait=wait)


def _assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 2)], ids=["plain", "gab_epf"])
def test_frame_groups_equal_the_rect_route(ctx, oracle, gab, epf):
    from jxl_rs_amd import lib
    w, h = 600, 420
    specs = _frame_specs(w, h, np.random.default_rng(601))
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
    w, h = 300, 260
    fmt = 16 | lib.MODULAR_XYB if kind == "xyb" else 8
    bits = 16 if kind == "xyb" else 8
    specs = _frame_specs(w, h, np.random.default_rng(6), n_channels=1 if kind == "grey" else 3)
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


def test_frame_replaced_async_and_repainted(ctx, oracle):
    """after a run one squeeze group is replaced through the _async form and the frame runs again; then another one is
    replaced and only its group repainted (jxlh_frame_repaint_groups)"""
    from jxl_rs_amd import lib
    w, h = 512, 512
    rng = np.random.default_rng(13)
    specs = _frame_specs(w, h, rng, grid=256)
    p = _params(ctx, w, h, 1, 1)
    ctx.modular_frame_begin(p)
    _set_groups(ctx, specs, 8)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    _assert_planes(got, _route_b(ctx, oracle, p, specs, 8, 8), "first run")
    ctx.modular_frame_begin(p)
    _set_groups(ctx, specs, 8)
    ctx.frame_run()
    repl = [_spec(rng, 0, 0, 256, 256, 3, [mr.rct(0, 9)], [], wp=gr.WP_B)]
    _set_groups(ctx, repl, 8, wait=False)
    ctx.sync()
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    repl2 = [_spec(rng, 256, 0, 256, 256, 3, [], [], "random", scale=100)]
    _set_groups(ctx, repl2, 8)
    ctx.repaint_groups([1])
    ctx.sync()
    repainted = ctx.read_planes()
    _assert_planes(got, _route_b(ctx, oracle, p, repl + specs[1:], 8, 8), "replaced")
    _assert_planes(repainted, _route_b(ctx, oracle, p, repl + repl2 + specs[2:], 8, 8), "repainted")
    with pytest.raises(lib.JxlHipError) as e:  # one sample_format per frame
        _set_groups(ctx, repl, 12)
    assert e.value.status == lib.ERR_INVALID_ARGUMENT


def test_frame_states(ctx):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    rng = np.random.default_rng(3)
    arena, (groups, coded, params) = lib.pack_local_squeeze_groups([_spec(rng, 0, 0, 20, 20, 3, [], [], "random")])

    def status(c, fn="jxlh_frame_set_modular_groups_squeeze"):
        return getattr(c.L, fn)(c._ctx, arena.ctypes.data, arena.size, groups, 1, coded, len(coded), params, len(params), None, 8, None)

    fresh = jxl_rs_amd.Context(0, 1)
    try:
        assert status(fresh) == lib.ERR_BAD_STATE and status(fresh, "jxlh_frame_set_modular_groups_squeeze_async") == lib.ERR_BAD_STATE
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
