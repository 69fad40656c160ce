"""Group-local Modular transforms on the device (run with -m gpu on an MI355X): jxlh_modular_local_transforms (the
stage-level form, exact i32 read-back) and jxlh_frame_set_modular_groups* (the frame form, against the existing
rect-by-rect route).  Expected samples are the committed oracle's RCT and palette applied per group in the reference's
order (tests/modular_local_ref.py); everything is integer, every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import modular_local_ref as mr
from helpers import bit_equal, diff_report

pytestmark = pytest.mark.gpu

CANARY = np.int32(0x5ca1ab1e)
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


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


def _spec(x0, y0, n_channels, steps, coded):
    return {"x0": x0, "y0": y0, "n_channels": n_channels, "steps": _lib_steps(steps), "ref_steps": steps, "coded": coded}


def _expected(oracle, specs, n_out, w, h, stride, bit_depth, fan=False):
    """the out planes after the call: canaries everywhere but in the rects"""
    want = [np.full((h, stride), CANARY, dtype=np.int32) for _ in range(n_out)]
    for sp in specs:
        gh, gw = sp["coded"][0].shape
        fin = mr.local_apply(oracle, sp["n_channels"], sp["ref_steps"], sp["coded"], bit_depth)
        if fan and len(fin) == 1:
            fin = fin * 3
        for c, f in enumerate(fin):
            want[c][sp["y0"]:sp["y0"] + gh, sp["x0"]:sp["x0"] + gw] = f
    return want


def _run_stage(ctx, specs, n_out, w, h, stride, bit_depth, device_arena=False, **pack):
    """jxlh_modular_local_transforms into canary-filled device planes of h rows at `stride`; -> the planes, whole"""
    from jxl_rs_amd import lib
    arena, groups = lib.pack_local_groups(specs, fill=0x0badf00d, **pack)
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(n_out)]
    keep = None
    try:
        if device_arena:
            keep = lib.DeviceArray(arena)
            ctx.modular_local_transforms(keep, groups, bit_depth, outs, w, h, stride, n=len(specs), arena_samples=arena.size)
        else:
            ctx.modular_local_transforms(arena, groups, bit_depth, outs, w, h, stride, n=len(specs))
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
def test_every_rct_on_ragged_rects(ctx, oracle):
    """890 x 760 planes on a 128 grid: 42 rects, the right column 122 wide, the bottom row 120 high; rect k carries
    rct_type k.  Samples span the i32 range, with rows of INT32_MIN / INT32_MAX: the arithmetic wraps."""
    w, h, grid = 890, 760, 128
    rng = np.random.default_rng(4201)
    specs = []
    for gy in range(0, h, grid):
        for gx in range(0, w, grid):
            gw, gh = min(grid, w - gx), min(grid, h - gy)
            coded = [rng.integers(I32_MIN, I32_MAX, size=(gh, gw), dtype=np.int64, endpoint=True).astype(np.int32) for _ in range(3)]
            for c in range(3):
                coded[c][2 * c] = I32_MIN
                coded[c][2 * c + 1] = I32_MAX
                coded[c][7 + c] = (I32_MIN, I32_MAX, -1)[c]
            specs.append(_spec(gx, gy, 3, [mr.rct(0, len(specs))], coded))
    assert len(specs) == 42 and specs[6]["coded"][0].shape == (128, 122) and specs[41]["coded"][0].shape == (120, 122)
    stride = 892
    got = _run_stage(ctx, specs, 3, w, h, stride, 8)
    _assert_same(got, _expected(oracle, specs, 3, w, h, stride, 8), "42 RCTs")


def _index_plane(shape, size, rng):
    """indices that hit every branch of get_palette_value: in the table, the 4x4x4 cube [size, size + 64), the 5x5x5
    cube and beyond, negative ones including -1 and -143 (the delta table's period)"""
    idx = rng.integers(0, size, size=shape, dtype=np.int64)
    flat = idx.reshape(-1)
    n = flat.size
    flat[0:n // 8] = rng.integers(size, size + 64, size=n // 8)
    flat[n // 8:n // 4] = rng.integers(size + 64, size + 64 + 200, size=n // 4 - n // 8)
    flat[n // 4:3 * n // 8] = rng.integers(-300, 0, size=3 * n // 8 - n // 4)
    special = [-1, -143, -144, -2, size - 1, size, size + 63, size + 64, size + 64 + 124, size + 64 + 125, I32_MIN, I32_MAX - 1000000]
    flat[n - len(special):] = special
    return idx.astype(np.int32)


@pytest.mark.parametrize("bit_depth", [8, 12, 16])
def test_palettes(ctx, oracle, bit_depth):
    """num_colors 1, 2, 256 and 5000 (5000 entries or more do not fit the 4096 entries of LDS: read from global memory) x
    num_c 1, 3, 4, side by side in one call"""
    rng = np.random.default_rng([77, bit_depth])
    gw, gh = 37, 29
    specs = []
    for i, num_colors in enumerate((1, 2, 256, 5000)):
        for j, num_c in enumerate((1, 3, 4)):
            table = rng.integers(-(1 << bit_depth), 1 << bit_depth, size=(num_c, num_colors), dtype=np.int64).astype(np.int32)
            n_channels = max(3, num_c)
            begin = 1 if num_c == 1 else 0
            steps = [mr.palette(begin, num_c, table)]
            coded = [_index_plane((gh, gw), num_colors, rng) if k == begin else
                     rng.integers(0, 1 << bit_depth, size=(gh, gw), dtype=np.int64).astype(np.int32)
                     for k in range(n_channels - num_c + 1)]
            specs.append(_spec(3 + 40 * i, 1 + 32 * j, n_channels, steps, coded))
    w, h, stride = 170, 100, 172
    got = _run_stage(ctx, specs, 4, w, h, stride, bit_depth)
    _assert_same(got, _expected(oracle, specs, 4, w, h, stride, bit_depth), f"palettes at {bit_depth} bits")


def test_step_mixes_side_by_side(ctx, oracle):
    """the lists of tests/test_modular_local_cpu.py, one group each, different programs next to each other in one call
    (a group without steps among them)"""
    rng = np.random.default_rng(303)
    gw, gh = 45, 38
    specs = []
    for i, (name, (n_channels, steps)) in enumerate(mr.LISTS.items()):
        coded = mr.coded_for_test(n_channels, steps, (gh, gw), rng, -9, 40)  # indices also leave the 6 entries
        specs.append(_spec(48 * (i % 5), 40 * (i // 5), n_channels, steps, coded))
    assert any(not sp["ref_steps"] for sp in specs)
    w, h, stride = 240, 80, 240
    got = _run_stage(ctx, specs, 4, w, h, stride, 8)
    _assert_same(got, _expected(oracle, specs, 4, w, h, stride, 8), "step mixes")


def _geometry_specs(rects, rng):
    specs = []
    for k, (x0, y0, gw, gh) in enumerate(rects):
        if k % 3 == 2:
            table = rng.integers(0, 256, size=(3, 19), dtype=np.int64).astype(np.int32)
            steps = [mr.palette(0, 3, table)]
            coded = [rng.integers(-5, 19 + 64 + 130, size=(gh, gw), dtype=np.int64).astype(np.int32)]
        else:
            steps = [mr.rct(0, (5 * k + 3) % 42)]
            coded = [rng.integers(-300, 300, size=(gh, gw), dtype=np.int64).astype(np.int32) for _ in range(3)]
        specs.append(_spec(x0, y0, 3, steps, coded))
    return specs


SMALL_RECTS = [(0, 0, 1, 1), (4, 0, 3, 3), (8, 0, 127, 129), (136, 0, 128, 127), (268, 0, 129, 128), (400, 4, 1, 129),
               (404, 4, 129, 1), (404, 8, 3, 127), (412, 8, 128, 128), (0, 132, 128, 3)]
BIG_RECTS = [(0, 0, 1024, 1024), (1024, 0, 6, 1024), (0, 1024, 1024, 6), (1024, 1024, 6, 6)]  # 1030 x 1030 on a 1024 grid
# what makes a group leave the 16-byte path: an odd x0, odd arena offsets, coded_stride = w + 1, an odd plane stride
MODES = {"aligned": {}, "odd_x0": {"dx": 1}, "odd_offsets": {"pack": {"skew": 1}},
         "odd_stride": {"pack": {"align": 1, "stride_pad": 1}}, "odd_plane_stride": {"dstride": 1}}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("rects,w,h", [(SMALL_RECTS, 544, 140), (BIG_RECTS, 1032, 1030)], ids=["sides_1_to_129", "grid_1024"])
def test_geometry_vector_and_scalar_paths(ctx, oracle, rects, w, h, mode):
    """rect sides 1, 3, 127, 128, 129, 1024; the same data aligned (16-byte accesses) and with each thing that forces the
    4-byte path.  Canaries around every rect and between the rows (the planes' padding) stay."""
    m = MODES[mode]
    dx = m.get("dx", 0)
    rng = np.random.default_rng(len(rects))  # the same data in every mode
    specs = _geometry_specs([(x0 + dx, y0, gw, gh) for x0, y0, gw, gh in rects], rng)
    stride = w + 4 + m.get("dstride", 0)
    pw = w + dx
    got = _run_stage(ctx, specs, 3, pw, h, stride, 8, **m.get("pack", {}))
    want = _expected(oracle, specs, 3, pw, h, stride, 8)
    assert sum(int((p == CANARY).sum()) for p in want) > 3 * h * 4, "canaries exist"
    _assert_same(got, want, mode)


def test_host_and_device_arena_agree(ctx, oracle):
    rng = np.random.default_rng(9)
    specs = _geometry_specs(SMALL_RECTS, rng)
    a = _run_stage(ctx, specs, 3, 544, 140, 548, 8)
    b = _run_stage(ctx, specs, 3, 544, 140, 548, 8, device_arena=True)
    _assert_same(a, b, "host arena vs device arena")
    _assert_same(a, _expected(oracle, specs, 3, 544, 140, 548, 8), "host arena")


def test_refusals_launch_nothing(ctx):
    """a batch whose third group is refused leaves the planes as they were, names the group and its status"""
    from jxl_rs_amd import lib
    rng = np.random.default_rng(1)
    w, h, stride = 64, 40, 64
    table = rng.integers(0, 256, size=(3, 8), dtype=np.int64).astype(np.int32)

    def batch(third, **over):
        specs = [_spec(0, 0, 3, [mr.rct(0, 9)], [np.ones((20, 20), np.int32)] * 3),
                 _spec(20, 0, 3, [], [np.ones((20, 20), np.int32)] * 3), third]
        arena, groups = lib.pack_local_groups(specs)
        for k, v in over.items():
            setattr(groups[2], k, v)
        return arena, groups

    third = _spec(40, 0, 3, [mr.palette(0, 3, table)], [np.zeros((20, 20), np.int32)])
    delta = _spec(40, 0, 3, [mr.palette(0, 3, table, num_deltas=2)], [np.zeros((20, 20), np.int32)])
    four = _spec(40, 0, 4, [], [np.zeros((20, 20), np.int32)] * 4)
    cases = [(batch(delta), lib.ERR_UNSUPPORTED), (batch(third, x0=45), lib.ERR_INVALID_ARGUMENT),
             (batch(third, y0=21), lib.ERR_INVALID_ARGUMENT), (batch(four), lib.ERR_INVALID_ARGUMENT),
             (batch(third, n_coded=3), lib.ERR_INVALID_ARGUMENT)]
    outs = [lib.DeviceArray(np.full((h, stride), CANARY, dtype=np.int32)) for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[o.ptr for o in outs])
    try:
        for (arena, groups), want in cases:
            bad = C.c_size_t(99)
            st = ctx.L.jxlh_modular_local_transforms(ctx._ctx, arena.ctypes.data, arena.size, groups, 3, 8, ptrs, 3, w, h, stride, C.byref(bad))
            assert st == want and bad.value == 2
            assert b"group 2" in ctx.L.jxlh_last_error(ctx._ctx)
        host = np.zeros((h, stride), np.int32)  # out planes are device planes
        arena, groups = batch(third)
        hp = (C.c_void_p * 3)(host.ctypes.data, outs[1].ptr, outs[2].ptr)
        assert ctx.L.jxlh_modular_local_transforms(ctx._ctx, arena.ctypes.data, arena.size, groups, 3, 8, hp, 3, w, h, stride, None) == lib.ERR_INVALID_ARGUMENT
        ctx.sync()
        for o in outs:
            assert np.all(o.download(np.int32, h * stride) == CANARY)
        # ... and the same batch, accepted, writes
        assert ctx.L.jxlh_modular_local_transforms(ctx._ctx, arena.ctypes.data, arena.size, groups, 3, 8, ptrs, 3, w, h, stride, None) == lib.OK
        assert not np.all(outs[0].download(np.int32, h * stride) == CANARY)
    finally:
        for o in outs:
            o.free()


# ---------------------------------------------------------------- frame form
def _frame_specs(oracle, w, h, rng, grid=128, n_channels=3, bits=8):
    specs = []
    for gy in range(0, h, grid):
        for gx in range(0, w, grid):
            gw, gh = min(grid, w - gx), min(grid, h - gy)
            k = len(specs)
            if n_channels == 1:
                table = rng.integers(0, 1 << bits, size=(1, 40), dtype=np.int64).astype(np.int32)
                steps = [mr.palette(0, 1, table)] if k % 2 else []
                coded = [rng.integers(0, 40 if k % 2 else 1 << bits, size=(gh, gw), dtype=np.int64).astype(np.int32)]
            elif k % 3 == 1:
                table = rng.integers(0, 1 << bits, size=(3, 100), dtype=np.int64).astype(np.int32)
                steps = [mr.palette(0, 3, table)]
                coded = [rng.integers(0, 100, size=(gh, gw), dtype=np.int64).astype(np.int32)]
            else:
                steps = [mr.rct(0, (7 * k + 1) % 42)]
                coded = [rng.integers(0, (1 << bits) // 4, size=(gh, gw), dtype=np.int64).astype(np.int32) for _ in range(3)]
            specs.append(_spec(gx, gy, n_channels, steps, coded))
    return specs


def _params(ctx, w, h, gab, epf):
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = gab, epf
    return p


def _route_b(ctx, oracle, p, specs, fmt, bits):
    """the existing route: the oracle's transforms per group, one rect call each"""
    ctx.modular_frame_begin(p)
    for sp in specs:
        fin = mr.local_apply(oracle, sp["n_channels"], sp["ref_steps"], sp["coded"], bits)
        fin = fin * 3 if len(fin) == 1 else fin
        ctx.set_modular_channels(*fin, fmt, x0=sp["x0"], y0=sp["y0"])
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes()


def _assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


@pytest.mark.parametrize("gab,epf", [(0, 0), (1, 2)], ids=["plain", "gab_epf"])
def test_frame_groups_equal_the_rect_route(ctx, oracle, gab, epf):
    from jxl_rs_amd import lib
    w, h = 600, 420
    specs = _frame_specs(oracle, w, h, np.random.default_rng(600))
    p = _params(ctx, w, h, gab, epf)
    want = _route_b(ctx, oracle, p, specs, 8, 8)
    arena, groups = lib.pack_local_groups(specs)
    ctx.modular_frame_begin(p)
    ctx.set_modular_groups(arena, groups, 8, n=len(specs))
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "groups vs rects")
    assert len(np.unique(want[0])) > 50


@pytest.mark.parametrize("kind", ["grey", "xyb"])
def test_frame_grey_fans_out_and_xyb_format(ctx, oracle, kind):
    from jxl_rs_amd import lib
    w, h = 300, 200
    fmt = 16 | lib.MODULAR_XYB if kind == "xyb" else 8
    bits = 16 if kind == "xyb" else 8
    specs = _frame_specs(oracle, w, h, np.random.default_rng(5), n_channels=1 if kind == "grey" else 3, bits=bits)
    p = _params(ctx, w, h, 0, 0)
    want = _route_b(ctx, oracle, p, specs, fmt, bits)
    arena, groups = lib.pack_local_groups(specs)
    ctx.modular_frame_begin(p)
    ctx.set_modular_groups(arena, groups, fmt, n=len(specs))
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    _assert_planes(got, want, kind)
    if kind == "grey":
        assert bit_equal(got[0], got[1]) and bit_equal(got[0], got[2])


def test_frame_mixed_with_rects_replaced_and_async(ctx, oracle):
    """some rects by the old call, the others by the new one; after a run one rect is replaced through the _async form
    (followed by jxlh_ctx_sync) and the frame runs again"""
    from jxl_rs_amd import lib
    w, h = 384, 256
    rng = np.random.default_rng(11)
    specs = _frame_specs(oracle, w, h, rng)
    p = _params(ctx, w, h, 1, 1)
    old, new = specs[::2], specs[1::2]
    ctx.modular_frame_begin(p)
    for sp in old:
        ctx.set_modular_channels(*mr.local_apply(oracle, 3, sp["ref_steps"], sp["coded"], 8), 8, x0=sp["x0"], y0=sp["y0"])
    arena, groups = lib.pack_local_groups(new)
    ctx.set_modular_groups(arena, groups, 8, n=len(new))
    ctx.frame_run()
    ctx.sync()
    _assert_planes(ctx.read_planes(), _route_b(ctx, oracle, p, specs, 8, 8), "mixed")
    # the same frame again, then rect 0 replaced
    ctx.modular_frame_begin(p)
    for sp in old:
        ctx.set_modular_channels(*mr.local_apply(oracle, 3, sp["ref_steps"], sp["coded"], 8), 8, x0=sp["x0"], y0=sp["y0"])
    ctx.set_modular_groups(arena, groups, 8, n=len(new))
    ctx.frame_run()
    repl = _frame_specs(oracle, 128, 128, np.random.default_rng(12))[:1]
    repl[0]["ref_steps"], repl[0]["steps"] = [mr.rct(0, 33)], _lib_steps([mr.rct(0, 33)])
    arena2, groups2 = lib.pack_local_groups(repl)
    ctx.set_modular_groups(arena2, groups2, 8, n=1, wait=False)
    ctx.sync()
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    _assert_planes(got, _route_b(ctx, oracle, p, repl + specs[1:], 8, 8), "replaced")
    with pytest.raises(lib.JxlHipError) as e:  # one sample_format per frame
        ctx.set_modular_groups(arena2, groups2, 12, n=1)
    assert e.value.status == lib.ERR_INVALID_ARGUMENT


def test_frame_states(ctx):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    spec = _spec(0, 0, 3, [mr.rct(0, 1)], [np.zeros((8, 8), np.int32)] * 3)
    arena, groups = lib.pack_local_groups([spec])

    def status(c, fn="jxlh_frame_set_modular_groups"):
        return getattr(c.L, fn)(c._ctx, arena.ctypes.data, arena.size, groups, 1, 8, None)

    fresh = jxl_rs_amd.Context(0, 1)
    try:
        assert status(fresh) == lib.ERR_BAD_STATE and status(fresh, "jxlh_frame_set_modular_groups_async") == lib.ERR_BAD_STATE
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
    q = _params(ctx, 64, 64, 0, 0)
    ctx.modular_frame_begin(q)
    groups[0].x0 = 60  # the rect leaves the coded size
    assert status(ctx) == lib.ERR_INVALID_ARGUMENT
    groups[0].x0 = 0
    assert status(ctx) == lib.OK
