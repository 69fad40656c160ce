"""jxlh_frame_repaint_groups and jxlh_repaint_changed_rects on the device (jxl_hip_repaint.h; run with -m gpu on an
MI355X): groups of upsampled VarDCT frames and of Modular frames repainted after a whole run.  Every comparison is bit
for bit, and the expected side is always the oracle (jxlo_vardct_frame or the Modular stages, then jxlo_upsample and the
noise functions: tests/repaint_ref.py); a fresh context's whole run of the same final inputs is compared as well, which
tells a wrong kernel (both differ from the oracle) from stale rows (only the repainted context does)."""
import numpy as np
import pytest

import patches_ref as pr
import repaint_ref as rr
import save_ref as sr
import splines_ref
from helpers import bit_equal, diff_report, gpu_params_from, run_oracle_frame

pytestmark = pytest.mark.gpu

W, H = 300, 600  # 2 x 3 groups
STAGES = {"none": dict(epf_iters=0, gab=False), "gab_epf2": dict(epf_iters=2, gab=True), "epf3": dict(epf_iters=3, gab=True),
          "per_stage_epf1": dict(epf_iters=1, gab=False, flags=1)}
LISTS = [[3], [2, 3], [0, 3], [0, 1, 2, 3, 4, 5]]  # one group; a whole group row; the two diagonal groups; all
LUM = (0.2627, 0.678, 0.0593)


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fresh():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


_WL = {}


def workloads(w, h, stage, **more):
    """(A, B): the same frame from two seeds; B's coefficients arrive later, group by group"""
    from jxl_rs_amd import synth
    key = (w, h, stage, tuple(sorted(more.items())))
    if key not in _WL:
        opts = {k: v for k, v in STAGES[stage].items() if k != "flags"}
        mix = synth.MIX_DCT8 if "hshift" in more else synth.MIX_D1
        _WL[key] = (synth.make_vardct(w, h, mix=mix, seed=61, **opts, **more), synth.make_vardct(w, h, mix=mix, seed=62, **opts, **more))
    return _WL[key]


def params(ctx, wl, stage, n, noise, size=None):
    over = dict(flags=STAGES[stage].get("flags", 0), upsampling=n)
    if size:
        over.update(xsize_upsampled=size[0], ysize_upsampled=size[1])
    if noise:
        over.update(rr.NOISE)
    p = gpu_params_from(ctx, wl, **over)
    for i in range(8):
        p.noise_lut[i] = rr.NOISE_LUT[i] if noise else 0.0
    return p


def submit(ctx, wl, groups, transport):
    from jxl_rs_amd import lib
    if transport == "dense":
        for g in groups:
            ctx.submit_group(g, wl.coeffs[g])
    else:  # the slot-bucketed entries, packed by the library's own packer
        parts = [lib.host_pack_slots(wl.coeffs[g], group_id=g) for g in groups]
        assert all(len(q[3]) == 0 for q in parts)
        ctx.submit_groups_slots(np.asarray(groups, dtype=np.uint32), np.concatenate([q[0] for q in parts]),
                                np.concatenate([q[1].reshape(-1) for q in parts]), np.concatenate([q[2] for q in parts]), None)
    ctx.slot_wait(0)


def begin(ctx, wl, p, transport="dense", groups=None, before=None):
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    if before:
        before(ctx)
    submit(ctx, wl, range(wl.coeffs.shape[0]) if groups is None else groups, transport)


def assert_planes(got, want, what):
    for c in range(3):
        assert got[c].shape == want[c].shape, (what, c, got[c].shape, want[c].shape)
        assert bit_equal(got[c], want[c]), f"{what}: plane {c}: {diff_report(got[c], want[c])}"


def planes_of(ctx):
    ctx.sync()
    return ctx.read_planes()


def arrivals(ctx, fresh, oracle, a, b, stage, n, noise, lists, transport="dense", size=None, before=None, coded_of=None,
             repaint_first=False):
    """whole run of A (or, repaint_first, no run at all), then for every list: its groups arrive from the other workload,
    repaint_groups, and the result equals the oracle's frame of the mixed inputs and a fresh context's whole run"""
    p = params(ctx, a, stage, n, noise, size)
    begin(ctx, a, p, transport, before=before)
    cur, from_b = a, set()
    if not repaint_first:
        ctx.frame_run()
    for groups in lists:
        src_b = [g for g in groups if g not in from_b]
        src_a = [g for g in groups if g in from_b]
        cur = rr.with_groups_from(rr.with_groups_from(cur, b, src_b), a, src_a)
        from_b = (from_b | set(src_b)) - set(src_a)
        submit(ctx, cur, groups, transport)
        ctx.repaint_groups(groups)
        coded = coded_of(cur) if coded_of else None
        want = rr.vardct_result(oracle, cur, n, noise, size, coded)
        got = planes_of(ctx)
        begin(fresh, cur, params(fresh, cur, stage, n, noise, size), transport, before=before)
        fresh.frame_run()
        assert_planes(planes_of(fresh), want, f"{stage} x{n} {groups}: a FRESH context against the oracle")
        assert_planes(got, want, f"{stage} x{n} {groups}: repainted against the oracle")


# ---------------------------------------------------------------- VarDCT, upsampled
@pytest.mark.parametrize("stage", list(STAGES))
def test_vardct_upsampling_2_every_list(ctx, fresh, oracle, stage):
    a, b = workloads(W, H, stage)
    arrivals(ctx, fresh, oracle, a, b, stage, 2, True, LISTS)


@pytest.mark.parametrize("n,lists", [(4, [[3], [0, 3]]), (8, [[2]])], ids=["x4", "x8"])
def test_vardct_upsampling_4_and_8(ctx, fresh, oracle, n, lists):
    a, b = workloads(W, H, "gab_epf2")
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", n, True, lists)


def test_vardct_entries_transport(ctx, fresh, oracle):
    a, b = workloads(W, H, "gab_epf2")
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[3], [0, 5]], transport="entries")


def test_vardct_without_noise_and_without_filters(ctx, fresh, oracle):
    """the band route whose bands are the group rows themselves: centre rows [254, 514) of an upsampled frame"""
    a, b = workloads(W, H, "none")
    arrivals(ctx, fresh, oracle, a, b, "none", 4, False, [[2], [0, 5]])


def test_two_repaints_on_overlapping_rows_add_the_noise_once(ctx, fresh, oracle):
    a, b = workloads(W, H, "gab_epf2")
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[2], [3], [2, 3], [0, 2]])


def test_repaint_before_any_whole_run_is_a_whole_run(ctx, fresh, oracle):
    a, b = workloads(W, H, "gab_epf2")
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[1]], repaint_first=True)


def test_one_block_last_column_and_a_cut_result(ctx, fresh, oracle):
    a, b = workloads(264, 520, "gab_epf2")
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[1], [2, 5]])
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 4, True, [[4]], size=(264 * 4 - 3, 520 * 4 - 1))


@pytest.mark.parametrize("size", [(8, 600), (600, 8)], ids=["8x600", "600x8"])
def test_images_narrower_than_the_window(ctx, fresh, oracle, size):
    a, b = workloads(size[0], size[1], "gab_epf2")
    ng = a.coeffs.shape[0]
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 8 if size[0] == 8 else 2, True, [[1], [0, ng - 1]])


def test_420_takes_the_whole_run(ctx, fresh, oracle):
    a, b = workloads(W, H, "gab_epf2", hshift=(1, 0, 1), vshift=(1, 0, 1))
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[3]])


def test_lf_only_groups_that_arrive_later(ctx, fresh, oracle):
    """mark all, run, submit two, repaint: the two are transformed, the others stay filled from the LF image"""
    from lf_fill_ref import expected_planes
    a, _ = workloads(W, H, "gab_epf2")
    ng = a.coeffs.shape[0]
    p = params(ctx, a, "gab_epf2", 2, True)
    begin(ctx, a, p, groups=[])
    ctx.set_groups_lf_only(list(range(ng)))
    ctx.frame_run()
    assert_planes(planes_of(ctx), rr.finish(oracle, expected_planes(oracle, a, list(range(ng))), 2, True), "all marked")
    arrived = [1, 4]
    submit(ctx, a, arrived, "dense")
    ctx.repaint_groups(arrived)
    marked = [g for g in range(ng) if g not in arrived]
    assert_planes(planes_of(ctx), rr.finish(oracle, expected_planes(oracle, a, marked), 2, True), "two arrived")


def test_patches_and_splines_across_the_band_edge(ctx, fresh, oracle):
    """a patch dictionary, then splines, that cross rows 252 / 260 -- the edges of group row 1's band under gab + epf 2"""
    a, b = workloads(W, H, "gab_epf2")
    rng = np.random.default_rng(19)
    refs = [[rng.uniform(-0.5, 1.5, (64, 96)).astype(np.float32) for _ in range(3)]]
    patches = [(20, 240, 0, 0, 0, 90, 40), (150, 500, 0, 3, 5, 60, 30), (100, 230, 0, 10, 10, 40, 50)]
    blendings = [(pr.ADD, 0, False), (pr.REPLACE, 0, False), (pr.MUL, 0, False)]
    segs = np.float32([[60.0 + 8 * i, 236.0 + 3 * i, 6.0, 0.7, 0.3, 0.4, -0.3, 0.2] for i in range(12)])
    ref = splines_ref.Ref(fused=True)

    def with_patches(c):
        c.set_reference(0, refs[0])
        c.set_patches(patches, blendings, [])

    def with_splines(c):
        c.set_splines(segs)

    def patched(wl):
        col, _ = run_oracle_frame(oracle, wl)
        return pr.apply_patches([np.ascontiguousarray(q) for q in col], patches, blendings, refs, [])

    def drawn(wl):
        col, _ = run_oracle_frame(oracle, wl)
        return ref.draw([np.ascontiguousarray(q) for q in col], segs)

    try:
        arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[3], [0]], before=with_patches, coded_of=patched)
    finally:
        ctx.set_patches([], [], [])
        fresh.set_patches([], [], [])
    arrivals(ctx, fresh, oracle, a, b, "gab_epf2", 2, True, [[2], [5]], before=with_splines, coded_of=drawn)
    ctx.set_splines(np.zeros((0, 8), np.float32))
    fresh.set_splines(np.zeros((0, 8), np.float32))


# ---------------------------------------------------------------- VarDCT, upsampling 1
@pytest.mark.parametrize("stage", ["gab_epf2", "none"])
def test_upsampling_1_equals_rerender_groups(ctx, fresh, oracle, stage):
    a, b = workloads(W, H, stage)
    mixed = rr.with_groups_from(a, b, [0, 3])
    out = []
    for c, call in ((ctx, "repaint_groups"), (fresh, "rerender_groups")):
        begin(c, a, params(c, a, stage, 1, True))
        c.frame_run()
        submit(c, mixed, [0, 3], "dense")
        getattr(c, call)([0, 3])
        out.append(planes_of(c))
    assert_planes(out[0], out[1], "repaint_groups against rerender_groups on a twin context")
    assert_planes(out[0], rr.vardct_result(oracle, mixed, 1, True), "against the oracle")


# ---------------------------------------------------------------- Modular frames
def modular_params(ctx, gab, epf, n, noise):
    p = ctx.default_params(W, H)
    p.gab, p.epf_iters, p.upsampling, p.epf_sigma_for_modular = gab, epf, n, rr.SIGMA_FOR_MODULAR
    if noise:
        p.noise, p.visible_frame_index = 1, 3
        for i in range(8):
            p.noise_lut[i] = rr.NOISE_LUT[i]
    return p


def modular_whole(c, p, chans):
    c.modular_frame_begin(p)
    c.set_modular_channels(*chans, 8)
    c.frame_run()


MODULAR = [(0, 0, 1, False), (1, 2, 1, True), (0, 0, 2, True), (1, 2, 2, True), (1, 2, 2, False)]


@pytest.mark.parametrize("gab,epf,n,noise", MODULAR, ids=[f"gab{g}-epf{e}-x{n}-noise{int(z)}" for g, e, n, z in MODULAR])
def test_modular_cells_replaced_by_rect(ctx, fresh, oracle, gab, epf, n, noise):
    """a cell's samples are replaced (jxlh_frame_set_modular_channels) and the cell repainted: one cell, then two cells
    in non-adjacent group rows"""
    chans = rr.modular_samples(5, W, H)
    other = rr.modular_samples(6, W, H)
    p = modular_params(ctx, gab, epf, n, noise)
    modular_whole(ctx, p, chans)
    assert_planes(planes_of(ctx), rr.modular_result(oracle, chans, gab, epf, n, noise), "whole run")
    cur = [c.copy() for c in chans]
    for groups in ([3], [0, 5]):
        for g in groups:
            x0, y0, x1, y1 = rr.cell(W, H, g)
            for c in range(3):
                cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1] + 64
            ctx.set_modular_channels(*[np.ascontiguousarray(c[y0:y1, x0:x1]) for c in cur], 8, x0=x0, y0=y0)
        ctx.repaint_groups(groups)
        want = rr.modular_result(oracle, cur, gab, epf, n, noise)
        got = planes_of(ctx)
        modular_whole(fresh, p, cur)
        assert_planes(planes_of(fresh), want, f"{groups}: a FRESH context against the oracle")
        assert_planes(got, want, f"{groups}: repainted against the oracle")


def test_modular_cells_replaced_by_groups(ctx, fresh, oracle):
    """the same with the batched intake (jxlh_frame_set_modular_groups): the cells as decoded groups without transforms"""
    from jxl_rs_amd import lib
    chans, other = rr.modular_samples(5, W, H), rr.modular_samples(6, W, H)
    p = modular_params(ctx, 1, 2, 2, True)
    modular_whole(ctx, p, chans)
    cur = [c.copy() for c in chans]
    groups, specs = [1, 4], []
    for g in groups:
        x0, y0, x1, y1 = rr.cell(W, H, g)
        for c in range(3):
            cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1] + 64
        specs.append(dict(x0=x0, y0=y0, n_channels=3, steps=[], coded=[c[y0:y1, x0:x1] for c in cur]))
    arena, packed = lib.pack_local_groups(specs)
    ctx.set_modular_groups(arena, packed, 8, n=len(specs))
    ctx.repaint_groups(groups)
    want = rr.modular_result(oracle, cur, 1, 2, 2, True)
    got = planes_of(ctx)
    modular_whole(fresh, p, cur)
    assert_planes(planes_of(fresh), want, "a FRESH context against the oracle")
    assert_planes(got, want, "repainted against the oracle")


# ---------------------------------------------------------------- save rects
@pytest.mark.parametrize("kind", ["vardct_x2", "modular_x2"])
def test_save_rects_of_the_changed_rects(ctx, fresh, oracle, kind):
    """after each of three arrivals only repaint_changed_rects' rects are saved into a host image kept across arrivals:
    it equals a fresh context's whole frame_save, and a poisoned copy shows that nothing outside the rects was written"""
    from jxl_rs_amd import lib
    from test_gpu_save import lib_desc as to_lib
    desc = sr.desc([0, 1, 2], sr.U16)

    def lib_desc(c):
        return to_lib(desc)

    if kind == "vardct_x2":
        a, b = workloads(W, H, "gab_epf2")
        p = params(ctx, a, "gab_epf2", 2, True)
        begin(ctx, a, p)
        cur = a
    else:
        chans, other = rr.modular_samples(5, W, H), rr.modular_samples(6, W, H)
        p = modular_params(ctx, 1, 2, 2, True)
        ctx.modular_frame_begin(p)
        ctx.set_modular_channels(*chans, 8)
        cur = [c.copy() for c in chans]
    ctx.frame_run()
    image = ctx.frame_save(lib_desc(ctx), None)
    for groups in ([3], [0, 5], [1, 2]):
        if kind == "vardct_x2":
            cur = rr.with_groups_from(cur, b, groups)
            submit(ctx, cur, groups, "dense")
        else:
            for g in groups:
                x0, y0, x1, y1 = rr.cell(W, H, g)
                for c in range(3):
                    cur[c][y0:y1, x0:x1] = other[c][y0:y1, x0:x1] + 64
                ctx.set_modular_channels(*[np.ascontiguousarray(c[y0:y1, x0:x1]) for c in cur], 8, x0=x0, y0=y0)
        ctx.repaint_groups(groups)
        rects = ctx.repaint_changed_rects(groups)
        before = image.copy()
        ctx.frame_save_rects(lib_desc(ctx), rects, None, out=image)
        assert not np.array_equal(image, before), groups
        poisoned = np.full_like(image, 0x5a)
        ctx.frame_save_rects(lib_desc(ctx), rects, None, out=poisoned)
        oh, ow = image.shape[0], image.shape[1] // 3  # rows of three interleaved samples per pixel
        out = rr.outside(rects, ow, oh)
        assert np.all(poisoned.reshape(oh, ow, 3)[out] == 0x5a), groups
        assert np.array_equal(poisoned.reshape(oh, ow, 3)[~out], image.reshape(oh, ow, 3)[~out]), groups
        if kind == "vardct_x2":
            begin(fresh, cur, params(fresh, cur, "gab_epf2", 2, True))
            fresh.frame_run()
        else:
            modular_whole(fresh, p, cur)
        assert np.array_equal(image, fresh.frame_save(lib_desc(fresh), None)), groups


# ---------------------------------------------------------------- statuses
def test_statuses_in_order_and_a_refused_call_changes_nothing(ctx, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    a, _ = workloads(W, H, "gab_epf2")
    L = ctx.L
    ids = np.zeros(1, dtype=np.uint32)
    assert L.jxlh_frame_repaint_groups(None, ids.ctypes.data, 1) == lib.ERR_INVALID_ARGUMENT
    never = jxl_rs_amd.Context(0, 1)
    try:
        assert never.try_repaint_groups(None) == lib.ERR_INVALID_ARGUMENT  # null ids come before the state
        assert never.try_repaint_groups([0]) == lib.ERR_BAD_STATE          # outside a frame
        never.frame_begin(params(never, a, "gab_epf2", 2, True))
        assert never.try_repaint_groups([0]) == lib.ERR_BAD_STATE          # VarDCT without its dequantisation tables
        assert never.try_repaint_groups([99]) == lib.ERR_BAD_STATE         # ... which comes before the ids
    finally:
        never.close()
    begin(ctx, a, params(ctx, a, "gab_epf2", 2, True))
    ctx.frame_run()
    before = planes_of(ctx)
    assert ctx.try_repaint_groups(None) == lib.ERR_INVALID_ARGUMENT
    assert ctx.try_repaint_groups([0, 6]) == lib.ERR_INVALID_ARGUMENT  # an id beyond the 2 x 3 grid
    assert ctx.try_repaint_groups([]) == lib.OK                        # nothing enqueued
    assert_planes(planes_of(ctx), before, "refused calls and the empty list leave the result alone")
    assert_planes(before, rr.vardct_result(oracle, a, 2, True), "the whole run")
    # the other calls keep their refusals
    with pytest.raises(jxl_rs_amd.JxlHipError) as e:
        ctx.rerender_groups([0])
    assert e.value.status == lib.ERR_UNSUPPORTED
    assert lib.try_changed_rects(ctx.params, [0])[0] == lib.ERR_UNSUPPORTED
    assert_planes(planes_of(ctx), before, "... and change nothing either")
    # Modular: an id beyond the grid; no tables needed
    ctx.modular_frame_begin(modular_params(ctx, 0, 0, 2, False))
    assert ctx.try_repaint_groups([6]) == lib.ERR_INVALID_ARGUMENT
    assert ctx.try_repaint_groups([5]) == lib.OK  # (never rendered: a whole run of zero samples)


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib
    a, _ = workloads(W, H, "gab_epf2")
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            begin(c, a, params(c, a, "gab_epf2", 1, False))
            assert c.try_repaint_groups([0]) == lib.ERR_UNSUPPORTED
            assert c.try_repaint_groups([99]) == lib.ERR_UNSUPPORTED  # ... before the ids are looked at
    finally:
        for c in peers:
            c.close()
