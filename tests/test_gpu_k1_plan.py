"""One case per branch of K1's launch plan (csrc/k1_plan.h, issued by csrc/k1_launch.hip), on the smallest frames that
reach the branch.  Every case is bit-exact against helpers.run_oracle_frame, and the work-list counters of the launch
(k1_counters) agree with the varblock counts of the transform map over the groups the launch covered.

Frames: 264 x 264 (2 x 2 groups, the second row and column one block wide: the class lists continue across groups, and
a band or a group list is a strict subset of the frame); 520 x 264 where the mix holds 64..256-pixel transforms (they
need a whole group); 4:2:0 on MIX_8X8.  The density cases run on 512 x 256 (two whole groups): the density hint is the
entries per coefficient of whole groups (coeff_epoch.h), so a group of one block column would dilute it below both
thresholds whatever its varblocks hold.

Which kernels a branch launches is held by the host test (tests/test_k1_plan_cpu.py); here the launches of every branch
run, on the device, to the oracle's bits."""
import numpy as np
import pytest

from helpers import bit_equal, diff_report, gpu_params_from, run_oracle_frame

pytestmark = pytest.mark.gpu

SUB420 = dict(hshift=(1, 0, 1), vshift=(1, 0, 1))
FORMS = ["dense", "pairs", "entries", "direct"]
NAME = {0: "dct8", 4: "dct16x16", 5: "dct32x32", 6: "dct16x8", 7: "dct8x16", 8: "dct32x8", 9: "dct8x32", 10: "dct32x16",
        11: "dct16x32"}
SPECIAL = (1, 2, 3, 12, 13, 14, 15, 16, 17)
LARGE = tuple(range(18, 27))


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    return Oracle(fused=True)


_cache = {}


def _frame(oracle, key, w, h, **kw):
    """(workload, the oracle's planes): made once per key, shared by the cases and left unchanged"""
    from jxl_rs_amd import synth
    if key not in _cache:
        wl = synth.make_vardct(w, h, **kw)
        _cache[key] = (wl, run_oracle_frame(oracle, wl)[0])
    return _cache[key]


def _d1(oracle):
    """without filters: a band run's transforms then cover the band's own group rows only (with filters they take a
    halo group row on each side, run_plan.h, which on two group rows is the whole frame)"""
    from jxl_rs_amd import synth
    return _frame(oracle, "d1", 264, 264, mix=synth.MIX_D1, seed=71, epf_iters=0, gab=False)


def _sub(oracle):
    from jxl_rs_amd import synth
    return _frame(oracle, "420", 264, 264, mix=synth.MIX_8X8, seed=72, epf_iters=1, **SUB420)


def _all(oracle):
    from jxl_rs_amd import synth
    return _frame(oracle, "all", 520, 264, mix=synth.MIX_ALL, seed=73, epf_iters=1)


def _map_counts(wl, groups=None):
    """varblocks per counter name from the transform map (bit 7 = a varblock's first block), over `groups` or the frame"""
    xg = (wl.xblocks + 31) // 32
    ng = xg * ((wl.yblocks + 31) // 32)
    first = []
    for g in (range(ng) if groups is None else groups):
        tm = wl.transform_map[(g // xg) * 32:(g // xg + 1) * 32, (g % xg) * 32:(g % xg + 1) * 32]
        first.append(tm[tm >= 128] & 127)
    first = np.concatenate(first + [np.zeros(0, np.uint8)])
    out = {name: int((first == t).sum()) for t, name in NAME.items()}
    out["special"] = int(np.isin(first, SPECIAL).sum())
    out["large"] = int(np.isin(first, LARGE).sum())
    return out


def _submit(ctx, wl, form, groups, dense_groups=()):
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    slotted = [g for g in groups if g not in dense_groups]
    if form == "dense":
        slotted, dense_groups = [], groups
    elif form == "pairs":
        for g in slotted:
            ctx.submit_group_sparse(g, *synth.to_sparse(wl.coeffs[g]))
    elif slotted:
        parts = {g: jl.host_pack_slots(wl.coeffs[g], group_id=g) for g in slotted}
        assert all(len(parts[g][3]) == 0 for g in slotted)
        ctx.submit_groups_slots(np.asarray(slotted, dtype=np.uint32), np.concatenate([parts[g][0] for g in slotted]),
                                np.concatenate([parts[g][1].reshape(-1) for g in slotted]),
                                np.concatenate([parts[g][2] for g in slotted]), None)
    for g in dense_groups:
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)


def _begin(ctx, wl, form, flags=0, dense_groups=()):
    from jxl_rs_amd import lib as jl
    p = gpu_params_from(ctx, wl)
    p.flags = flags | (jl.FRAME_DENSE_DEQUANT if form == "entries" else 0)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    _submit(ctx, wl, form, list(range(wl.coeffs.shape[0])), dense_groups)


def _hold(ctx, wl, want, what, run, groups=None, routed=()):
    """run() on the uploaded frame: the planes are the oracle's, the launch's counters the map's over `groups`"""
    ctx.kernel_timing_reset()
    ctx.kernel_timing(True)
    try:
        run()
        ctx.sync()
        got = ctx.read_planes()
        k1 = ctx.k1_counters()
    finally:
        ctx.kernel_timing(False)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"{what}, plane {c}: {diff_report(got[c], want[c])}"
    xg = (wl.xblocks + 31) // 32
    covered = list(range(xg * ((wl.yblocks + 31) // 32))) if groups is None else list(groups)
    have = _map_counts(wl, [g for g in covered if g not in routed])
    there = _map_counts(wl, [g for g in covered if g in routed])
    for name in have:
        # (the special and large varblocks of a routed group stay on the frame's lists: they read dense slabs anyway)
        n = have[name] + (there[name] if name in ("special", "large") else 0)
        assert k1["varblocks"][name] == n, (what, name, k1["varblocks"], have)
    for name in NAME.values():
        assert k1["dense_route_varblocks"][name] == there[name], (what, name, k1["dense_route_varblocks"], there)
    return k1


# ------------------------------------------------------------------ the four forms: whole run, band, group list
@pytest.mark.parametrize("form", FORMS)
def test_forms_444(ctx, oracle, form):
    wl, want = _d1(oracle)
    assert wl.coeffs.shape[0] == 4
    have = _map_counts(wl)
    assert all(have[name] > 0 for name in NAME.values()) and have["special"] == 0 and have["large"] == 0, have
    _begin(ctx, wl, form)
    _hold(ctx, wl, want, f"{form}, whole run", ctx.frame_run)
    # the band and the group list render the resident content again (nothing resubmitted: the frame stays in its form):
    # the planes stay the oracle's, the launch's counters are the band's / the list's
    _hold(ctx, wl, want, f"{form}, band", lambda: ctx.frame_run(1, 2), groups=[2, 3])
    _hold(ctx, wl, want, f"{form}, group list", lambda: ctx.rerender_groups([1, 2]), groups=[1, 2])


@pytest.mark.parametrize("form", FORMS)
def test_forms_420(ctx, oracle, form):
    wl, want = _sub(oracle)
    have = _map_counts(wl)
    assert have["dct8"] > 0 and have["special"] > 0 and sum(have.values()) == have["dct8"] + have["special"], have
    _begin(ctx, wl, form)
    _hold(ctx, wl, want, f"4:2:0 {form}", ctx.frame_run)


# ------------------------------------------------------------------ the direct form's dense-pass choices
@pytest.mark.parametrize("density,hint", [(0.05, 0), (0.2, 1), (0.4, 2)])
def test_direct_form_densities(ctx, oracle, density, hint):
    """one density on each side of the 0.125 and 0.25 entries-per-coefficient thresholds: the fallback launch behind
    both direct kernels, behind the dense pass of the 16..32-point classes, and no fallback launch at all"""
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    key = f"density{density}"
    if key not in _cache:
        wl = synth.make_vardct(512, 256, mix=synth.MIX_D1, seed=74, epf_iters=1)
        rng = np.random.default_rng(int(density * 100))
        m = rng.random(wl.coeffs.shape) < density
        wl.coeffs = np.where(m, rng.integers(-30, 31, size=wl.coeffs.shape), 0).astype(np.int32)
        _cache[key] = (wl, run_oracle_frame(oracle, wl)[0])
    wl, want = _cache[key]
    ng = wl.coeffs.shape[0]
    # what coeff_epoch.h computes: entries of the groups read in place over their 3 x 65536 coefficients
    share = sum(int(jl.host_pack_slots(wl.coeffs[g], group_id=g)[2].sum()) for g in range(ng)) / (ng * 3 * 65536)
    assert (2 if share > 0.25 else 1 if share > 0.125 else 0) == hint, share
    assert min(abs(share - 0.125), abs(share - 0.25)) > 0.02, share
    _begin(ctx, wl, "direct")
    _hold(ctx, wl, want, f"direct form at {share:.3f} entries per coefficient", ctx.frame_run)


def test_direct_form_routed_group(ctx, oracle):
    """one group arrives as a dense slab: its DCT classes run from the dense-route lists"""
    wl, want = _d1(oracle)
    _begin(ctx, wl, "direct", dense_groups=(0,))
    k1 = _hold(ctx, wl, want, "direct form, group 0 routed", ctx.frame_run, routed=(0,))
    assert all(k1["dense_route_varblocks"][name] > 0 for name in NAME.values()), k1["dense_route_varblocks"]


# ------------------------------------------------------------------ special and large varblocks
@pytest.mark.parametrize("form", ["dense", "direct"])
def test_special_and_large(ctx, oracle, form):
    """every transform type; in the direct form the groups that hold special / large varblocks are expanded to dense
    slabs inside the launch"""
    wl, want = _all(oracle)
    have = _map_counts(wl)
    assert have["special"] > 0 and have["large"] > 0, have
    _begin(ctx, wl, form)
    _hold(ctx, wl, want, f"all types, {form}", ctx.frame_run)


# ------------------------------------------------------------------ the strip flag on an all-closed map
def test_strip_all_closed_is_scan_only(ctx, oracle):
    """every varblock lies inside a 32x32 quadrant of its tile: the strip kernel takes every tile, K1 is its scan alone
    and leaves every work list empty"""
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    wl, want = _frame(oracle, "closed", 264, 264, mix=synth.MIX_D1, seed=75, epf_iters=2, aligned=True)
    _begin(ctx, wl, "dense", flags=jl.FRAME_STRIP)
    ctx.kernel_timing_reset()
    ctx.kernel_timing(True)
    try:
        ctx.frame_run()
        ctx.sync()
        got = ctx.read_planes()
        k1 = ctx.k1_counters()
    finally:
        ctx.kernel_timing(False)
    ran, tiles, by_class = ctx.frame_path()
    assert ran and by_class == 0 and tiles == 25, (ran, tiles, by_class)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"strip, plane {c}: {diff_report(got[c], want[c])}"
    assert not any(k1["varblocks"].values()) and not any(k1["dense_route_varblocks"].values()), k1
