"""K1 (dequantisation, chroma-from-luma, LLF, IDCT) held to the CPU oracle at the edges of its input domain, where the
synthetic content (jxl_rs_amd/synth.py) never goes: coefficient magnitudes up to the whole i32 range, wrapping `+=`
(frame/group.rs:566-572), the ends of the header fields and maps, quant biases on both sides of every condition of the
entries form's direct path (csrc/abi_frame.hip, FrameDev::se_direct_ok), and coefficient densities up to 1.

Every case computes the oracle frame first and compares each submission form with it bit for bit:
  dense       the dense slab (jxlh_submit_group)
  pairs       (position, value) pairs read in place, values outside i16 in `wide`
  expand      the same pairs with JXLH_FRAME_EXPAND_SPARSE (expanded to dense slabs on the device)
  slots       the slot-bucketed entries of the C packer (jxlh_host_pack_slots: split values, `wide`), read in place
  slots_dd    the same entries with JXLH_FRAME_DENSE_DEQUANT
"""
import copy

import numpy as np
import pytest

from helpers import bit_equal, diff_report, gpu_params_from, oracle_params_from

pytestmark = pytest.mark.gpu

FORMS = ("dense", "pairs", "expand", "slots", "slots_dd")
I32_MIN, I32_MAX = -2**31, 2**31 - 1
# each an edge of K1: the adjust_quant_bias table (|q| < 128), the entries' 10 / 12 bits, the packer's split limit
# (96 x 511 = 49 056, 96 x 2047 = 196 512), i16 pairs, f32's exact integers (2^24), the i32 ends
LADDER = [0, 1, -1, 2, -2, 3, -3, 127, -127, 128, -128, 129, -129, 511, -511, 512, -512, 2047, -2047, 2048, -2048,
          32767, -32767, 32768, -32768, 49056, -49056, 49057, -49057, 196512, -196512, 196513, -196513,
          2**24 - 1, -(2**24 - 1), 2**24, -2**24, 2**24 + 1, -(2**24 + 1), I32_MAX, I32_MIN + 1, I32_MIN]

# what ran, over the whole module (test_k1_kernel_coverage reads it last)
SEEN = {"varblocks": {}, "fallback_batches": 0, "dense_route_varblocks": 0, "kernels": set(), "forms": {}}


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


def _with(wl, coeffs=None, **attrs):
    w2 = copy.copy(wl)
    if coeffs is not None:
        w2.coeffs = np.ascontiguousarray(coeffs, dtype=np.int32)
    for k, v in attrs.items():
        setattr(w2, k, v)
    return w2


def _set_params(p, hdr):
    for k, v in hdr.items():
        if k == "quant_biases":
            for i in range(4):
                p.quant_biases[i] = v[i]
        else:
            setattr(p, k, v)
    return p


def oracle_frame(oracle, wl, hdr=None, tables=None):
    """the oracle's planes of wl with the header fields in hdr; asserts they are finite (non-finite output is out of
    scope: the case's scales are picked so that it is not)"""
    p = _set_params(oracle_params_from(oracle, wl), hdr or {})
    lf = oracle.dequant_lf(p, *wl.lf_q)
    planes, _ = oracle.vardct_frame(p, wl.coeffs, wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob, lf,
                                    wl.tables if tables is None else tables, num_threads=8)
    want = [pl[:wl.ysize, :wl.xsize].copy() for pl in planes]
    for c in range(3):
        assert np.isfinite(want[c]).all(), f"the oracle's plane {c} is not finite"
    return want


def _begin(ctx, wl, hdr, flags, tables):
    p = _set_params(gpu_params_from(ctx, wl), hdr or {})
    p.flags = flags
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables if tables is None else tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)


def pack_slots(coeffs):
    """jxlh_host_pack_slots of every group (split values, `wide`), or None when the slot form cannot carry the content:
    a channel's run holds at most 65536 entries (jxlh_submit_groups_slots), and the packer fails past the room it is
    given for split values"""
    from jxl_rs_amd import lib as jl
    out = []
    for g in range(coeffs.shape[0]):
        try:
            q = jl.host_pack_slots(coeffs[g], group_id=g, wide_capacity=max(4096, int(np.count_nonzero(coeffs[g]))))
        except jl.JxlHipError:
            return None
        if int(q[2].max()) > 65536:
            return None
        out.append(q)
    return out


def submit(ctx, form, coeffs, slots=None, slot_flags=None, groups=None):
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    ng = coeffs.shape[0]
    if form == "dense":
        for g in range(ng):
            ctx.submit_group(g, coeffs[g])
    elif form in ("pairs", "expand"):
        for g in range(ng):
            ctx.submit_group_sparse(g, *synth.to_sparse(coeffs[g]))
    else:
        ids = list(range(ng)) if groups is None else list(groups)
        parts = slots if slots is not None else pack_slots(coeffs)
        parts = [parts[g] for g in ids]
        wide = [q[3] for q in parts if len(q[3])]
        ctx.submit_groups_slots(np.asarray(ids, dtype=np.uint32), np.concatenate([q[0] for q in parts]),
                                np.concatenate([q[1].reshape(-1) for q in parts]), np.concatenate([q[2] for q in parts]),
                                np.concatenate(wide) if wide else None,
                                flags=jl.GROUP_COMPLETE if slot_flags is None else slot_flags)
    ctx.slot_wait(0)


def _flags(form):
    from jxl_rs_amd import lib as jl
    return {"expand": jl.FRAME_EXPAND_SPARSE, "slots_dd": jl.FRAME_DENSE_DEQUANT}.get(form, 0)


def _record(form, k1, kt):
    for k, v in k1["varblocks"].items():
        SEEN["varblocks"][k] = SEEN["varblocks"].get(k, 0) + v
    SEEN["fallback_batches"] += sum(k1["fallback_batches"].values())
    SEEN["dense_route_varblocks"] += sum(k1["dense_route_varblocks"].values())
    SEEN["kernels"] |= set(kt)
    f = SEEN["forms"].setdefault(form, {"varblocks": 0, "fallback_batches": 0})
    f["varblocks"] += sum(k1["varblocks"].values())
    f["fallback_batches"] += sum(k1["fallback_batches"].values())


def run_forms(ctx, wl, want, what, hdr=None, tables=None, forms=FORMS):
    """every submission form of wl.coeffs that can carry it against `want` (the oracle's planes); returns
    {form: k1_counters()}"""
    slots = pack_slots(wl.coeffs) if any(f.startswith("slots") for f in forms) else None
    if slots is None:
        forms = [f for f in forms if not f.startswith("slots")]
    out = {}
    for form in forms:
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        _begin(ctx, wl, hdr, _flags(form), tables)
        submit(ctx, form, wl.coeffs, slots)
        ctx.frame_run()
        ctx.sync()
        got = ctx.read_planes()
        k1 = ctx.k1_counters()
        kt = ctx.kernel_times()
        ctx.kernel_timing(False)
        for c in range(3):
            assert bit_equal(got[c], want[c]), f"{what}, form {form}, plane {c}: {diff_report(got[c], want[c])}"
        _record(form, k1, kt)
        out[form] = k1
    return out


def sprinkle(coeffs, values, rng, per_value):
    """put every value at `per_value` random HF positions of each channel (positions the synthetic content holds a
    non-zero coefficient at: inside a varblock, outside its LLF corner)"""
    out = coeffs.copy()
    flat = out.reshape(out.shape[0], 3, -1)
    for g in range(flat.shape[0]):
        for c in range(3):
            nz = np.flatnonzero(flat[g, c])
            if len(nz) == 0:
                continue
            k = min(len(nz), per_value * len(values))
            pos = rng.choice(nz, size=k, replace=False)
            flat[g, c, pos] = np.resize(np.asarray(values, np.int64), k).astype(np.int64).astype(np.int32)
    return out


# ------------------------------------------------------------------ magnitude ladder
LADDER_HDR = dict(global_scale=65536)   # inv_global_scale = 1: |q| up to 2^31 stays far inside f32 after the IDCT


@pytest.mark.parametrize("ttype", list(range(27)) + ["MIX_ALL"])
def test_magnitude_ladder(ctx, oracle, ttype):
    from jxl_rs_amd import synth
    mix = synth.MIX_ALL if ttype == "MIX_ALL" else {ttype: 1.0}
    size = (512, 512) if ttype == "MIX_ALL" else (256, 256)
    wl = synth.make_vardct(*size, mix=mix, seed=100 + (ttype if isinstance(ttype, int) else 27), epf_iters=1)
    rng = np.random.default_rng(7 if ttype == "MIX_ALL" else ttype)
    wl = _with(wl, sprinkle(wl.coeffs, LADDER, rng, 3), raw_quant=np.where(wl.raw_quant > 0, 256, 0).astype(np.int32))
    flat = wl.coeffs.reshape(-1)
    assert all((flat == v).any() for v in LADDER[1:]), "every ladder value is in the frame"
    want = oracle_frame(oracle, wl, LADDER_HDR)
    run_forms(ctx, wl, want, f"ladder, type {ttype}", LADDER_HDR)


# ------------------------------------------------------------------ wrapping +=
def test_wrapping_accumulation(ctx, oracle):
    """updates whose i32 sum overflows: the expected frame is the oracle's on the np.int32-wrapped sum
    (jxlo_coeffs.c:20; the reference's `current_coeffs[idx] += coeff` in a release build wraps).  The big values sit
    in two of the eight groups, which the slot form then routes to their dense slabs."""
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    wl = synth.make_vardct(1024, 512, mix=synth.MIX_D1, seed=61, epf_iters=1)
    rng = np.random.default_rng(61)
    ng = wl.coeffs.shape[0]
    hot = [1, 6]
    base = wl.coeffs.copy()
    big = np.zeros_like(base)
    big[hot] = sprinkle(np.where(base[hot] != 0, 1, 0).astype(np.int32), [I32_MAX, I32_MIN, I32_MAX - 5, I32_MIN + 9],
                        rng, 6)
    big = np.where(np.abs(big.astype(np.int64)) > 1000, big, 0).astype(np.int32)
    add = np.where(big > 0, 30000, np.where(big < 0, -30000, 0)).astype(np.int32)   # pushes every big value over
    wrapped = big.astype(np.int64) + add.astype(np.int64)
    wrapped = ((wrapped + 2**31) % 2**32 - 2**31).astype(np.int32)
    assert (big != 0).sum() > 100 and (np.sign(wrapped) == -np.sign(big))[big != 0].all(), "every sum wrapped"
    total = np.where(big != 0, wrapped, base).astype(np.int32)
    w_tot = _with(wl, total)
    want = oracle_frame(oracle, w_tot, LADDER_HDR)
    # the oracle's own sparse expansion agrees with the wrapped sum
    for g in hot:
        p1, n1, wd1 = synth.to_sparse(np.where(big[g] != 0, add[g], base[g]))
        exp = oracle.expand_sparse(p1, n1, np.concatenate([wd1, synth.to_sparse(big[g])[2]]))
        assert np.array_equal(exp.reshape(3, -1), total[g].reshape(3, -1)), g

    def run(what, body, flags=0):
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        _begin(ctx, w_tot, LADDER_HDR, flags, None)
        body()
        ctx.frame_run()
        ctx.sync()
        got = ctx.read_planes()
        k1, kt = ctx.k1_counters(), ctx.kernel_times()
        ctx.kernel_timing(False)
        for c in range(3):
            assert bit_equal(got[c], want[c]), f"{what}, plane {c}: {diff_report(got[c], want[c])}"
        _record(what, k1, kt)
        return k1, kt

    # (1) one pairs list per group with duplicate positions: the i16 update and the big value in `wide`
    def dup_pairs():
        for g in range(ng):
            p1, n1, wd1 = synth.to_sparse(np.where(big[g] != 0, add[g], base[g]))
            ctx.submit_group_sparse(g, p1, n1, np.concatenate([wd1, synth.to_sparse(big[g])[2]]))
        ctx.slot_wait(0)
    for flags in (0, jl.FRAME_EXPAND_SPARSE):
        run(f"duplicate pairs, flags {flags}", dup_pairs, flags)

    # (2) the big values resident in place (one run), then a JXLH_GROUP_ACCUMULATE pass of the updates on their groups
    def accumulate():
        submit(ctx, "slots", np.where(big != 0, big, base).astype(np.int32))
        ctx.frame_run()
        ctx.sync()
        submit(ctx, "slots", add, slot_flags=jl.GROUP_COMPLETE | jl.GROUP_ACCUMULATE, groups=hot)
    for flags in (0, jl.FRAME_DENSE_DEQUANT):
        k1, kt = run(f"accumulated pass, flags {flags}", accumulate, flags)
        if flags == 0:
            assert "k_entries_to_pairs" in kt, sorted(kt)   # the resident groups' earlier pass, widened to pairs

    # (3) `wide` alone: the big value and its update as two wide entries at one position
    def wide_dups():
        parts = pack_slots(np.where(big != 0, 0, base).astype(np.int32))
        for g in hot:
            sel = np.flatnonzero(big[g].reshape(-1))
            w = np.stack([np.concatenate([sel, sel]) + g * 3 * 65536,
                          np.concatenate([big[g].reshape(-1)[sel], add[g].reshape(-1)[sel]]).view(np.uint32)],
                         axis=1).astype(np.uint32)
            parts[g] = (parts[g][0], parts[g][1], parts[g][2], w)
        submit(ctx, "slots", base, slots=parts)
    k1, _ = run("wide duplicates", wide_dups)
    assert sum(k1["dense_route_varblocks"].values()) > 0, "the two groups with wide values are routed"


# ------------------------------------------------------------------ header and map ends
def _d1(seed, size=(512, 512), **kw):
    from jxl_rs_amd import synth
    return synth.make_vardct(*size, mix=synth.MIX_D1, seed=seed, epf_iters=kw.pop("epf_iters", 2), **kw)


def test_raw_quant_ends_with_epf(ctx, oracle):
    wl = _d1(71, epf_iters=3)
    rng = np.random.default_rng(71)
    rq = np.where(rng.random(wl.raw_quant.shape) < 0.5, 1, 256).astype(np.int32)
    # one value per varblock: the varblock's first block decides (k1_scan), the sigma map reads every block
    wl = _with(wl, raw_quant=np.where(wl.raw_quant > 0, rq, 0).astype(np.int32))
    assert (wl.raw_quant == 1).any() and (wl.raw_quant == 256).any()
    want = oracle_frame(oracle, wl)
    run_forms(ctx, wl, want, "raw_quant 1 and 256")


def test_colour_tile_ends(ctx, oracle):
    wl = _d1(72)
    rng = np.random.default_rng(72)
    pick = lambda s: rng.choice(np.array([-128, 127], np.int8), size=s).astype(np.int8)
    wl = _with(wl, ytox=pick(wl.ytox.shape), ytob=pick(wl.ytob.shape))
    want = oracle_frame(oracle, wl)
    run_forms(ctx, wl, want, "ytox / ytob at -128 and 127")


@pytest.mark.parametrize("hdr", [dict(global_scale=1, quant_lf=65536), dict(global_scale=73728, quant_lf=65536),
                                 dict(global_scale=73728, quant_lf=1),
                                 dict(color_factor=1, base_correlation_x=65504.0, base_correlation_b=-65504.0),
                                 dict(color_factor=65793, base_correlation_x=-65504.0, base_correlation_b=65504.0)],
                         ids=["gs1_qlf65536", "gs73728_qlf65536", "gs73728_qlf1", "cf1_base_max", "cf65793_base_min"])
def test_header_ends(ctx, oracle, hdr):
    wl = _d1(73, size=(512, 256))
    want = oracle_frame(oracle, wl, hdr)
    run_forms(ctx, wl, want, f"header {hdr}", hdr)


DEFAULT_BIASES = (1.0 - 0.05465007330715401, 1.0 - 0.07005449891748593, 1.0 - 0.049935103337343655, 0.145)
F = np.float32
# (bias_c for all three channels or bias3, direct path expected)
BIAS_STRADDLES = [
    ("c", F(1e-6), True), ("c", np.nextafter(F(1e-6), F(0)), False),
    ("c", F(1e6), True), ("c", np.nextafter(F(1e6), F(np.inf)), False),
    ("c", F(0.0), False), ("c", F(-0.5), False),
    ("3", F(0.0), True), ("3", F(-0.75), True), ("3", F(4.0), False), ("3", np.nextafter(F(4.0), F(5)), True),
]


def _entries_frame(seed):
    """d1 content, with one group dense enough that the direct path leaves batches to the dense pass: the fallback
    counters then tell whether the direct path ran"""
    wl = _d1(seed, size=(768, 512), epf_iters=1)
    rng = np.random.default_rng(seed)
    c = wl.coeffs.copy()
    for g in (1,):
        m = rng.random(c[g].shape) < 0.5
        c[g] = np.where(m, rng.integers(-9, 10, size=c[g].shape), c[g]).astype(np.int32)
    return _with(wl, c)


@pytest.mark.parametrize("which,value,direct", BIAS_STRADDLES,
                         ids=[f"bias{w}={float(v):.9g}" for w, v, _ in BIAS_STRADDLES])
def test_quant_bias_straddles_the_direct_path(ctx, oracle, which, value, direct):
    wl = _entries_frame(74)
    assert (np.abs(wl.coeffs) == 2).any()    # bias3 = 4: 2 - 4/2 = +0, the table's signed-zero case
    b = list(DEFAULT_BIASES)
    if which == "c":
        b[0] = b[1] = b[2] = float(value)
    else:
        b[3] = float(value)
    hdr = dict(quant_biases=b)
    want = oracle_frame(oracle, wl, hdr)
    k1 = run_forms(ctx, wl, want, f"bias{which} = {value!r}", hdr)
    fb = sum(k1["slots"]["fallback_batches"].values())
    assert (fb > 0) == direct, f"bias{which} = {value!r}: direct path {'expected' if direct else 'not expected'}, " \
                               f"fallback batches {fb}"
    assert sum(k1["slots_dd"]["fallback_batches"].values()) == 0


@pytest.mark.parametrize("zero", [False, True], ids=["tables_ok", "zero_entry"])
def test_dequant_table_with_a_zero_entry(ctx, oracle, zero):
    wl = _entries_frame(75)
    tabs = [np.array(t, np.float32, copy=True) for t in wl.tables]
    if zero:
        tabs[0][5] = 0.0                 # DCT8, channel X, one HF weight
    want = oracle_frame(oracle, wl, tables=tabs)
    k1 = run_forms(ctx, wl, want, f"dequant table, zero entry {zero}", tables=tabs)
    fb = sum(k1["slots"]["fallback_batches"].values())
    assert (fb == 0) == zero, fb


# ------------------------------------------------------------------ density
DENSITIES = [(0.0, 0), (0.25, 30), (0.25, 30000), (0.6, 30), (0.6, 30000), (1.0, 30), (1.0, 30000)]


@pytest.mark.parametrize("mix", ["MIX_D1", "MIX_ALL", 24])
@pytest.mark.parametrize("density,mag", DENSITIES, ids=[f"{d}x{m}" for d, m in DENSITIES])
def test_density(ctx, oracle, mix, density, mag):
    """density 0: an all-zero frame; type 24 = 256x256 (one varblock per group)"""
    from jxl_rs_amd import synth
    m = {mix: 1.0} if isinstance(mix, int) else getattr(synth, mix)
    wl = synth.make_vardct(512, 512, mix=m, seed=81, epf_iters=1)
    rng = np.random.default_rng(int(density * 100) + mag)
    c = np.where(rng.random(wl.coeffs.shape) < density, rng.integers(-mag, mag + 1, size=wl.coeffs.shape), 0)
    wl = _with(wl, c.astype(np.int32))
    want = oracle_frame(oracle, wl)
    run_forms(ctx, wl, want, f"density {density}, +-{mag}, {mix}")


# ------------------------------------------------------------------ coverage
def test_k1_kernel_coverage():
    """Over the module's cases every K1 kernel ran at least once.  kernel_times() names the host-side launches
    (k_expand_sparse, k_entries_to_pairs); the class kernels are seen through the work-list counters
    (k1_counters()) of the form that ran them: a class with varblocks ran its k1_dct8 / k1_dct16_32 / k1_special /
    k1_large_* kernels in that form, fallback batches are the fallback launch, dense-route varblocks the one-launch
    form of the routed groups."""
    assert SEEN["forms"], "runs after the module's other tests"
    names = ["dct8", "dct16x8", "dct8x16", "dct16x16", "dct32x8", "dct8x32", "dct32x16", "dct16x32", "dct32x32",
             "special", "large"]
    missing = [k for k in names if SEEN["varblocks"].get(k, 0) == 0]
    assert not missing, missing
    for form in FORMS:
        assert SEEN["forms"].get(form, {}).get("varblocks", 0) > 0, form
    assert SEEN["forms"]["slots"]["fallback_batches"] > 0, "the fallback launch"
    assert SEEN["dense_route_varblocks"] > 0, "routed groups (wide values, accumulated passes)"
    for k in ("k1_vardct", "k_expand_sparse", "k_entries_to_pairs"):
        assert k in SEEN["kernels"], (k, sorted(SEEN["kernels"]))
