"""Dense-slab K1, the 16..32-point class kernel (csrc/k_vardct.hip: run_dct_class on dense slabs) at the places where its
batch geometry can go wrong.  The dense form runs the classes with a 32-point side at half the varblocks per batch of
the entries form (32x32: 1, 32x16 / 16x32: 2, 8x32 / 32x8: 4), requests all three channels' coefficients of a batch
together and dequantises X and B right behind Y, with the batch's own dequantised Y for their chroma-from-luma; the
finished X values wait in registers and the B values in LDS while the channels before them are transformed.

Every case compares helpers.run_gpu_frame with helpers.run_oracle_frame bit for bit.
  - one transform type per frame, on one group and on two (a class list that continues across groups)
  - partial last batches and classes of exactly one varblock (lanes of a batch without a varblock): hand-placed maps,
    the counts asserted
  - the d1 mix with wide chroma-from-luma factors, a raw_quant spread and extreme coefficients at both ends of varblocks
  - both output layouts (8x8-tiled planes for the filters, raster planes read directly)
  - a group routed to its dense slab inside a slot-form frame (k1_dct16_32<kFormDense, false, true>: kK1Dct1632DenseAll
    of csrc/k1_plan.h)
"""
import copy

import numpy as np
import pytest

from helpers import bit_equal, diff_report, gpu_params_from, run_gpu_frame, run_oracle_frame

pytestmark = pytest.mark.gpu

# varblocks per batch of the dense class kernels (csrc/k_vardct.hip: the Shape aliases k1_dct8 / k1_dct16_32 run on dense slabs)
DENSE_NB = {0: 8, 4: 4, 5: 1, 6: 8, 7: 8, 8: 4, 9: 4, 10: 2, 11: 2}
NAME = {0: "dct8", 4: "dct16x16", 5: "dct32x32", 6: "dct16x8", 7: "dct8x16", 8: "dct32x8", 9: "dct8x32", 10: "dct32x16",
        11: "dct16x32"}
LAYOUTS = [dict(gab=True, epf_iters=2), dict(gab=False, epf_iters=0)]
LAYOUT_IDS = ["tiled", "raster"]


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


def _counts(wl):
    """varblocks per transform type, from the map (bit 7 = a varblock's first block)"""
    first = wl.transform_map[wl.transform_map >= 128] & 127
    return {int(t): int(n) for t, n in zip(*np.unique(first, return_counts=True))}


def _hold(ctx, oracle, wl, what, **over):
    """the frame on the device against the oracle; returns the device's work-list counters"""
    want, _ = run_oracle_frame(oracle, wl, **over)
    for c in range(3):
        assert np.isfinite(want[c]).all(), f"{what}: the oracle's plane {c} is not finite"
    ctx.kernel_timing_reset()
    ctx.kernel_timing(True)
    got, _ = run_gpu_frame(ctx, wl, **over)
    k1 = ctx.k1_counters()
    ctx.kernel_timing(False)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"{what}, plane {c}: {diff_report(got[c], want[c])}"
    have = _counts(wl)
    for t, name in NAME.items():
        assert k1["varblocks"][name] == have.get(t, 0), (what, name, k1["varblocks"], have)
    return k1


# ------------------------------------------------------------------ one transform type per frame
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("size", [(256, 256), (512, 256)], ids=["1group", "2groups"])
@pytest.mark.parametrize("ttype", [4, 5, 6, 7, 8, 9, 10, 11])
def test_one_type_per_frame(ctx, oracle, ttype, size, layout):
    from jxl_rs_amd import synth
    wl = synth.make_vardct(*size, mix={ttype: 1.0}, seed=200 + ttype, **layout)
    n = _counts(wl).get(ttype, 0)
    assert n >= 2 * DENSE_NB[ttype] * (size[0] // 256), f"type {ttype}: {n} varblocks"
    assert np.any(wl.ytox != 0) and np.any(wl.ytob != 0)
    _hold(ctx, oracle, wl, f"type {ttype}, {size}, {layout}")


# ------------------------------------------------------------------ partial last batches, classes of one varblock
def _place(wl, want):
    """a frame of 8x8 DCTs with want = {type: count} larger varblocks placed by hand in group 0: each at the first free
    position (raster order) aligned to its own size.  Coefficients stay where they are: varblocks lie back to back in
    raster order of their first block, whatever the map says, and any slab content is valid input."""
    from jxl_rs_amd import synth
    assert set(_counts(wl)) == {0}
    tmap, rq = wl.transform_map.copy(), wl.raw_quant.copy()
    bw, bh = min(32, wl.xblocks), min(32, wl.yblocks)
    free = np.ones((bh, bw), dtype=bool)
    for t, n in sorted(want.items(), key=lambda kv: -synth.COVERED_X[kv[0]] * synth.COVERED_Y[kv[0]]):
        cx, cy = synth.COVERED_X[t], synth.COVERED_Y[t]
        spots = [(x, y) for y in range(0, bh - cy + 1, cy) for x in range(0, bw - cx + 1, cx)]
        for _ in range(n):
            x, y = next((x, y) for x, y in spots if free[y:y + cy, x:x + cx].all())
            free[y:y + cy, x:x + cx] = False
            tmap[y:y + cy, x:x + cx] = t
            tmap[y, x] = t | 0x80
            rq[y:y + cy, x:x + cx] = rq[y, x]
    w2 = copy.copy(wl)
    w2.transform_map, w2.raw_quant = tmap, rq
    return w2


# {type: varblocks}: NB + 1 (a full batch and a partial one) or exactly one (a partial batch with nothing behind it);
# 32x32 runs one varblock per batch: one batch, and two
PLACEMENTS = [{5: 1, 10: 3, 11: 1, 8: 5, 9: 1, 4: 5, 6: 9, 7: 1},
              {5: 2, 10: 1, 11: 3, 8: 1, 9: 5, 4: 1, 6: 1, 7: 9}]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("want", PLACEMENTS, ids=["a", "b"])
def test_partial_batches(ctx, oracle, want, layout):
    """264 x 200: 33 x 25 blocks, a second group of one block column; the large varblocks sit in group 0"""
    from jxl_rs_amd import synth
    wl = _place(synth.make_vardct(264, 200, mix=synth.MIX_DCT8, seed=31, **layout), want)
    have = _counts(wl)
    for t, n in want.items():
        assert have[t] == n, (t, have)
        assert n == 1 or n % DENSE_NB[t] != 0 or DENSE_NB[t] == 1, (t, n)
    assert sum(1 for n in want.values() if n == 1) >= 3
    assert have[0] % DENSE_NB[0] != 0, have[0]
    _hold(ctx, oracle, wl, f"hand-placed {want}, {layout}")


# ------------------------------------------------------------------ the d1 mix at the ends of its inputs
EXTREMES = [1, -1, 32767, -32767, 2**30, -2**30]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_d1_group_extremes(ctx, oracle, layout):
    from jxl_rs_amd import synth
    wl = synth.make_vardct(256, 256, mix=synth.MIX_D1, seed=41, **layout)
    rng = np.random.default_rng(41)
    have = _counts(wl)
    assert all(have.get(t, 0) > 0 for t in NAME), have
    # chroma-from-luma factors at the ends of their range, different from tile to tile: a batch mixes varblocks of
    # several colour tiles, and the Y a lane multiplies by them must be this batch's
    wl.ytox = rng.choice(np.array([-128, -77, 5, 127], np.int8), size=wl.ytox.shape).astype(np.int8)
    wl.ytob = rng.choice(np.array([-128, -3, 90, 127], np.int8), size=wl.ytob.shape).astype(np.int8)
    wl.raw_quant = np.where(wl.raw_quant > 0, rng.choice(np.array([1, 2, 7, 16, 100, 256]), size=wl.raw_quant.shape),
                            0).astype(np.int32)
    # extreme coefficients at the first and the last position of every varblock, all three channels
    coeffs = wl.coeffs.copy()
    off, k = 0, 0
    for by in range(wl.yblocks):
        for bx in range(wl.xblocks):
            raw = int(wl.transform_map[by, bx])
            if raw < 128:
                continue
            n = synth.COVERED_X[raw & 127] * synth.COVERED_Y[raw & 127] * 64
            for c in range(3):
                coeffs[0, c, off] = EXTREMES[(k + 2 * c) % 6]
                coeffs[0, c, off + n - 1] = EXTREMES[(k + 2 * c + 3) % 6]
            k += 1
            off += n
    assert off == 65536
    assert all((coeffs[0, c] == v).any() for v in EXTREMES for c in range(3))
    wl.coeffs = coeffs
    # inv_global_scale = 1: |q| = 2^30 stays far inside f32 through the IDCT
    _hold(ctx, oracle, wl, f"d1 group with extreme inputs, {layout}", global_scale=65536)


# ------------------------------------------------------------------ routed groups
def test_routed_group(ctx, oracle):
    """one group arrives as a dense slab, the others slot-bucketed: the frame stays in the in-place form and the routed
    group's DCT classes run through the one-launch dense form"""
    from jxl_rs_amd import lib as jl
    from jxl_rs_amd import synth
    wl = synth.make_vardct(1024, 256, mix=synth.MIX_D1, seed=51, epf_iters=2)
    ng = wl.coeffs.shape[0]
    want, _ = run_oracle_frame(oracle, wl)
    g_dense = 2
    parts = [jl.host_pack_slots(wl.coeffs[g], group_id=g) for g in range(ng)]
    assert all(len(q[3]) == 0 for q in parts)
    slotted = [g for g in range(ng) if g != g_dense]
    ctx.kernel_timing_reset()
    ctx.kernel_timing(True)
    p = gpu_params_from(ctx, wl)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.submit_groups_slots(np.asarray(slotted, dtype=np.uint32), np.concatenate([parts[g][0] for g in slotted]),
                            np.concatenate([parts[g][1].reshape(-1) for g in slotted]),
                            np.concatenate([parts[g][2] for g in slotted]), None)
    ctx.submit_group(g_dense, wl.coeffs[g_dense])
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    k1 = ctx.k1_counters()
    ctx.kernel_timing(False)
    for c in range(3):
        assert bit_equal(got[c], want[c]), f"routed group, plane {c}: {diff_report(got[c], want[c])}"
    routed = k1["dense_route_varblocks"]
    tm = wl.transform_map[:, g_dense * 32:(g_dense + 1) * 32]
    first = tm[tm >= 128] & 127
    for t, name in NAME.items():
        assert routed[name] == int((first == t).sum()), (name, routed)
    assert all(routed[NAME[t]] > 0 for t in (5, 10, 11, 8, 9, 4)), routed
