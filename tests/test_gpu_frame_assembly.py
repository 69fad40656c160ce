"""A VarDCT frame assembled the way a decoder assembles it: jxlh_frame_set_lf_quantized, jxlh_frame_set_lf and
jxlh_frame_set_hf_meta called once per rect -- LF groups, ragged rects at odd origins, caller row strides wider than the
rect (the padding poisoned), an extra_precision per rect, host and device pointers, any order against each other and
against the coefficient submissions -- instead of once per frame at the origin with a tight stride.

The truth of every case is the CPU oracle on the whole arrays (helpers.run_oracle_frame); every case compares the LF
image (smoothed where smoothing is on) and 100 % of the samples of the three planes bit for bit.  The one restriction:
with LF smoothing off, the LF of a sub-sampled channel is compared on the samples the channel holds (the top-left
corner of each LF group's rect, helpers.subsampled_corner_mask -- geometry, never data)."""
import time

import numpy as np
import pytest

from helpers import (bit_equal, diff_report, gpu_params_from, lf_group_rects, lf_piece, oracle_lf_piece, ragged_lf_rects,
                     ragged_map_rects, rects_cover, run_oracle_frame, subsampled_corner_mask, upload_frame_piecewise)

pytestmark = pytest.mark.gpu
STRIP = 4  # JXLH_FRAME_STRIP


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


_FRAMES = {}
ORACLE_SECONDS = {}  # the oracle's wall time per frame (printed by the last test of the module)


def _frame(oracle, w, h, mix, seed, **opts):
    """the workload and what the oracle makes of it, once per module"""
    from jxl_rs_amd import synth
    key = (w, h, mix, seed, tuple(sorted(opts.items())))
    if key not in _FRAMES:
        wl = synth.make_vardct(w, h, mix=getattr(synth, mix), seed=seed, **opts)
        t0 = time.time()
        want, want_lf = run_oracle_frame(oracle, wl, num_threads=16)
        ORACLE_SECONDS[f"{w}x{h} {mix}"] = max(ORACLE_SECONDS.get(f"{w}x{h} {mix}", 0.0), time.time() - t0)
        _FRAMES[key] = (wl, want, want_lf)
    return _FRAMES[key]


def _check(ctx, want, want_lf, what, lf_masks=None, run=True):
    if run:
        ctx.frame_run()
        ctx.sync()
    got, got_lf = ctx.read_planes(), ctx.read_lf()
    for c in range(3):
        if lf_masks is None:
            assert bit_equal(got_lf[c], want_lf[c]), f"{what}: LF ch{c}: {diff_report(got_lf[c], want_lf[c])}"
        else:
            m = lf_masks[c]
            assert bit_equal(got_lf[c][m], want_lf[c][m]), f"{what}: LF ch{c} on the samples the channel holds"
        assert got[c].shape == want[c].shape
        assert bit_equal(got[c], want[c]), f"{what}: plane {c}: {diff_report(got[c], want[c])}"


def _scrub(ctx, wl):
    """Renders a flat frame of the same size first.  A case that repeats a frame on one context would otherwise find
    the right pixels already in the buffers a wrongly skipped kernel fails to write."""
    from copy import copy
    from helpers import run_gpu_frame
    flat = copy(wl)
    flat.coeffs = np.zeros_like(wl.coeffs)
    flat.lf_q = [np.full_like(q, 3) for q in wl.lf_q]
    flat.transform_map = np.full_like(wl.transform_map, 0x80)  # DCT8 everywhere
    flat.raw_quant = np.ones_like(wl.raw_quant)
    flat.epf_map = np.zeros_like(wl.epf_map)
    flat.ytox, flat.ytob = np.zeros_like(wl.ytox), np.zeros_like(wl.ytob)
    run_gpu_frame(ctx, flat)


def _ep_by_index(shift):
    return lambda i, rect: (i + shift) % 4


# ---------------------------------------------------------------- a. LF-group assembly, 4:4:4
LF_GROUP_FRAMES = [
    # (w, h, mix, epf_iters, flags to run, extra_precision of LF group i = (i + shift) % 4)
    (2304, 2120, "MIX_ALL", 2, (0,), 0),     # 2 x 2 LF groups: all four precisions in one frame
    (2100, 300, "MIX_D1", 3, (0, 1), 1),     # 2 x 1
    (300, 2100, "MIX_ALL", 3, (0, 1), 2),    # 1 x 2
]


@pytest.mark.parametrize("lf_mode", ["quantized", "float", "mixed"])
@pytest.mark.parametrize("case", LF_GROUP_FRAMES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-epf{c[3]}")
def test_lf_group_assembly(ctx, oracle, case, lf_mode):
    """LF and maps arrive per LF group, shuffled, in padded arrays, each LF group with its own extra_precision; LF
    smoothing runs across the seams between the groups, where a wrong destination offset shows.  lf_mode float / mixed:
    (some of) the rects dequantised by the host and handed to jxlh_frame_set_lf."""
    w, h, mix, epf, flag_list, shift = case
    wl, want, want_lf = _frame(oracle, w, h, mix, seed=w + h, epf_iters=epf, lf_smoothing=True, unique_groups=10)
    rects = lf_group_rects(wl.xblocks, wl.yblocks)
    assert len(rects) > 1 and (rects_cover(rects, wl.xblocks, wl.yblocks) == 1).all()
    eps = {_ep_by_index(shift)(i, r) for i, r in enumerate(rects)}
    assert len(eps) == min(4, len(rects))
    as_float = {"quantized": False, "float": True, "mixed": lambda i, r: i % 2 == 0}[lf_mode]
    for flags in (flag_list if lf_mode == "quantized" else flag_list[:1]):
        upload_frame_piecewise(ctx, wl, rects, rects, order=w + flags, pitch_pad=7, extra_precision=_ep_by_index(shift),
                               lf_as_float=as_float, oracle=oracle, flags=flags)
        _check(ctx, want, want_lf, f"{w}x{h} {mix} per LF group, {lf_mode}, flags={flags}")


def test_all_four_precisions_are_exercised():
    """(the cases above between them use every extra_precision)"""
    seen = set()
    for w, h, _, _, _, shift in LF_GROUP_FRAMES:
        n = -(-w // 2048) * -(-h // 2048)
        seen |= {(i + shift) % 4 for i in range(n)}
    assert seen == {0, 1, 2, 3}


def test_low_bits_need_the_rects_own_precision(ctx, oracle):
    """quantised values that are not multiples of 1 << extra_precision: only (factor * inv_quant_lf) * mul of the rect's
    own precision dequantises them like the oracle does rect by rect (run_oracle_frame's lf= override)"""
    wl, _, _ = _frame(oracle, 520, 300, "MIX_D1", seed=3, epf_iters=1, lf_smoothing=True)
    rects = ragged_lf_rects(wl.xblocks, wl.yblocks, 11)
    ep = lambda i, r: (i * 7 + 1) % 4
    _, lf = upload_frame_piecewise(ctx, wl, rects, ragged_map_rects(wl.xblocks, wl.yblocks, 11), pitch_pad=3,
                                   extra_precision=ep, low_bits=5, oracle=oracle)
    whole = oracle_lf_piece(oracle, wl, wl.lf_q)
    assert not all(bit_equal(lf[c], whole[c]) for c in range(3)), "the low bits changed nothing"
    want, want_lf = run_oracle_frame(oracle, wl, lf=lf)
    _check(ctx, want, want_lf, "low bits below the rect's precision")


# ---------------------------------------------------------------- b. + c. ragged rects on small frames
RAGGED = [(520, 300, "MIX_ALL", 2), (777, 513, "MIX_D1", 3), (66, 34, "MIX_ALL", 2)]


@pytest.mark.parametrize("lf_mode", ["quantized", "float", "mixed"])
@pytest.mark.parametrize("case", RAGGED, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}-epf{c[3]}")
def test_ragged_rects(ctx, oracle, case, lf_mode):
    """LF rects at odd origins, 1 block wide / high among them, map rects 8-aligned that end inside colour tiles their
    neighbours also deliver; sizes grow and shrink from call to call (the K0a staging buffer reallocates); one
    zero-sized rect of each kind"""
    w, h, mix, epf = case
    wl, want, want_lf = _frame(oracle, w, h, mix, seed=w * 3 + h, epf_iters=epf, lf_smoothing=True)
    xb, yb = wl.xblocks, wl.yblocks
    lf_rects = ragged_lf_rects(xb, yb, w) + [(xb // 2, yb // 2, 0, 3), (1, 1, 2, 0)]
    map_rects = ragged_map_rects(xb, yb, w) + [(8 * (xb // 16), 0, 0, 0)]
    sizes = [rw * rh for _, _, rw, rh in lf_rects]
    assert any(a < b for a, b in zip(sizes, sizes[1:])) and any(a > b for a, b in zip(sizes, sizes[1:]))
    as_float = {"quantized": False, "float": True, "mixed": lambda i, r: i % 3 == 1}[lf_mode]
    for flags in (0, 1):
        upload_frame_piecewise(ctx, wl, lf_rects, map_rects, order=h + flags, pitch_pad=5,
                               extra_precision=lambda i, r: (i * 5 + 2) % 4, lf_as_float=as_float, oracle=oracle,
                               flags=flags)
        _check(ctx, want, want_lf, f"{w}x{h} ragged rects, {lf_mode}, flags={flags}")


# ---------------------------------------------------------------- d. transform families seen in one rect only
def _families_frame(oracle):
    """768 x 512 (3 x 2 groups): small aligned DCTs everywhere (closed inside their 64x64 tiles), but group 1 alone holds
    large transforms (types 18..26) and group 4 alone special ones (types 1..3, 12..17)"""
    from jxl_rs_amd import synth
    key = "families"
    if key not in _FRAMES:
        kw = dict(epf_iters=2, gab=True, aligned=True)
        wl = synth.make_vardct(768, 512, mix=synth.MIX_D1, seed=31, **kw)
        large = synth.make_vardct(768, 512, mix={0: 0.4, 18: 0.2, 21: 0.2, 22: 0.1, 24: 0.1}, seed=32, **kw)
        special = synth.make_vardct(768, 512, mix=synth.MIX_8X8, seed=33, **kw)
        for g, src in ((1, large), (4, special)):
            ys, xs = slice((g // 3) * 32, (g // 3) * 32 + 32), slice((g % 3) * 32, (g % 3) * 32 + 32)
            wl.transform_map[ys, xs] = src.transform_map[ys, xs]
            wl.raw_quant[ys, xs] = src.raw_quant[ys, xs]
            wl.coeffs[g] = src.coeffs[g]
        t = wl.transform_map & 127
        lg, sp = t >= 18, ((t >= 1) & (t <= 3)) | ((t >= 12) & (t <= 17))
        assert lg[0:32, 32:64].any() and lg.sum() == lg[0:32, 32:64].sum()
        assert sp[32:64, 32:64].any() and sp.sum() == sp[32:64, 32:64].sum()
        want, want_lf = run_oracle_frame(oracle, wl)
        _FRAMES[key] = (wl, want, want_lf)
    return _FRAMES[key]


# the six group rects; L = 1 holds the large transforms, S = 4 the special ones
FAMILY_ORDERS = {"large-first_special-middle": [1, 0, 2, 4, 3, 5], "large-middle_special-last": [0, 2, 1, 3, 5, 4],
                 "large-last_special-first": [4, 0, 2, 3, 5, 1]}


@pytest.mark.parametrize("mode", ["two-kernel", "strip", "strip-device-maps"])
@pytest.mark.parametrize("order", sorted(FAMILY_ORDERS))
def test_family_seen_in_one_rect_only(ctx, oracle, order, mode):
    """which class kernels a frame launches at all (has_special, has_large) and whether the strip kernel may skip them
    (every rect closed) are facts gathered across the rects: the one rect that holds the family / breaks the rule
    arrives first, in the middle, or last"""
    wl, want, want_lf = _families_frame(oracle)
    rects = [(x, y, 32, 32) for y in (0, 32) for x in (0, 32, 64)]
    seq = FAMILY_ORDERS[order]
    flags = 0 if mode == "two-kernel" else STRIP
    _scrub(ctx, wl)
    p = gpu_params_from(ctx, wl, flags=flags)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    upload_frame_piecewise(ctx, wl, [], rects, order=seq, pitch_pad=4, begin=False, submit=False,
                           on_device=mode == "strip-device-maps")
    upload_frame_piecewise(ctx, wl, lf_group_rects(wl.xblocks, wl.yblocks), [], begin=False)
    _check(ctx, want, want_lf, f"families, {order}, {mode}")
    if flags:
        ran, tiles, by_class = ctx.frame_path()
        assert ran and 0 < by_class < tiles, (ran, tiles, by_class)


# ---------------------------------------------------------------- e. device-pointer inputs
@pytest.mark.parametrize("lf_as_float", [False, True], ids=["quantized", "float"])
def test_device_pointer_inputs(ctx, oracle, lf_as_float):
    """LF and all five maps handed over as device pointers into pitched device buffers (hipMemcpyDefault both ways in
    copy2d; a device-resident transform map is not inspected)"""
    wl, want, want_lf = _frame(oracle, 777, 513, "MIX_ALL", seed=8, epf_iters=2, lf_smoothing=True)
    xb, yb = wl.xblocks, wl.yblocks
    upload_frame_piecewise(ctx, wl, ragged_lf_rects(xb, yb, 2), ragged_map_rects(xb, yb, 2), order=9, pitch_pad=6,
                           extra_precision=lambda i, r: i % 4, lf_as_float=lf_as_float, on_device=True, oracle=oracle)
    _check(ctx, want, want_lf, f"device pointers, lf_as_float={lf_as_float}")


# ---------------------------------------------------------------- f. order against the rest of the frame
def test_maps_before_lf_and_setters_between_submissions(ctx, oracle):
    """the header orders nothing between the setters and the submissions inside a frame: maps first, coefficients
    before / between / after the rects"""
    wl, want, want_lf = _frame(oracle, 520, 300, "MIX_ALL", seed=14, epf_iters=2, lf_smoothing=True)
    xb, yb = wl.xblocks, wl.yblocks
    lf_rects, map_rects = ragged_lf_rects(xb, yb, 6), ragged_map_rects(xb, yb, 6)
    ng = wl.coeffs.shape[0]
    nl, nm = len(lf_rects), len(map_rects)

    def submit(groups):
        for g in groups:
            ctx.submit_group(g, wl.coeffs[g], slot=g % 2)

    def rects(lf_idx, map_idx, **kw):
        upload_frame_piecewise(ctx, wl, [lf_rects[i] for i in lf_idx], [map_rects[i] for i in map_idx], pitch_pad=2,
                               begin=False, submit=False, **kw)

    def begin():
        ctx.frame_begin(gpu_params_from(ctx, wl))
        ctx.set_dequant_tables(wl.tables)

    def finish(what):
        ctx.slot_wait(0)
        ctx.slot_wait(1)
        _check(ctx, want, want_lf, what)

    begin()   # maps, then LF, then coefficients
    rects([], range(nm))
    rects(range(nl), [])
    submit(range(ng))
    finish("maps before LF")
    begin()   # coefficients first
    submit(range(ng))
    rects(range(nl), range(nm), order=3)
    finish("coefficients before every rect")
    begin()   # everything interleaved
    submit(range(0, ng, 2))
    rects(range(0, nl, 2), range(1, nm, 2))
    submit(range(1, ng, 4))
    rects(range(1, nl, 2), range(0, nm, 2), extra_precision=2)
    submit(range(3, ng, 4))
    finish("rects between the submissions")


def test_rect_delivered_twice_last_one_wins(ctx, oracle):
    """a rect set with wrong data and then again with the right data: the frame holds the later call's"""
    from copy import copy
    wl, want, want_lf = _frame(oracle, 520, 300, "MIX_ALL", seed=14, epf_iters=2, lf_smoothing=True)
    xb, yb = wl.xblocks, wl.yblocks
    lf_rects, map_rects = ragged_lf_rects(xb, yb, 7), ragged_map_rects(xb, yb, 7)
    rng = np.random.default_rng(5)
    bad = copy(wl)
    bad.lf_q = [q + rng.integers(-40, 41, size=q.shape, dtype=np.int32) for q in wl.lf_q]
    bad.raw_quant = wl.raw_quant + 3
    bad.epf_map = (wl.epf_map + 1) & 7
    bad.transform_map = np.where(wl.transform_map & 128, 128, 0).astype(np.uint8)  # every first block a DCT8
    bad.ytox, bad.ytob = (-wl.ytox).astype(np.int8), (wl.ytob // 2).astype(np.int8)
    upload_frame_piecewise(ctx, bad, lf_rects[1::2], map_rects[::2], pitch_pad=1, submit=False)
    upload_frame_piecewise(ctx, wl, lf_rects, map_rects, order=2, pitch_pad=1, extra_precision=1, begin=False)
    _check(ctx, want, want_lf, "every second rect delivered twice")


def _groups_touched(wl, rect, reach=1):
    """the 256x256 groups holding a block within `reach` blocks of the rect (LF smoothing reads a 3x3 neighbourhood)"""
    x0, y0, w, h = rect
    gx = range(max(0, x0 - reach) // 32, min(wl.xblocks - 1, x0 + w - 1 + reach) // 32 + 1)
    gy = range(max(0, y0 - reach) // 32, min(wl.yblocks - 1, y0 + h - 1 + reach) // 32 + 1)
    return [y * wl.xgroups + x for y in gy for x in gx]


@pytest.mark.parametrize("how", ["frame_run", "rerender_groups"])
@pytest.mark.parametrize("as_float", [False, True], ids=["quantized", "float"])
def test_lf_rect_replaced_after_a_run(ctx, oracle, how, as_float):
    """an LF rect replaced after jxlh_frame_run: the next render smooths again from the raw LF image and equals the
    oracle on the new LF -- through a whole run, and through jxlh_frame_rerender_groups of the groups the changed
    samples (and their smoothing neighbours) lie in"""
    from copy import copy
    wl, want, want_lf = _frame(oracle, 777, 513, "MIX_D1", seed=19, epf_iters=2, lf_smoothing=True)
    _scrub(ctx, wl)
    upload_frame_piecewise(ctx, wl, lf_group_rects(wl.xblocks, wl.yblocks), lf_group_rects(wl.xblocks, wl.yblocks))
    _check(ctx, want, want_lf, "before the replacement")
    rect = (29, 30, 9, 5)   # across a group corner: blocks 29..37 x 30..34
    new = copy(wl)
    new.lf_q = [q.copy() for q in wl.lf_q]
    rng = np.random.default_rng(1)
    for q in new.lf_q:
        q[30:35, 29:38] += rng.integers(-3, 4, size=(5, 9), dtype=np.int32)
    want2, want_lf2 = run_oracle_frame(oracle, new)
    assert not bit_equal(want_lf2[1], want_lf[1])
    upload_frame_piecewise(ctx, new, [rect], [], pitch_pad=3, extra_precision=3, lf_as_float=as_float, oracle=oracle,
                           begin=False, submit=False)
    if how == "frame_run":
        ctx.frame_run()
    else:
        touched = _groups_touched(wl, rect)
        assert len(touched) == 4 and len(touched) < wl.coeffs.shape[0]
        ctx.rerender_groups(touched)
    ctx.sync()
    _check(ctx, want2, want_lf2, f"LF rect replaced, then {how}", run=False)


# ---------------------------------------------------------------- g. sub-sampled frames per LF group
SUBSAMPLINGS = {"420": ((1, 0, 1), (1, 0, 1)), "422": ((1, 0, 1), (0, 0, 0)), "440": ((0, 0, 0), (1, 0, 1)),
                "mixed": ((1, 0, 0), (0, 0, 1))}
SUB_FRAMES = [(40, 2100, "420"), (40, 2100, "422"), (40, 2100, "440"), (40, 2100, "mixed"), (2100, 40, "mixed"),
              (2100, 2100, "420"), (2100, 2100, "mixed")]


def _sub_frame(oracle, w, h, sub, smoothing):
    """A sub-sampled workload whose chroma LF holds data only where the channel has samples.  Returns (the workload
    the device gets, planes, LF of the oracle, masks): with smoothing off the device's copy is poisoned outside the
    corners while the oracle's holds zeros; with smoothing on both hold zeros (the reference's LF image is
    zero-initialised and dequant_lf writes the corner only)."""
    from copy import copy
    from jxl_rs_amd import synth
    key = ("sub", w, h, sub, smoothing)
    if key not in _FRAMES:
        hs, vs = SUBSAMPLINGS[sub]
        wl = synth.make_vardct(w, h, mix=synth.MIX_8X8, seed=w + 5 * h, hshift=hs, vshift=vs, epf_iters=1, gab=True,
                               lf_smoothing=smoothing, unique_groups=6)
        masks = [subsampled_corner_mask(wl, c) for c in range(3)]
        assert any(not m.all() for m in masks)
        coded = (1, 0, 2)  # lf_q is in coded order Y, X, B
        zeroed = copy(wl)
        zeroed.lf_q = [np.where(masks[coded[i]], q, 0).astype(np.int32) for i, q in enumerate(wl.lf_q)]
        dev = zeroed
        if not smoothing:
            dev = copy(wl)
            dev.lf_q = [np.where(masks[coded[i]], q, 0x7fffffff).astype(np.int32) for i, q in enumerate(wl.lf_q)]
        t0 = time.time()
        want, want_lf = run_oracle_frame(oracle, zeroed, num_threads=16)
        ORACLE_SECONDS[f"{w}x{h} {sub}"] = time.time() - t0
        _FRAMES[key] = (dev, want, want_lf, masks)
    return _FRAMES[key]


@pytest.mark.parametrize("smoothing", [False, True], ids=["raw", "smoothed"])
@pytest.mark.parametrize("w,h,sub", SUB_FRAMES, ids=lambda v: str(v))
def test_subsampled_frame_per_lf_group(ctx, oracle, w, h, sub, smoothing):
    """the chroma LF of a sub-sampled frame sits in the top-left corner of each LF group's rect; frames crossing an LF
    group vertically and both ways, delivered per LF group, dense and as pairs.  Smoothing off: what lies outside the
    corners is never read (poison there on the device, zeros for the oracle).  Smoothing on: it is read, and zeros --
    what the reference's LF image holds there -- give the reference's result."""
    from jxl_rs_amd import synth
    dev, want, want_lf, masks = _sub_frame(oracle, w, h, sub, smoothing)
    rects = lf_group_rects(dev.xblocks, dev.yblocks)
    assert len(rects) > 1
    ng = dev.coeffs.shape[0]
    for form in ("dense", "pairs"):
        if form == "pairs" and ng > 9 and smoothing:
            continue  # (the large frames as pairs once)
        upload_frame_piecewise(ctx, dev, rects, rects, order=w + h, pitch_pad=3, extra_precision=lambda i, r: (i + 1) % 4,
                               submit=form == "dense")
        if form == "pairs":
            for g in range(ng):
                ctx.submit_group_sparse(g, *synth.to_sparse(dev.coeffs[g]))
            ctx.slot_wait(0)
        _check(ctx, want, want_lf, f"{w}x{h} {sub} smoothing={smoothing} {form}", lf_masks=None if smoothing else masks)


@pytest.mark.parametrize("w,h,sub", [(40, 2100, "420"), (2100, 2100, "mixed")], ids=lambda v: str(v))
def test_subsampled_frame_float_lf_with_nan_outside_the_corners(ctx, oracle, w, h, sub):
    """the same through jxlh_frame_set_lf: NaN outside the corners, smoothing off"""
    dev, want, want_lf, masks = _sub_frame(oracle, w, h, sub, False)
    p = gpu_params_from(ctx, dev)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(dev.tables)
    rects = lf_group_rects(dev.xblocks, dev.yblocks)
    for i in np.random.default_rng(w).permutation(len(rects)):
        x0, y0, rw, rh = rect = rects[i]
        lf = oracle_lf_piece(oracle, dev, lf_piece(dev, rect))
        lf = [np.where(masks[c][y0:y0 + rh, x0:x0 + rw], lf[c], np.float32(np.nan)) for c in range(3)]
        big = [np.full((rh, rw + 4), np.nan, dtype=np.float32) for _ in range(3)]
        for c in range(3):
            big[c][:, 1:1 + rw] = lf[c]
        ctx.set_lf(*[b[:, 1:1 + rw] for b in big], x0=x0, y0=y0)
    upload_frame_piecewise(ctx, dev, [], rects, begin=False)
    _check(ctx, want, want_lf, f"{w}x{h} {sub} float LF", lf_masks=masks)


# ---------------------------------------------------------------- h. argument errors
def test_invalid_calls_return_their_status_and_leave_the_frame_intact(ctx, oracle):
    """every invalid call comes back with its documented status, in the middle of an assembly that then finishes and
    still equals the oracle"""
    import jxl_rs_amd
    from jxl_rs_amd import lib, JxlHipError
    wl, want, want_lf = _frame(oracle, 520, 300, "MIX_ALL", seed=14, epf_iters=2, lf_smoothing=True)
    xb, yb = wl.xblocks, wl.yblocks
    assert (xb, yb) == (65, 38)
    lf_rects, map_rects = ragged_lf_rects(xb, yb, 8), ragged_map_rects(xb, yb, 8)
    upload_frame_piecewise(ctx, wl, lf_rects[::2], map_rects[::2], pitch_pad=2, submit=False)

    qi = [np.full((16, 24), 0x7fffffff, dtype=np.int32) for _ in range(3)]
    qf = [np.full((16, 24), np.nan, dtype=np.float32) for _ in range(3)]
    tm, em = np.full((16, 24), 0xff, dtype=np.uint8), np.full((16, 24), 0xff, dtype=np.uint8)
    cm = [np.full((4, 6), 0x7f, dtype=np.int8) for _ in range(2)]
    ai = [a.ctypes.data for a in qi]    # raw pointers: the binding passes w, h and the strides through as given
    af = [a.ctypes.data for a in qf]
    am = [tm.ctypes.data, qi[0].ctypes.data, em.ctypes.data, cm[0].ctypes.data, cm[1].ctypes.data]

    def refused(status, call, *a, **kw):
        with pytest.raises(JxlHipError) as e:
            call(*a, **kw)
        assert e.value.status == status, (e.value, a, kw)

    inv = lib.ERR_INVALID_ARGUMENT
    # stride < w
    refused(inv, ctx.set_lf_quantized, *ai, x0=0, y0=0, w=24, h=16, stride=23)
    refused(inv, ctx.set_lf, *af, x0=0, y0=0, w=24, h=16, stride=23)
    refused(inv, ctx.set_hf_meta, *am, x0=0, y0=0, w=24, h=16, map_stride=23, cmap_stride=6)
    # a rect that leaves the frame (to the right, below, and by an origin beyond it)
    for x0, y0, w, h in ((xb - 23, 0, 24, 16), (0, yb - 15, 24, 16), (xb + 1, 0, 0, 0), (0, 0xFFFFFFF0, 24, 16)):
        refused(inv, ctx.set_lf_quantized, *ai, x0=x0, y0=y0, w=w, h=h, stride=24)
        refused(inv, ctx.set_lf, *af, x0=x0, y0=y0, w=w, h=h, stride=24)
    for x0, y0, w, h in ((48, 0, 24, 16), (0, 24, 24, 16), (72, 0, 0, 0)):
        refused(inv, ctx.set_hf_meta, *am, x0=x0, y0=y0, w=w, h=h, map_stride=24, cmap_stride=6)
    # map origins off the colour-tile grid
    refused(inv, ctx.set_hf_meta, *am, x0=4, y0=0, w=24, h=16, map_stride=24, cmap_stride=6)
    refused(inv, ctx.set_hf_meta, *am, x0=0, y0=9, w=24, h=16, map_stride=24, cmap_stride=6)
    # cmap_stride < ceil(w / 8)
    refused(inv, ctx.set_hf_meta, *am, x0=0, y0=0, w=17, h=16, map_stride=24, cmap_stride=2)
    # extra_precision > 3
    refused(inv, ctx.set_lf_quantized, *ai, x0=0, y0=0, w=24, h=16, stride=24, extra_precision=4)
    # a null plane
    refused(inv, ctx.set_lf_quantized, ai[0], 0, ai[2], x0=0, y0=0, w=24, h=16, stride=24)
    # outside a frame
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        refused(lib.ERR_BAD_STATE, fresh.set_lf_quantized, *ai, x0=0, y0=0, w=24, h=16, stride=24)
        refused(lib.ERR_BAD_STATE, fresh.set_lf, *af, x0=0, y0=0, w=24, h=16, stride=24)
        refused(lib.ERR_BAD_STATE, fresh.set_hf_meta, *am, x0=0, y0=0, w=24, h=16, map_stride=24, cmap_stride=6)
    finally:
        fresh.close()
    # legal: zero-sized rects, also at the frame's far corner
    ctx.set_lf_quantized(*ai, x0=xb, y0=yb, w=0, h=0, stride=24)
    ctx.set_lf(*af, x0=3, y0=5, w=0, h=7, stride=24)
    ctx.set_hf_meta(*am, x0=64, y0=32, w=0, h=0, map_stride=24, cmap_stride=6)

    upload_frame_piecewise(ctx, wl, lf_rects[1::2], map_rects[1::2], pitch_pad=2, begin=False)
    _check(ctx, want, want_lf, "assembly finished after the refused calls")


def test_zz_report_oracle_times():
    """(not a check: the oracle's wall time per frame of this module, for the record; shown with -s / -rP)"""
    for k, v in sorted(ORACLE_SECONDS.items(), key=lambda kv: -kv[1]):
        print(f"oracle {k}: {v:.2f} s")
