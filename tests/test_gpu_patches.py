"""Patches on the device (k_patches.hip) held bit for bit to the numpy restatement of the reference (patches_ref.py):
through the stage hook, and inside whole VarDCT frames -- reference slots filled from the host and saved from an earlier
frame, extra channels, upsampling, noise, repeated / banded / partial renders -- plus the dictionary's validation."""
import numpy as np
import pytest

import patches_ref as pr
from helpers import bit_equal, diff_report, run_oracle_frame, upload_frame
from test_patches_cpu import KAT, kat_row_planes

pytestmark = pytest.mark.gpu

ALPHA, ASSOC = pr.EC_ALPHA, pr.EC_ALPHA_ASSOCIATED


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def _begin(ctx, w, h):
    ctx.frame_begin(ctx.default_params(w, h))


def _planes(rng, n, h, w):
    return [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(n)]


def _assert_planes(got, want, what):
    for c, (g, e) in enumerate(zip(got, want)):
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


def _set_refs(ctx, refs):
    for s, planes in enumerate(refs):
        ctx.set_reference(s, planes)


# ---------------------------------------------------------------- stage hook
def _mode_grid(num_ec):
    """every colour mode x clamp x alpha channel, with extra-channel blendings cycling through every mode"""
    out = []
    k = 0
    for mode in range(8):
        for clamp in (False, True):
            for alpha in range(max(1, min(num_ec, 2))):
                ec = [((mode + 3 * i + k) % 8, (alpha + i + k) % max(num_ec, 1), bool((k + i) & 1)) for i in range(num_ec)]
                out.append([(mode, alpha, clamp)] + ec)
                k += 1
    return out


EC_SETS = [
    [],
    [ALPHA],
    [ALPHA | ASSOC],
    [0, ALPHA],
    [ALPHA | ASSOC, 0],
    [ALPHA, ALPHA | ASSOC],
    [0, 0],  # no alpha-type channel: the colour blend modes fall back
]


@pytest.mark.parametrize("flags", EC_SETS, ids=["ec%d_%s" % (len(f), "_".join(map(str, f))) for f in EC_SETS])
def test_stage_hook_every_mode(ctx, flags):
    num_ec = len(flags)
    rng = np.random.default_rng(11 + 7 * num_ec + sum(flags))
    w, h = 300, 220
    _begin(ctx, w, h)
    refs = [_planes(rng, 3 + num_ec, 64, 96) for _ in range(2)]
    # alpha pairs that make new_a == 0: zero alpha on both sides over part of the slot and the image
    for r in refs:
        for i in range(num_ec):
            r[3 + i][:16, :32] = 0.0
    _set_refs(ctx, refs)
    grid = _mode_grid(num_ec)
    patches, blendings = [], []
    for j, bl in enumerate(grid * 3):
        xs, ys = int(rng.integers(4, 60)), int(rng.integers(4, 50))
        patches.append((int(rng.integers(0, w - xs + 1)), int(rng.integers(0, h - ys + 1)), j & 1,
                        int(rng.integers(0, 96 - xs + 1)), int(rng.integers(0, 64 - ys + 1)), xs, ys))
        blendings += bl
    # the colour BlendAbove overwrites the alpha channel with its own new_a: a clamp that differs from the alpha
    # channel's own blending shows whether that happens
    if num_ec and any(f & ALPHA for f in flags):
        a = 0 if flags[0] & ALPHA else 1
        for _ in range(8):
            patches.append((0, 0, 0, 0, 16, 80, 40))
            bl = [(pr.BLEND_ABOVE, a, True)] + [(pr.BLEND_ABOVE, a, False)] * num_ec
            blendings += bl
    base = _planes(rng, 3 + num_ec, h, w)
    for i in range(num_ec):
        base[3 + i][:20, :40] = 0.0
    ctx.set_patches(patches, blendings, flags)
    got = ctx.stage_patches(base)
    want = pr.apply_patches([p.copy() for p in base], patches, blendings, refs, flags)
    _assert_planes(got, want, "stage hook")
    assert any(not np.array_equal(a, b) for a, b in zip(want, base))


@pytest.mark.parametrize("case", KAT["add_one_row_cases"], ids=[c["name"] for c in KAT["add_one_row_cases"]])
def test_stage_hook_add_one_row_kat(ctx, case):
    """the reference's add_one_row tests through the device kernel: within their tolerance of the values they
    expect, and bit for bit the restatement"""
    frame, refs, patches, blendings = kat_row_planes(case)
    h, w = frame[0].shape
    _begin(ctx, w, h)
    for s in range(4):
        ctx.clear_reference(s)
    for s, planes in refs.items():
        ctx.set_reference(s, planes)
    ctx.set_patches(patches, blendings, case["ec_flags"])
    got = ctx.stage_patches(frame)
    for c, want in enumerate(case["expected"]):
        assert np.max(np.abs(got[c] - np.array(want, np.float32))) <= KAT["add_one_row_max_abs_delta"], (c, got[c], want)
    _assert_planes(got, pr.apply_patches([p.copy() for p in frame], patches, blendings, refs, case["ec_flags"]), "kat")


def test_overlap_order(ctx):
    rng = np.random.default_rng(2000)
    w, h, num_ec, flags = 1031, 777, 1, [ALPHA]
    _begin(ctx, w, h)
    refs = [_planes(rng, 3 + num_ec, 128, 160) for _ in range(3)]
    _set_refs(ctx, refs)
    patches, blendings = [], []
    for _ in range(2000):
        xs, ys = int(rng.integers(1, 120)), int(rng.integers(1, 100))
        patches.append((int(rng.integers(0, w + 1 - xs + 1)), int(rng.integers(0, h + 7 - ys + 1)), int(rng.integers(0, 3)),
                        int(rng.integers(0, 160 - xs + 1)), int(rng.integers(0, 128 - ys + 1)), xs, ys))
        for _ in range(1 + num_ec):
            blendings.append((int(rng.integers(0, 8)), 0, bool(rng.integers(0, 2))))
    base = _planes(rng, 3 + num_ec, h, w)
    ctx.set_patches(patches, blendings, flags)
    got = ctx.stage_patches(base)
    want = pr.apply_patches([p.copy() for p in base], patches, blendings, refs, flags)
    _assert_planes(got, want, "2000 overlapping patches")
    pairs = [blendings[2 * i:2 * i + 2] for i in range(len(patches))][::-1]
    ctx.set_patches(patches[::-1], [b for p in pairs for b in p], flags)
    rev = ctx.stage_patches(base)
    assert any(not np.array_equal(a, b) for a, b in zip(rev, got)), "reversed order gave the same image"


# ---------------------------------------------------------------- whole frames
def _frame_dictionary(rng, w, h, num_ec, n, ref_w=512, ref_h=256, slots=(0, 1)):
    patches, blendings = [], []
    for _ in range(n):
        xs, ys = int(rng.integers(8, 64)), int(rng.integers(8, 48))
        patches.append((int(rng.integers(0, w - xs + 1)), int(rng.integers(0, h - ys + 1)), int(rng.choice(slots)),
                        int(rng.integers(0, ref_w - xs + 1)), int(rng.integers(0, ref_h - ys + 1)), xs, ys))
        for _ in range(1 + num_ec):
            blendings.append((int(rng.integers(0, 8)), int(rng.integers(0, max(num_ec, 1))), bool(rng.integers(0, 2))))
    return patches, blendings


def _ec_samples(rng, w, h, num_ec):
    return [rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32) for _ in range(num_ec)]


def _render(ctx, wl, patches, blendings, flags, ecs=(), **over):
    upload_frame(ctx, wl, **over)
    for i, s in enumerate(ecs):
        ctx.set_extra_channel(i, s, 16)
    if patches is not None:
        ctx.set_patches(patches, blendings, flags)
    ctx.frame_run()
    ctx.sync()


def _read_all(ctx, num_ec, w, h):
    return ctx.read_planes() + [ctx.read_extra_channel(i, w, h) for i in range(num_ec)]


@pytest.mark.parametrize("size,ecflags", [((1400, 1100), []), ((1400, 1100), [ALPHA, 0]), ((3840, 2160), [ALPHA | ASSOC])],
                         ids=["1.5mp", "1.5mp_2ec", "4k_1ec"])
def test_frame_matches_oracle_and_restatement(ctx, oracle, size, ecflags):
    from jxl_rs_amd import synth
    w, h = size
    num_ec = len(ecflags)
    rng = np.random.default_rng(w + num_ec)
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=w + 3, epf_iters=2)
    refs = [_planes(rng, 3 + num_ec, 256, 512) for _ in range(2)]
    _set_refs(ctx, refs)
    patches, blendings = _frame_dictionary(rng, w, h, num_ec, 1500)
    ecs = _ec_samples(rng, w, h, num_ec)
    # the extra channels' converted values, as the frame path makes them without patches
    _render(ctx, wl, None, None, ecflags, ecs)
    ec_base = [ctx.read_extra_channel(i, w, h) for i in range(num_ec)]
    _render(ctx, wl, patches, blendings, ecflags, ecs)
    got = _read_all(ctx, num_ec, w, h)
    col, _ = run_oracle_frame(oracle, wl)
    want = pr.apply_patches([np.ascontiguousarray(c) for c in col] + ec_base, patches, blendings, refs, ecflags)
    _assert_planes(got, want, "patched frame")
    # the output stage reads the patched planes
    import json
    import os
    k = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kat.json")))["output_stage"]
    xp = oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, 255.0)
    assert np.array_equal(ctx.read_rgb8(xp, 3), oracle.xyb_to_rgb8(xp, want[:3], w, h, 3))
    # idempotence: a second run over the same frame draws the patches once, on colour and extra channels
    ctx.frame_run()
    ctx.sync()
    _assert_planes(_read_all(ctx, num_ec, w, h), want, "second frame_run")


def test_frame_saved_reference_feeds_the_next_frame(ctx, oracle):
    from jxl_rs_amd import synth
    rng = np.random.default_rng(77)
    w, h = 900, 700
    wl1 = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=1, epf_iters=1)
    wl2 = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=2, epf_iters=2)
    refs = [_planes(rng, 4, 256, 512)]
    _set_refs(ctx, refs)
    ecs1 = _ec_samples(rng, w, h, 1)
    p1, b1 = _frame_dictionary(rng, w, h, 1, 300, slots=(0,))
    _render(ctx, wl1, None, None, [ALPHA], ecs1)
    ec1 = ctx.read_extra_channel(0, w, h)
    _render(ctx, wl1, p1, b1, [ALPHA], ecs1)
    ctx.save_reference(2)
    col1, _ = run_oracle_frame(oracle, wl1)
    frame1 = pr.apply_patches([np.ascontiguousarray(c) for c in col1] + [ec1], p1, b1, refs, [ALPHA])
    ecs2 = _ec_samples(rng, w, h, 1)
    _render(ctx, wl2, None, None, [ALPHA], ecs2)
    ec2 = ctx.read_extra_channel(0, w, h)
    p2, b2 = _frame_dictionary(rng, w, h, 1, 400, ref_w=w, ref_h=h, slots=(2,))
    _render(ctx, wl2, p2, b2, [ALPHA], ecs2)
    col2, _ = run_oracle_frame(oracle, wl2)
    all_refs = {0: refs[0], 2: frame1}
    want = pr.apply_patches([np.ascontiguousarray(c) for c in col2] + [ec2], p2, b2, all_refs, [ALPHA])
    _assert_planes(_read_all(ctx, 1, w, h), want, "frame patched from a saved reference")
    ctx.clear_reference(2)


def test_frame_upsampled_and_noise(ctx, oracle):
    from jxl_rs_amd import synth
    rng = np.random.default_rng(5)
    w, h = 520, 390
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=9, epf_iters=1)
    refs = [_planes(rng, 3, 256, 512)]
    _set_refs(ctx, refs)
    patches, blendings = _frame_dictionary(rng, w, h, 0, 400, slots=(0,))
    col, _ = run_oracle_frame(oracle, wl)
    patched = pr.apply_patches([np.ascontiguousarray(c) for c in col], patches, blendings, refs, [])
    # upsampling 2: the patches are drawn at the coded size, before Upsample2x (frame/render.rs:644-671)
    _render(ctx, wl, patches, blendings, [], upsampling=2)
    want = [oracle.upsample(2, np.ascontiguousarray(p)) for p in patched]
    _assert_planes(ctx.read_planes(), want, "upsampled patched frame")
    # noise: added after the patches
    lut = np.float32([0.02, 0.05, 0.1, 0.2, 0.15, 0.1, 0.05, 0.3])
    over = dict(noise=1, visible_frame_index=1)
    p = upload_frame(ctx, wl, **over)
    for i in range(8):
        p.noise_lut[i] = float(lut[i])
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.set_patches(patches, blendings, [])
    ctx.frame_run()
    ctx.sync()
    rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(1, 0, w, h)]
    want = oracle.noise_add(lut, 0.0, 1.0, [p.copy() for p in patched], rnd)
    _assert_planes(ctx.read_planes(), want, "patched frame with noise")


@pytest.mark.parametrize("epf_iters,gab", [(2, True), (0, False)], ids=["filtered", "unfiltered"])
def test_bands_and_rerender_equal_whole_frame(ctx, epf_iters, gab):
    from jxl_rs_amd import synth
    rng = np.random.default_rng(31 + epf_iters)
    w, h = 1100, 1300
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=4, epf_iters=epf_iters, gab=gab)
    refs = [_planes(rng, 4, 256, 512)]
    _set_refs(ctx, refs)
    patches, blendings = _frame_dictionary(rng, w, h, 1, 800, slots=(0,))
    # patches that straddle every group-row edge
    for gy in range(1, (h + 255) // 256):
        for x in range(0, w - 60, 97):
            patches.append((x, gy * 256 - 13, 0, 7, 9, 60, 30))
            blendings += [(pr.ADD, 0, False), (pr.ADD, 0, False)]
    ecs = _ec_samples(rng, w, h, 1)
    _render(ctx, wl, patches, blendings, [ALPHA], ecs)
    whole = _read_all(ctx, 1, w, h)
    # group-row bands
    ygroups = (h + 255) // 256
    upload_frame(ctx, wl)
    ctx.set_extra_channel(0, ecs[0], 16)
    ctx.set_patches(patches, blendings, [ALPHA])
    for g0, g1 in ((0, 2), (2, 3), (3, ygroups)):
        ctx.frame_run(g0, g1)
    ctx.sync()
    _assert_planes(_read_all(ctx, 1, w, h), whole, "band runs")
    # re-render a few groups after a whole render
    ctx.frame_run()
    ctx.rerender_groups([0, 5, 9, len(wl.coeffs) - 1])
    ctx.sync()
    _assert_planes(_read_all(ctx, 1, w, h), whole, "rerender_groups")


def test_subsampled_unfiltered_band_runs_keep_patches(ctx, oracle):
    """a 4:2:0 frame without filters: the result lives in the planes the transforms write, and a band's halo group row
    would overwrite the neighbouring band's patches -- band runs render the whole frame instead"""
    from jxl_rs_amd import synth
    rng = np.random.default_rng(420)
    w, h = 700, 900
    hs = vs = (1, 0, 1)
    wl = synth.make_vardct(w, h, mix=synth.MIX_8X8, seed=17, epf_iters=0, gab=False, hshift=hs, vshift=vs)
    refs = [_planes(rng, 3, 256, 512)]
    _set_refs(ctx, refs)
    patches, blendings = _frame_dictionary(rng, w, h, 0, 500, slots=(0,))
    for gy in range(1, (h + 255) // 256):  # across every group-row edge
        for x in range(0, w - 60, 83):
            patches.append((x, gy * 256 - 20, 0, 5, 3, 60, 40))
            blendings.append((pr.ADD, 0, False))
    col, _ = run_oracle_frame(oracle, wl)
    want = pr.apply_patches([np.ascontiguousarray(c) for c in col], patches, blendings, refs, [])
    _render(ctx, wl, patches, blendings, [])
    _assert_planes(ctx.read_planes(), want, "4:2:0 whole frame")
    upload_frame(ctx, wl)
    ctx.set_patches(patches, blendings, [])
    for g0, g1 in ((0, 2), (2, 3), (3, 4)):
        ctx.frame_run(g0, g1)
    ctx.sync()
    _assert_planes(ctx.read_planes(), want, "4:2:0 band runs")


# ---------------------------------------------------------------- validation
def test_validation_and_clearing(ctx, oracle):
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(3)
    w, h = 300, 260  # padded: 304 x 264
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=42, epf_iters=2)
    for s in range(4):
        ctx.clear_reference(s)
    ctx.set_reference(0, _planes(rng, 4, 50, 60))
    ecs = _ec_samples(rng, w, h, 1)
    _render(ctx, wl, None, None, [ALPHA], ecs)
    plain = _read_all(ctx, 1, w, h)
    ok_p = (10, 10, 0, 0, 0, 20, 20)
    ok_b = [(pr.REPLACE, 0, False), (pr.REPLACE, 0, False)]
    bad = [
        ([(10, 10, 1, 0, 0, 20, 20)], ok_b, [ALPHA], None),          # slot not set
        ([(10, 10, 7, 0, 0, 20, 20)], ok_b, [ALPHA], None),          # slot out of range
        ([ok_p], ok_b * 1 + [(0, 0, 0)], [ALPHA, 0], None),          # num_ec != the frame's / the slot's
        ([ok_p], [ok_b[0]], [], None),                               # num_ec 0 against a 4-channel slot
        ([(10, 10, 0, 45, 0, 20, 20)], ok_b, [ALPHA], None),         # reference rectangle beyond the slot (x)
        ([(10, 10, 0, 0, 31, 20, 20)], ok_b, [ALPHA], None),         # ... (y)
        ([ok_p], [(8, 0, 0), ok_b[1]], [ALPHA], None),               # mode >= 8
        ([(285, 10, 0, 0, 0, 20, 20)], ok_b, [ALPHA], None),         # beyond the padded width (304)
        ([(10, 245, 0, 0, 0, 20, 20)], ok_b, [ALPHA], None),         # beyond the padded height (264)
    ]
    upload_frame(ctx, wl)
    ctx.set_extra_channel(0, ecs[0], 16)
    for patches, blendings, flags, nec in bad:
        st = ctx.try_set_patches(patches, blendings, flags, nec)
        assert st == lib.ERR_INVALID_ARGUMENT, (patches, blendings, flags, st)
    # with one extra channel the reference never reads alpha_channel (it stays 0): any value is accepted
    assert ctx.try_set_patches([ok_p], [(pr.BLEND_ABOVE, 5, 0), ok_b[1]], [ALPHA]) == lib.OK
    # alpha channel out of range, with two extra channels
    ctx.set_reference(1, _planes(rng, 5, 50, 60))
    two = [(10, 10, 1, 0, 0, 20, 20)]
    upload_frame(ctx, wl)
    assert ctx.try_set_patches(two, [(pr.BLEND_ABOVE, 2, 0), (0, 0, 0), (0, 0, 0)], [ALPHA, 0]) == lib.ERR_INVALID_ARGUMENT
    assert ctx.try_set_patches(two, [(pr.BLEND_ABOVE, 1, 0), (0, 0, 0), (0, 0, 0)], [ALPHA, 0]) == lib.OK
    # inside the padded size is accepted (the reference's bound), drawing is clipped at the frame's edge
    upload_frame(ctx, wl)
    ctx.set_extra_channel(0, ecs[0], 16)
    assert ctx.try_set_patches([(284, 244, 0, 0, 0, 20, 20)], ok_b, [ALPHA]) == lib.OK
    # the rejected calls left the frame as it was; n = 0 clears the dictionary: the no-patch frame bit for bit
    ctx.set_patches([], [], [ALPHA])
    ctx.frame_run()
    ctx.sync()
    _assert_planes(_read_all(ctx, 1, w, h), plain, "cleared dictionary")
    # a reference slot that changed under the dictionary: the run refuses before it launches anything
    ctx.set_patches([ok_p], ok_b, [ALPHA])
    ctx.clear_reference(0)
    with pytest.raises(lib.JxlHipError):
        ctx.frame_run()
    ctx.set_reference(0, _planes(rng, 4, 50, 60))
    # save_reference needs a rendered frame
    upload_frame(ctx, wl)
    with pytest.raises(lib.JxlHipError):
        ctx.save_reference(3)


def test_sharded_frame_with_patches_is_unsupported(ctx):
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(8)
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            c.set_reference(0, _planes(rng, 3, 40, 40))
            upload_frame(c, wl)
            c.set_patches([(5, 5, 0, 0, 0, 30, 30)], [(pr.ADD, 0, False)], [])
        with pytest.raises(lib.JxlHipError) as e:
            lib.frames_run_sharded_local(peers)
        assert e.value.status == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
