"""Frame blending on the device (k_blend.hip) held bit for bit to the numpy restatement of the reference
(blending_ref.py): through the stage hook, inside whole VarDCT frames with and without a colour stage in front, over a
four-frame animation that lives in the reference slots, plus the call's state rules and validation.

bit_equal compares bit patterns, so every test first asserts that the expected planes are finite."""
import json
import os

import numpy as np
import pytest

import blending_ref as br
import patches_ref as pr
from helpers import bit_equal, diff_report, run_oracle_frame, upload_frame
from test_gpu_patches import EC_SETS

pytestmark = pytest.mark.gpu

ALPHA, ASSOC = pr.EC_ALPHA, pr.EC_ALPHA_ASSOCIATED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def _planes(rng, n, h, w):
    return [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(n)]


def _zero_alpha_patch(planes, num_ec):
    """alpha pairs that make new_a == 0: zero alpha over part of the planes"""
    for i in range(num_ec):
        planes[3 + i][:16, :32] = 0.0


def _lib_desc(d, num_ec=None):
    from jxl_rs_amd import lib
    return lib.blend_desc(d.x0, d.y0, d.image_w, d.image_h, d.color, d.ec, d.ec_flags, num_ec)


def _set_slots(ctx, refs):
    """refs: dict slot -> planes; the other slots are cleared"""
    for s in range(4):
        ctx.clear_reference(s)
    for s, planes in refs.items():
        ctx.set_reference(s, planes)


def _assert_finite(planes):
    for c, p in enumerate(planes):
        assert np.isfinite(p).all(), f"expected channel {c} is not finite"


def _assert_planes(got, want, what):
    assert len(got) == len(want)
    for c, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape, (what, c, g.shape, e.shape)
        assert bit_equal(g, e), f"{what}: channel {c}: {diff_report(g, e)}"


def _read_all(ctx, num_ec):
    w, h = ctx.out_size
    return ctx.read_planes() + [ctx.read_extra_channel(i, w, h) for i in range(num_ec)]


# origins of a fw x fh frame in an iw x ih image: negative, inside, straddling each edge, wholly outside on every side
def _origins(iw, ih, fw, fh):
    return [(0, 0), (17, 9), (-13, -9), (-13, 20), (21, -9), (iw - fw + 30, 11), (30, ih - fh + 25), (iw - 7, ih - 5),
            (-fw - 3, 10), (iw, 10), (10, -fh), (10, ih + 2), (-fw, -fh), (iw + 3, ih + 3), (iw - 1, ih - 1),
            (1 - fw, 1 - fh)]


# ---------------------------------------------------------------- stage hook
def _mode_grid(num_ec):
    """every colour mode x clamp x alpha channel; extra-channel blendings cycle through every mode; colour and extra
    channels read different slots, slot 3 is never set"""
    out = []
    k = 0
    for mode in range(5):
        for clamp in (False, True):
            for alpha in range(max(1, min(num_ec, 2))):
                color = (mode, alpha, clamp, k % 4)
                ec = [((mode + 2 * i + k + 1) % 5, (alpha + i + k) % max(num_ec, 1), bool((k + i) & 1), (k + i + 1) % 4)
                      for i in range(num_ec)]
                out.append((color, ec))
                k += 1
    return out


@pytest.mark.parametrize("flags", EC_SETS, ids=["ec%d_%s" % (len(f), "_".join(map(str, f))) for f in EC_SETS])
def test_stage_hook_every_mode(ctx, flags):
    num_ec = len(flags)
    rng = np.random.default_rng(101 + 7 * num_ec + sum(flags))
    iw, ih, fw, fh = 301, 157, 123, 77  # no multiple of 4 or 64 anywhere
    refs = {s: _planes(rng, 3 + num_ec, ih + s, iw + 3 * s) for s in range(3)}  # slots at least image-sized
    for r in refs.values():
        _zero_alpha_patch(r, num_ec)
    _set_slots(ctx, refs)
    origins = _origins(iw, ih, fw, fh)
    changed = 0
    for k, (color, ec) in enumerate(_mode_grid(num_ec)):
        x0, y0 = origins[k % len(origins)]
        frame = _planes(rng, 3 + num_ec, fh, fw)
        _zero_alpha_patch(frame, num_ec)
        d = br.BlendDesc(x0, y0, iw, ih, color, ec, flags)
        want = br.blend_frame(frame, refs, d)
        _assert_finite(want)
        got = ctx.stage_blend(_lib_desc(d), frame)
        _assert_planes(got, want, f"stage hook {color} {ec} at {(x0, y0)}")
        changed += any(not np.array_equal(a, b) for a, b in zip(want, br.source_planes(refs, d)))
    assert changed > 4  # the frames did land on the image


def test_stage_hook_origin_grid(ctx):
    rng = np.random.default_rng(7)
    flags = [ALPHA]
    for iw, ih, fw, fh in ((257, 66, 70, 31), (64, 9, 130, 23), (1030, 5, 515, 3)):
        refs = {0: _planes(rng, 4, ih, iw), 2: _planes(rng, 4, ih + 1, iw + 70)}
        _set_slots(ctx, refs)
        for j, (x0, y0) in enumerate(_origins(iw, ih, fw, fh)):
            frame = _planes(rng, 4, fh, fw)
            d = br.BlendDesc(x0, y0, iw, ih, (br.BLEND, 0, bool(j & 1), 0), [(br.BLEND, 0, bool(j & 2), 2)], flags)
            want = br.blend_frame(frame, refs, d)
            _assert_finite(want)
            _assert_planes(ctx.stage_blend(_lib_desc(d), frame), want, f"{iw}x{ih} frame {fw}x{fh} at {(x0, y0)}")


def test_stage_hook_eight_extra_channels(ctx):
    rng = np.random.default_rng(88)
    num_ec = 8
    flags = [0, ALPHA, 0, ALPHA | ASSOC, 0, 0, ALPHA, 0]
    iw, ih, fw, fh = 203, 61, 150, 40
    refs = {1: _planes(rng, 11, ih, iw), 3: _planes(rng, 11, ih, iw + 1)}
    _set_slots(ctx, refs)
    for k, (x0, y0) in enumerate(((-20, -7), (40, 11), (100, 30))):
        color = ((br.BLEND, br.ALPHA_WEIGHTED_ADD, br.MUL)[k], (1, 3, 6)[k], bool(k & 1), (1, 3, 0)[k])
        ec = [((i + k) % 5, (i * 3 + k) % num_ec, bool((i + k) & 1), (i + k) % 4) for i in range(num_ec)]
        frame = _planes(rng, 11, fh, fw)
        d = br.BlendDesc(x0, y0, iw, ih, color, ec, flags)
        want = br.blend_frame(frame, refs, d)
        _assert_finite(want)
        _assert_planes(ctx.stage_blend(_lib_desc(d), frame), want, f"8 extra channels, case {k}")


def test_stage_hook_full_size(ctx):
    """an 8192 x 8192 image, a 4096 x 4096 cropped frame with one alpha channel"""
    rng = np.random.default_rng(8192)
    iw = ih = 8192
    fw = fh = 4096

    def big(h, w):
        a = rng.random((h, w), dtype=np.float32)
        a *= np.float32(2.0)
        a -= np.float32(0.5)
        return a
    refs = {0: [big(ih, iw) for _ in range(4)]}
    _set_slots(ctx, refs)
    frame = [big(fh, fw) for _ in range(4)]
    d = br.BlendDesc(1111, 2049, iw, ih, (br.BLEND, 0, True, 0), [(br.BLEND, 0, True, 0)], [ALPHA])
    want = br.blend_frame(frame, refs, d)
    _assert_finite(want)
    got = ctx.stage_blend(_lib_desc(d), frame)
    for c in range(4):
        assert bit_equal(got[c], want[c]), f"channel {c}"
    ctx.clear_reference(0)


# ---------------------------------------------------------------- whole frames
def _ec_samples(rng, w, h, num_ec):
    return [rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32) for _ in range(num_ec)]


def _render(ctx, wl, ecs=(), patches=None, **over):
    upload_frame(ctx, wl, **over)
    for i, s in enumerate(ecs):
        ctx.set_extra_channel(i, s, 16)
    if patches is not None:
        ctx.set_patches(*patches)
    ctx.frame_run()


IMAGE = (1280, 1024)
FRAME_ORIGINS = [(-40, 100), (900, 700), (0, 0)]


@pytest.mark.parametrize("origin", FRAME_ORIGINS, ids=["x%d_y%d" % o for o in FRAME_ORIGINS])
def test_frame_color_none(ctx, oracle, origin):
    from jxl_rs_amd import synth
    rng = np.random.default_rng(512 + origin[0])
    w, h = 512, 384
    iw, ih = IMAGE
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=21, epf_iters=2)
    col, _ = run_oracle_frame(oracle, wl)
    refs = {1: _planes(rng, 3, ih, iw)}
    _set_slots(ctx, refs)
    for mode, clamp in ((br.ADD, False), (br.MUL, True), (br.REPLACE, False), (br.BLEND, False)):
        d = br.BlendDesc(origin[0], origin[1], iw, ih, (mode, 0, clamp, 1), [], [])
        want = br.blend_frame(col, refs, d)
        _assert_finite(want)
        _render(ctx, wl)
        ctx.blend(_lib_desc(d))
        assert ctx.out_size == (iw, ih)
        _assert_planes(_read_all(ctx, 0), want, f"frame at {origin}, mode {mode}")
        # a rect of the composed planes, and the device pointers' stride
        rect = ctx.read_planes_rect(100, 50, 300, 200)
        _assert_planes(rect, [p[50:250, 100:400] for p in want], "read_planes_rect of the composed image")
        assert ctx.device_planes()[1] == (iw + 63) // 64 * 64


def test_frame_with_alpha_channel_and_patches(ctx, oracle):
    """the patched copy of the frame -- colour and extra channel -- is what gets blended"""
    from jxl_rs_amd import synth
    from test_gpu_patches import _frame_dictionary
    rng = np.random.default_rng(99)
    w, h = 512, 384
    iw, ih = IMAGE
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=22, epf_iters=1)
    col, _ = run_oracle_frame(oracle, wl)
    refs = {0: _planes(rng, 4, ih, iw), 1: _planes(rng, 4, ih, iw)}
    _zero_alpha_patch(refs[0], 1)
    _set_slots(ctx, refs)
    ecs = _ec_samples(rng, w, h, 1)
    ecs[0][:16, :32] = 0
    _render(ctx, wl, ecs)
    ec_base = [ctx.read_extra_channel(0, w, h)]
    patches, blendings = _frame_dictionary(rng, w, h, 1, 300, ref_w=iw, ref_h=ih, slots=(0, 1))
    frame = pr.apply_patches([np.ascontiguousarray(c) for c in col] + [e.copy() for e in ec_base], patches, blendings, refs,
                             [ALPHA])
    assert any(not np.array_equal(a, b) for a, b in zip(frame[3:], ec_base))
    for origin in FRAME_ORIGINS:
        d = br.BlendDesc(origin[0], origin[1], iw, ih, (br.BLEND, 0, True, 0), [(br.BLEND, 0, False, 1)], [ALPHA])
        want = br.blend_frame(frame, refs, d)
        _assert_finite(want)
        _render(ctx, wl, ecs, (patches, blendings, [ALPHA]))
        ctx.blend(_lib_desc(d))
        _assert_planes(_read_all(ctx, 1), want, f"patched frame with alpha at {origin}")


def test_frame_upsampled(ctx, oracle):
    from jxl_rs_amd import synth
    rng = np.random.default_rng(4)
    w, h = 256, 192
    iw, ih = IMAGE
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=23, epf_iters=1)
    col, _ = run_oracle_frame(oracle, wl)
    frame = [oracle.upsample(2, np.ascontiguousarray(p)) for p in col]
    assert frame[0].shape == (384, 512)
    refs = {2: _planes(rng, 3, ih, iw)}
    _set_slots(ctx, refs)
    for origin in FRAME_ORIGINS:
        d = br.BlendDesc(origin[0], origin[1], iw, ih, (br.ADD, 0, False, 2), [], [])
        want = br.blend_frame(frame, refs, d)
        _assert_finite(want)
        _render(ctx, wl, upsampling=2)
        ctx.blend(_lib_desc(d))
        _assert_planes(_read_all(ctx, 0), want, f"upsampled frame at {origin}")


# ---------------------------------------------------------------- the colour stage in front
def _xyb_params(oracle, intensity_target=255.0):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["output_stage"]
    return oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, intensity_target)


LUM = (0.2627, 0.678, 0.0593)


def _oracle_colour(oracle, col, color, tf, param):
    h, w = col[0].shape
    if color == "ycbcr":
        rgb = oracle.ycbcr_to_rgb(*col)
    else:
        params = _xyb_params(oracle, 255.0 if tf != "pq" else param)
        rgb = oracle.xyb_to_linear(params, *col)
        if tf != "linear":
            rgb = oracle.from_linear(tf, rgb, param, LUM)
    return [np.asarray(p, np.float32).reshape(h, w) for p in rgb]


@pytest.mark.parametrize("color,tf,param", [("xyb", "linear", 0.0), ("xyb", "srgb", 0.0), ("xyb", "pq", 10000.0),
                                            ("ycbcr", "linear", 0.0)], ids=["xyb_linear", "xyb_srgb", "xyb_pq", "ycbcr"])
def test_frame_colour_stage_in_front(ctx, oracle, color, tf, param):
    """the colour stage runs on the frame's samples in f32 before the blend: expected = blend_frame of the oracle's
    colour stage.  First the stage alone (Replace, full frame, no slot), then blended."""
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(31)
    w, h = 512, 384
    iw, ih = IMAGE
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=24, epf_iters=2)
    col, _ = run_oracle_frame(oracle, wl)
    rgb = _oracle_colour(oracle, col, color, tf, param)
    _assert_finite(rgb)
    if color == "ycbcr":
        colour = ctx.output_desc(lib.COLOR_YCBCR, "linear", None, 0.0, LUM)
    else:
        colour = ctx.output_desc(lib.COLOR_XYB, tf, _xyb_params(oracle, 255.0 if tf != "pq" else param), param, LUM)
    _set_slots(ctx, {})
    _render(ctx, wl)
    alone = br.BlendDesc(0, 0, w, h, (br.REPLACE, 0, False, 0), [], [])
    ctx.blend(_lib_desc(alone), colour)
    _assert_planes(_read_all(ctx, 0), rgb, f"colour stage alone ({color} {tf})")
    refs = {0: _planes(rng, 3, ih, iw)}
    _set_slots(ctx, refs)
    for origin, mode in zip(FRAME_ORIGINS, (br.ADD, br.MUL, br.ADD)):
        d = br.BlendDesc(origin[0], origin[1], iw, ih, (mode, 0, True, 0), [], [])
        want = br.blend_frame(rgb, refs, d)
        _assert_finite(want)
        _render(ctx, wl)
        ctx.blend(_lib_desc(d), colour)
        _assert_planes(_read_all(ctx, 0), want, f"{color} {tf} in front of the blend at {origin}")


# ---------------------------------------------------------------- an animation that lives in the slots
def _u8(oracle, planes):
    h, w = planes[0].shape
    out = np.zeros((h, w, 3), np.uint8)
    for c in range(3):
        for y in range(h):
            for x in range(w):
                out[y, x, c] = oracle.f32_to_u8(float(planes[c][y, x]), x, y, c)
    return out


def _u16(planes):
    return np.stack([np.rint(np.clip(p, 0, 1) * np.float32(65535)).astype(np.uint16) for p in planes[:3]], axis=-1)


def _slot_contents(ctx, slot, nch, iw, ih):
    """a slot read back without patches: a frame wholly outside the image leaves the extend stage's copy of the slot"""
    from jxl_rs_amd import lib
    d = lib.blend_desc(iw, ih, iw, ih, (lib.BLEND_REPLACE, 0, 0, slot), [(lib.BLEND_REPLACE, 0, 0, slot)] * (nch - 3),
                       [0] * (nch - 3))
    return ctx.stage_blend(d, [np.zeros((1, 1), np.float32)] * nch)


def test_animation_of_four_frames(ctx, oracle):
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(2024)
    iw, ih = 200, 120
    flags = [ALPHA]
    sizes = [(iw, ih), (120, 72), (96, 80), (150, 90)]
    wls = [synth.make_vardct(w, h, mix=synth.MIX_D1, seed=40 + i, epf_iters=1 + (i & 1)) for i, (w, h) in enumerate(sizes)]
    ecs = [_ec_samples(rng, w, h, 1) for w, h in sizes]
    descs = [
        br.BlendDesc(0, 0, iw, ih, (br.REPLACE, 0, False, 0), [(br.REPLACE, 0, False, 0)], flags),
        br.BlendDesc(50, 30, iw, ih, (br.BLEND, 0, True, 0), [(br.BLEND, 0, True, 0)], flags),
        br.BlendDesc(-20, 60, iw, ih, (br.ALPHA_WEIGHTED_ADD, 0, False, 0), [(br.ADD, 0, False, 1)], flags),
        br.BlendDesc(70, -10, iw, ih, (br.MUL, 0, True, 2), [(br.MUL, 0, True, 2)], flags),
    ]
    save_to = [0, 0, 2, None]
    # the frames as the oracle makes them; the extra channels' converted values from a render of their own
    frames = []
    for wl, ec, (w, h) in zip(wls, ecs, sizes):
        col, _ = run_oracle_frame(oracle, wl)
        _render(ctx, wl, ec)
        frames.append([np.ascontiguousarray(c) for c in col] + [ctx.read_extra_channel(0, w, h)])
    host_slot1 = _planes(rng, 4, ih, iw)
    _set_slots(ctx, {1: host_slot1})
    refs = {1: host_slot1}
    for i, (wl, ec, d) in enumerate(zip(wls, ecs, descs)):
        want = br.blend_frame(frames[i], refs, d)
        _assert_finite(want)
        # no host synchronisation between the render, the blend and the save
        _render(ctx, wl, ec)
        ctx.blend(_lib_desc(d))
        if save_to[i] is not None:
            ctx.save_reference(save_to[i])
            refs[save_to[i]] = want
        _assert_planes(_read_all(ctx, 1), want, f"canvas of frame {i}")
        if save_to[i] is not None:
            _assert_planes(_slot_contents(ctx, save_to[i], 4, iw, ih), want, f"slot {save_to[i]} after frame {i}")
    got8 = ctx.read_output(lib.COLOR_NONE, "linear", None, 0.0, LUM, 8, 3)
    got16 = ctx.read_output(lib.COLOR_NONE, "linear", None, 0.0, LUM, 16, 3)
    assert np.array_equal(got16, _u16(want))
    assert np.array_equal(got8, _u8(oracle, want))
    assert len(np.unique(got8)) > 16


# ---------------------------------------------------------------- state and validation
def test_state_rules(ctx, oracle):
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(6)
    w, h = 300, 260
    iw, ih = 400, 300
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=42, epf_iters=2)
    col, _ = run_oracle_frame(oracle, wl)
    refs = {0: _planes(rng, 3, ih, iw)}
    _set_slots(ctx, refs)
    d = br.BlendDesc(-30, 20, iw, ih, (br.ADD, 0, False, 0), [], [])
    want = br.blend_frame(col, refs, d)
    _assert_finite(want)
    # before a render
    upload_frame(ctx, wl)
    assert ctx.try_blend(_lib_desc(d)) == lib.ERR_BAD_STATE
    ctx.frame_run()
    ctx.blend(_lib_desc(d))
    _assert_planes(_read_all(ctx, 0), want, "first blend")
    # twice: the same canvas (an Add would show a second application)
    ctx.blend(_lib_desc(d))
    _assert_planes(_read_all(ctx, 0), want, "second blend")
    # another image size in the same frame, and back
    d2 = br.BlendDesc(10, 10, 640, 333, (br.MUL, 0, True, 3), [], [])
    ctx.blend(_lib_desc(d2))
    _assert_planes(_read_all(ctx, 0), br.blend_frame(col, refs, d2), "larger image, unset slot")
    ctx.blend(_lib_desc(d))
    _assert_planes(_read_all(ctx, 0), want, "back to the first image")
    # the colour stage has run: only COLOR_NONE read-outs
    with pytest.raises(lib.JxlHipError) as e:
        ctx.read_output(lib.COLOR_XYB, "srgb", np.zeros(16, np.float32), 0.0, LUM, 8, 3)
    assert e.value.status == lib.ERR_BAD_STATE
    with pytest.raises(lib.JxlHipError) as e:
        ctx.read_ycbcr_rgb8(3)
    assert e.value.status == lib.ERR_BAD_STATE
    assert np.array_equal(ctx.read_output(lib.COLOR_NONE, "linear", None, 0.0, LUM, 16, 3), _u16(want))
    # a render discards the composition
    ctx.frame_run()
    ctx.sync()
    assert ctx.out_size == (w, h)
    _assert_planes(ctx.read_planes(), col, "frame_run after a blend")
    ctx.blend(_lib_desc(d))
    ctx.rerender_groups([0])
    ctx.sync()
    _assert_planes(ctx.read_planes(), col, "rerender_groups after a blend")


def test_validation_leaves_the_canvas(ctx, oracle):
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(16)
    w, h = 300, 260
    iw, ih = 400, 300
    wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=43, epf_iters=1)
    col, _ = run_oracle_frame(oracle, wl)
    refs = {0: _planes(rng, 5, ih, iw), 1: _planes(rng, 5, ih - 1, iw), 2: _planes(rng, 4, ih, iw)}
    _set_slots(ctx, refs)
    ecs = _ec_samples(rng, w, h, 2)
    _render(ctx, wl, ecs)
    ec_base = [ctx.read_extra_channel(i, w, h) for i in range(2)]
    flags = [ALPHA, 0]

    def ok(s=0):
        return (br.ADD, 0, False, s)
    good = br.BlendDesc(20, 10, iw, ih, ok(), [ok(), ok(3)], flags)
    want = br.blend_frame([np.ascontiguousarray(c) for c in col] + ec_base, refs, good)
    _assert_finite(want)
    ctx.blend(_lib_desc(good))
    bad = [
        (br.BlendDesc(20, 10, iw, ih, (5, 0, False, 0), [ok(), ok()], flags), None),             # mode > 4
        (br.BlendDesc(20, 10, iw, ih, ok(), [(7, 0, False, 0), ok()], flags), None),             # ... of an extra channel
        (br.BlendDesc(20, 10, iw, ih, ok(4), [ok(), ok()], flags), None),                        # source >= 4
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok(), ok(9)], flags), None),
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok(), ok()], flags), 9),                            # num_ec > 8
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok()], flags[:1]), None),                           # num_ec != handed over
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok(), ok(), ok()], flags + [0]), None),
        (br.BlendDesc(20, 10, iw, ih, (br.BLEND, 2, False, 0), [ok(), ok()], flags), None),      # alpha_channel >= num_ec
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok(), (br.ALPHA_WEIGHTED_ADD, 5, False, 0)], flags), None),
        (br.BlendDesc(20, 10, 0, ih, ok(), [ok(), ok()], flags), None),                          # empty image
        (br.BlendDesc(20, 10, iw, 0, ok(), [ok(), ok()], flags), None),
        (br.BlendDesc(20, 10, 1 << 16, 1 << 15, ok(), [ok(), ok()], flags), None),               # 2^31 pixels
        (br.BlendDesc(20, 10, iw, ih, ok(1), [ok(), ok()], flags), None),                        # slot smaller than the image
        (br.BlendDesc(20, 10, iw, ih, ok(), [ok(2), ok()], flags), None),                        # slot with other channels
    ]
    for d, nec in bad:
        st = ctx.try_blend(_lib_desc(d, nec))
        assert st == lib.ERR_INVALID_ARGUMENT, (d, nec, st)
        if d.image_w * d.image_h < 1 << 24:  # the stage hook makes the same checks (num_ec against n_channels)
            assert ctx.try_stage_blend(_lib_desc(d, nec), list(col) + ec_base)[0] == lib.ERR_INVALID_ARGUMENT, (d, nec)
    # for a mode that does not read it, alpha_channel is ignored
    assert ctx.try_blend(_lib_desc(br.BlendDesc(20, 10, iw, ih, (br.ADD, 77, False, 0), [ok(), ok(3)], flags))) == lib.OK
    # the stage hook's own: n_channels != 3 + num_ec
    assert ctx.try_stage_blend(_lib_desc(good), col)[0] == lib.ERR_INVALID_ARGUMENT
    # every rejected call left the composition as it was
    _assert_planes(_read_all(ctx, 2), want, "canvas after the rejected calls")


def test_sharded_context_is_unsupported(ctx):
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        d = lib.blend_desc(0, 0, 300, 600, (lib.BLEND_REPLACE, 0, 0, 0))
        for c in peers:
            upload_frame(c, wl)
            assert c.try_blend(d) == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()
