"""The rectangle-list save on the device (jxlh_stage_save_rects / jxlh_frame_save_rects[_async], the rect forms of
k_save.hip) against tests/save_ref.py: the pixels of the rects are bit-equal to the same pixels of the whole save and
EVERY other byte of a poisoned buffer -- other pixels, row padding, the bytes around the image -- is untouched, for
every format, layout and orientation, host and device destinations at a pitch and origin that are not dword-aligned;
the whole-image rect equals jxlh_frame_save; a repaint of jxlh_changed_rects' rects after jxlh_frame_rerender_groups
equals a fresh full save and the oracle's; and every argument / state error writes nothing."""
import copy
import ctypes as C

import numpy as np
import pytest

import save_ref as sr
from helpers import gpu_params_from, run_oracle_frame, upload_frame
from test_gpu_save import FORMATS, LUM, PIXELS, POISON, layouts, lib_desc, poisoned, sample_bytes, xyb_params

pytestmark = pytest.mark.gpu

SIZES = [(70, 130), (1030, 9)]  # (w, h): tile edges on both axes; the 256- and 1024-pixel column blocks of a row


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planes():
    """per size: 3 colour + 3 extra channels, values in -0.5 .. 1.5"""
    rng = np.random.default_rng(2027)
    return {(w, h): [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(6)] for w, h in SIZES}


def rect_lists(w, h, pixel_bytes):
    """name -> rects (x0, y0, w, h) of a w x h source"""
    from jxl_rs_amd import lib
    cols, rows = lib.save_tile_layout(pixel_bytes)
    ty = max(0, min(h, rows) - 3)
    crossing = [(cols - 2, ty, 5, 6), (250, 0, 12, 5) if w > 262 else (cols - 1, 0, 2, 1)]
    if w > 1024:
        crossing.append((1019, 1, 10, 7))
    if h > 2 * rows:
        crossing.append((5, 2 * rows - 1, cols + 3, 2))
    return {
        "single pixel": [(w // 2, h // 2, 1, 1)],
        "odd x0, odd width": [(3, 1, 7, 3), (w + 5, 0, 0, 3)],  # (and an empty rect, skipped wherever it starts)
        "across the blocks and tiles": crossing,
        "two overlapping": [(2, 3, 20, 4), (10, 5, 30, 3)],
        "whole image": [(0, 0, w, h)],
        "cut right and bottom": [(w - 5, h - 4, 100, 100)],
    }


def combined(w, h, pixel_bytes):
    """every kind of rect but the whole image, in one list"""
    return [r for name, rs in rect_lists(w, h, pixel_bytes).items() if name != "whole image" for r in rs]


def expected_buffer(d, w, h, rects, want, lead, bpr, row, oh, size):
    """the poisoned buffer with the pixels of the rects' union (clipped) taken from the whole save `want`"""
    mask = np.zeros((h, w, 1), dtype=bool)
    for x0, y0, rw, rh in rects:
        mask[y0:y0 + rh, x0:x0 + rw] = True
    pb = row // sr.oriented_size(d["orientation"], w, h)[0]
    bytemask = np.repeat(sr.orient(mask, d["orientation"])[:, :, 0], pb, axis=1)
    exp = np.full(size, POISON, dtype=np.uint8)
    body = exp[lead:lead + oh * bpr].reshape(oh, bpr)
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(oh, row)
    body[:, :row][bytemask] = wb[bytemask]
    return exp


def assert_buffer(buf, exp, lead, bpr, row, what):
    if np.array_equal(buf, exp):
        return
    bad = np.flatnonzero(buf != exp)
    i = int(bad[0])
    where = "around the image" if i < lead or i >= len(buf) - lead else \
        f"row {(i - lead) // bpr} byte {(i - lead) % bpr}" + (" (row padding)" if (i - lead) % bpr >= row else "")
    kind = "a byte that must stay untouched was written" if exp[i] == POISON else \
        ("a pixel of the rects was not written" if buf[i] == POISON else "a wrong sample")
    raise AssertionError(f"{what}: {len(bad)} bytes differ, first {where}: got {buf[i]} want {exp[i]} ({kind})")


def run_rects(ctx, d, pl, rects, want, what, colour=None, origin=(0, 0), pad=0, lead=16, device=False):
    from jxl_rs_amd import lib
    h, w = pl[0].shape
    buf, view, bpr, row, oh = poisoned(d, w, h, pad * sample_bytes(d), lead)
    exp = expected_buffer(d, w, h, rects, want, lead, bpr, row, oh, buf.size)
    dev = lib.DeviceArray(buf) if device else None
    st, _ = ctx.try_stage_save_rects(lib_desc(d), pl, rects, colour, origin, out=dev.ptr + lead if device else view,
                                     bytes_per_row=bpr)
    if device:
        buf = dev.download(np.uint8, buf.size)
        dev.free()
    assert st == 0, (what, st)
    assert_buffer(buf, exp, lead, bpr, row, what)


def whole_save(samples, d):
    s = sr.byte_order(sr.orient(samples, d["orientation"]), d["big_endian"])
    return s.reshape(s.shape[0], -1)


# ---------------------------------------------------------------- jxlh_stage_save_rects
@pytest.mark.parametrize("name,fmt", FORMATS, ids=[f[0] for f in FORMATS])
def test_formats_and_layouts(ctx, oracle, planes, name, fmt):
    """every format x layout, each under a row-form and a tile-form orientation, every kind of rect in one list"""
    fi = [f[0] for f in FORMATS].index(name)
    for i, (lname, channels, fill) in enumerate(layouts()):
        for si, (w, h) in enumerate(SIZES):
            pl = planes[(w, h)]
            samples = sr.save_samples(oracle, sr.desc(channels, fill_opaque_alpha=fill, **fmt), pl)
            for o in (1 + (i + fi + si) % 4, 5 + (i + fi + si) % 4):
                d = sr.desc(channels, fill_opaque_alpha=fill, orientation=o, **fmt)
                bps = sample_bytes(d)
                rects = combined(w, h, samples.shape[2] * bps)
                # pitches: tight, padded and dword-aligned, and (below 4-byte samples) no multiple of four
                pad = (0, 4 // bps * 3, 1 if bps < 4 else 2)[(i + o) % 3]
                run_rects(ctx, d, pl, rects, whole_save(samples, d), f"{name} {lname} {w}x{h} o{o} pad {pad}", pad=pad,
                          lead=(16, 16 + bps)[(i + si) % 2], device=(i + o + si) % 2 == 1)


@pytest.mark.parametrize("pname,px", PIXELS, ids=[p[0] for p in PIXELS])
def test_orientations_and_rect_lists(ctx, oracle, planes, pname, px):
    """orientations 1..8 x every rect list on its own x both sizes, for pixels of 1, 3, 4, 8 and 16 bytes"""
    bps = sr.SAMPLE_DTYPE[px["format"]]().itemsize
    n = 0
    for w, h in SIZES:
        pl = planes[(w, h)]
        samples = sr.save_samples(oracle, sr.desc(**px), pl)
        for lname, rects in rect_lists(w, h, samples.shape[2] * bps).items():
            for o in range(1, 9):
                n += 1
                d = sr.desc(orientation=o, **px)
                pad = (0, 4 // bps * 3, 1 if bps < 4 else 2)[n % 3]
                run_rects(ctx, d, pl, rects, whole_save(samples, d), f"{pname} {w}x{h} o{o} {lname} pad {pad}", pad=pad,
                          lead=(16, 16 + bps)[(n // 3) % 2], device=(n // 2) % 2 == 0)


def test_dither_phase_is_the_absolute_position(ctx, oracle, planes):
    """U8 at a non-zero frame origin: a rect's samples carry the dither of (frame_x0 + x, frame_y0 + y), not of the rect"""
    w, h = SIZES[0]
    pl = planes[(w, h)]
    for o in (1, 3, 6):
        d = sr.desc([0, 1, 2, 5], sr.U8, orientation=o)
        want = sr.save(oracle, d, pl, origin=(37, 21))
        assert not np.array_equal(want, sr.save(oracle, d, pl))
        for device in (False, True):
            run_rects(ctx, d, pl, combined(w, h, 4), want, f"dither o{o}", origin=(37, 21), pad=1, lead=17, device=device)


def test_spot_premultiply_and_colour_stage(ctx, oracle):
    from jxl_rs_amd import lib
    w, h = SIZES[0]
    rng = np.random.default_rng(91)
    pl = [rng.uniform(-0.015, 0.015, (h, w)), rng.uniform(0.0, 0.8, (h, w)), rng.uniform(0.0, 0.8, (h, w))]
    pl = [p.astype(np.float32) for p in pl] + [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(3)]
    spots = [(0, (0.9, 0.1, 0.3, 0.7)), (2, (0.2, 0.8, 0.5, 1.6))]
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    ref_colour = ("xyb", "srgb", xyb_params(oracle), 0.0, LUM)
    for o, fmt, depth in ((2, sr.U8, 8), (7, sr.U16, 10), (5, sr.F16, None)):
        d = sr.desc([2, 1, 0, 4], fmt, depth, premultiply=4, spot=spots, orientation=o)
        want = sr.save(oracle, d, pl, ref_colour)
        for device in (False, True):
            run_rects(ctx, d, pl, combined(w, h, 4 * sample_bytes(d)), want, f"stages o{o}", colour=colour, pad=3,
                      device=device)


# ---------------------------------------------------------------- jxlh_frame_save_rects on frames
@pytest.fixture(scope="module")
def frame():
    from jxl_rs_amd import synth
    return synth.make_vardct(300, 260, mix=synth.MIX_D1, seed=42, epf_iters=2)


def test_whole_image_rect_equals_frame_save(ctx, oracle, frame):
    """a frame with an alpha extra channel: the whole-image rect, and bands of rects, are jxlh_frame_save's bytes"""
    from jxl_rs_amd import lib
    rng = np.random.default_rng(77)
    w, h = frame.xsize, frame.ysize
    upload_frame(ctx, frame)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.frame_run()
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    xs, ys = [0, 1, 63, 64, 130, 257, w], [0, 31, 64, 65, 200, h]
    for d in (sr.desc([0, 1, 2, 3], sr.U8), sr.desc([0, 1, 2, 3], sr.U8, orientation=6),
              sr.desc([2, 1, 0], sr.F16, orientation=3), sr.desc([0, 3], sr.U16, 12, big_endian=True, orientation=8)):
        full = ctx.frame_save(lib_desc(d), colour)
        assert np.array_equal(ctx.frame_save_rects(lib_desc(d), [(0, 0, w, h)], colour), full), d
        assert np.array_equal(ctx.frame_save_rects(lib_desc(d), [(0, 0, 0xffffffff, 0xffffffff)], colour), full), d
        # bands: row bands in one call, column bands one call each, _async + one sync
        out = np.full_like(full, 0x5a)
        ctx.frame_save_rects(lib_desc(d), [(0, a, w, b - a) for a, b in zip(ys[:-1], ys[1:])], colour, out=out)
        assert np.array_equal(out, full), d
        out = np.full_like(full, 0x5a)
        for a, b in zip(xs[:-1], xs[1:]):
            ctx.frame_save_rects_async(lib_desc(d), [(a, 0, b - a, h)], colour, out=out)
        ctx.sync()
        assert np.array_equal(out, full), d
        dev = lib.DeviceArray(np.full_like(full, 0x5a))
        ctx.frame_save_rects(lib_desc(d), [(a, c, b - a, e - c) for a, b in zip(xs[:-1], xs[1:]) for c, e in zip(ys[:-1], ys[1:])],
                             colour, out=dev, bytes_per_row=full.strides[0])
        ctx.sync()
        got = dev.download(full.dtype, full.size).reshape(full.shape)
        dev.free()
        assert np.array_equal(got, full), d
    # no rects, and rects that are all empty: JXLH_OK, nothing written
    out = np.full_like(full, 0x5a)
    assert ctx.try_frame_save_rects(lib_desc(d), [], colour, out=out)[0] == lib.OK
    assert ctx.try_frame_save_rects(lib_desc(d), [(5, 5, 0, 9), (w + 1, h + 1, 0, 0)], colour, out=out)[0] == lib.OK
    ctx.sync()
    assert np.all(out == 0x5a)


REPAINT = [("gab_epf2", dict(epf_iters=2, gab=True), {}), ("gab_epf3", dict(epf_iters=3, gab=True), {}),
           ("noise", dict(epf_iters=0, gab=False), dict(noise=1, visible_frame_index=3)),
           ("420", dict(epf_iters=2, gab=True, hshift=(1, 0, 1), vshift=(1, 0, 1)), {})]
NOISE_LUT = [0.05 + 0.01 * i for i in range(8)]


def second_pass(wl, seed):
    """the workload with other coefficients: what each group holds once its later pass has arrived"""
    rng = np.random.default_rng(seed)
    new = copy.copy(wl)
    new.coeffs = np.where(rng.random(wl.coeffs.shape) < 0.5, wl.coeffs, 0).astype(np.int32)
    return new


@pytest.mark.parametrize("name,case,over", REPAINT, ids=[c[0] for c in REPAINT])
def test_repaint_after_rerender(ctx, oracle, name, case, over):
    """pass 1 saved whole into A; groups {4}, then {0, 8} change and only jxlh_changed_rects' rects are saved into A again:
    A is a fresh full save, and the save of the oracle's frame"""
    from jxl_rs_amd import lib, synth
    sub = "hshift" in case
    full = synth.make_vardct(600, 520, mix=synth.MIX_DCT8 if sub else synth.MIX_D1, seed=31, **case)  # 3 x 3 groups
    cur = second_pass(full, 3)  # the first pass holds about half of every group's coefficients
    p = gpu_params_from(ctx, cur, **over)
    if over:  # (an all-zero LUT would skip the stage)
        for i in range(8):
            p.noise_lut[i] = NOISE_LUT[i]
    ctx.frame_begin(p)
    ctx.set_dequant_tables(cur.tables)
    ctx.set_lf_quantized(*cur.lf_q)
    ctx.set_hf_meta(cur.transform_map, cur.raw_quant, cur.epf_map, cur.ytox, cur.ytob)
    for g in range(cur.coeffs.shape[0]):
        ctx.submit_group(g, cur.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    if sub:
        colour, ref_colour = ctx.output_desc(lib.COLOR_YCBCR, "linear", None, 0.0, LUM), ("ycbcr",)
    else:
        colour, ref_colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM), ("xyb", "srgb", xyb_params(oracle), 0.0, LUM)
    descs = [sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True), sr.desc([0, 1, 2], sr.F16, orientation=6)]
    A = [ctx.frame_save(lib_desc(d), colour) for d in descs]

    def oracle_planes(wl):
        want, _ = run_oracle_frame(oracle, wl)
        if over:
            rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(3, 0, wl.xsize, wl.ysize)]
            want = oracle.noise_add(np.float32(NOISE_LUT), 0.0, 1.0, want, rnd)
        return want

    for groups in ([4], [0, 8]):
        cur = copy.copy(cur)
        cur.coeffs = cur.coeffs.copy()
        for g in groups:
            cur.coeffs[g] = full.coeffs[g]
            ctx.submit_group(g, full.coeffs[g])
        ctx.slot_wait(0)
        ctx.rerender_groups(groups)
        rects = ctx.changed_rects(groups)
        assert len(rects) == len(groups)
        want = oracle_planes(cur)
        for d, a in zip(descs, A):
            before = a.copy()
            ctx.frame_save_rects(lib_desc(d), rects, colour, out=a)
            assert not np.array_equal(a, before), (name, groups)  # the pass did change the picture
            assert np.array_equal(a, ctx.frame_save(lib_desc(d), colour)), (name, groups, d["orientation"])
            assert np.array_equal(a, sr.save(oracle, d, want, ref_colour)), (name, groups, d["orientation"])


def test_repaint_of_a_group_going_from_lf_only_to_submitted(ctx, oracle):
    from jxl_rs_amd import lib, synth
    from lf_fill_ref import expected_planes
    wl = synth.make_vardct(600, 520, mix=synth.MIX_D1, seed=32, epf_iters=2)
    n = wl.xgroups * wl.ygroups
    marked = [4, 5]
    ctx.frame_begin(gpu_params_from(ctx, wl))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    ctx.set_groups_lf_only(marked)
    for g in range(n):
        if g not in marked:
            ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    ref_colour = ("xyb", "srgb", xyb_params(oracle), 0.0, LUM)
    d = sr.desc([0, 1, 2], sr.U8, orientation=5)
    a = ctx.frame_save(lib_desc(d), colour)
    assert np.array_equal(a, sr.save(oracle, d, expected_planes(oracle, wl, marked), ref_colour))
    for g in marked:  # the two neighbours arrive together: one rect
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.rerender_groups(marked)
    rects = ctx.changed_rects(marked)
    assert len(rects) == 1
    ctx.frame_save_rects(lib_desc(d), rects, colour, out=a)
    assert np.array_equal(a, ctx.frame_save(lib_desc(d), colour))
    assert np.array_equal(a, sr.save(oracle, d, run_oracle_frame(oracle, wl)[0], ref_colour))


def test_repaint_after_blend(ctx, oracle):
    """after jxlh_frame_blend the result is the canvas: the rects are shifted by the frame's (x0, y0) and clipped"""
    from jxl_rs_amd import lib, synth
    rng = np.random.default_rng(78)
    full = synth.make_vardct(600, 520, mix=synth.MIX_D1, seed=33, epf_iters=2)
    cur = second_pass(full, 4)
    w, h, iw, ih = full.xsize, full.ysize, 640, 500
    x0, y0 = -17, -23
    ctx.set_reference(0, [rng.uniform(-0.5, 1.5, (ih, iw)).astype(np.float32) for _ in range(4)])
    upload_frame(ctx, cur)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.frame_run()
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    bd = lib.blend_desc(x0, y0, iw, ih, (lib.BLEND_BLEND, 0, 1, 0), [(lib.BLEND_BLEND, 0, 0, 0)], [lib.EC_ALPHA])
    ctx.blend(bd, colour)
    d = sr.desc([0, 1, 2, 3], sr.U8, orientation=7)
    a = ctx.frame_save(lib_desc(d))
    groups = [0, 8]
    for g in groups:
        ctx.submit_group(g, full.coeffs[g])
    ctx.slot_wait(0)
    ctx.rerender_groups(groups)
    ctx.blend(bd, colour)
    shifted = []
    for rx, ry, rw, rh in ctx.changed_rects(groups).tolist():
        ax, ay, bx, by = max(0, rx + x0), max(0, ry + y0), min(iw, rx + rw + x0), min(ih, ry + rh + y0)
        if ax < bx and ay < by:
            shifted.append((ax, ay, bx - ax, by - ay))
    assert len(shifted) == 2
    before = a.copy()
    ctx.frame_save_rects(lib_desc(d), shifted, out=a)
    assert not np.array_equal(a, before)
    assert np.array_equal(a, ctx.frame_save(lib_desc(d)))
    pl = ctx.read_planes() + [ctx.read_extra_channel(0, iw, ih)]
    assert np.array_equal(a, sr.save(oracle, d, pl))
    # a colour stage on the blended frame is a state error, as for the save
    out = np.full_like(a, POISON)
    assert ctx.try_frame_save_rects(lib_desc(d), shifted, colour, out=out)[0] == lib.ERR_BAD_STATE and np.all(out == POISON)
    ctx.clear_reference(0)


# ---------------------------------------------------------------- errors
def test_argument_errors_write_nothing(ctx, planes):
    from jxl_rs_amd import lib
    INV = lib.ERR_INVALID_ARGUMENT
    W, H = SIZES[0]
    pl = planes[(W, H)]
    out = np.full((H + 8, (H + 8) * 16), POISON, np.uint8)  # large enough for every oriented image below
    good = dict(channels=[0, 1, 2], format=lib.SAVE_U8)
    whole = [(0, 0, W, H)]

    def call(desc, pl=pl, out=out, bpr=None, rects=whole, **kw):
        st, _ = ctx.try_stage_save_rects(desc, pl, rects, out=out, bytes_per_row=out.strides[0] if bpr is None else bpr, **kw)
        return st
    assert call(lib.save_desc(**good)) == lib.OK
    out[:] = POISON
    bad = [
        lib.save_desc([], lib.SAVE_U8),                                             # n_channels 0
        lib.save_desc([0, 1, 2, 3], lib.SAVE_U8, n_channels=5),                     # > 4
        lib.save_desc([0, 1, 2, 3], lib.SAVE_U8, fill_opaque_alpha=True),           # more than 4 samples with the fill
        lib.save_desc([0, 1, 11], lib.SAVE_U8),                                     # channel >= 3 + 8
        lib.save_desc([0, 1, 6], lib.SAVE_U8),                                      # ... a plane the call was not given
        lib.save_desc([0, 1, 2], 4),                                                # format
        lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=0),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=9),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, bit_depth=0),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, bit_depth=9),
        lib.save_desc([0, 1, 2], lib.SAVE_U16, bit_depth=17),
        lib.save_desc([0, 1, 2], lib.SAVE_F16, f16_clamp=(1.0, 0.0)),               # min > max
        lib.save_desc([0, 1, 2], lib.SAVE_F16, f16_clamp=(float("nan"), 1.0)),
        lib.save_desc([0, 1, 2], lib.SAVE_F16, f16_clamp=(0.0, float("nan"))),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=1),                       # not an extra channel
        lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=6),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(3, (0, 0, 0, 1))]),            # extra channel 3 of 3
        lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(8, (0, 0, 0, 1))]),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(0, (0, 0, 0, 1))], n_spot=9),
    ]
    for i, d in enumerate(bad):
        assert call(d) == INV, i
    d = lib.save_desc(**good)
    assert call(d, bpr=W * 3 - 1) == INV                                            # shorter than the row
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=5), bpr=H * 3 - 1) == INV   # ... the ORIENTED row
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=5), bpr=H * 3) == lib.OK
    out[:] = POISON
    d16 = lib.save_desc([0, 1, 2], lib.SAVE_U16)
    assert call(d16, bpr=W * 6 + 1) == INV                                          # pitch misaligned for the sample
    assert call(d16, out=out.reshape(-1)[1:], bpr=W * 6) == INV                     # ... and the origin
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_F32), out=out.reshape(-1)[2:], bpr=W * 12) == INV
    assert call(d, pl=pl[:2]) == INV                                                # fewer than three planes
    # the list's own refusals
    assert call(d, rects=[(W, 0, 1, 1)]) == INV and call(d, rects=[(0, H, 1, 1)]) == INV     # starts outside the result
    assert call(d, rects=[(0, 0, 1, 1), (W + 3, H + 3, 2, 2)]) == INV                        # ... behind a good one
    assert call(d, rects=[(1, 1, 0xffffffff, 1)]) == INV and call(d, rects=[(1, 1, 1, 0xffffffff)]) == INV  # overflow
    assert call(d, rects=[(0, 0, 1, 1)] * (lib.MAX_SAVE_RECTS + 1)) == INV
    L = lib.load()
    rect = np.array([[0, 0, 1, 1]], dtype=np.uint32)
    arr = (C.c_void_p * 3)(*[p.ctypes.data for p in pl[:3]])
    assert L.jxlh_stage_save_rects(ctx._ctx, None, C.byref(d), arr, 3, W, H, W, 0, 0, None, 1, out.ctypes.data,
                                   out.strides[0]) == INV                                # rects == NULL with n > 0
    assert L.jxlh_stage_save_rects(ctx._ctx, None, C.byref(d), arr, 3, W, H, W, 0, 0, None, 0, out.ctypes.data,
                                   out.strides[0]) == lib.OK                             # ... n == 0: nothing to do
    assert L.jxlh_stage_save_rects(ctx._ctx, None, None, None, 3, 4, 4, 4, 0, 0, rect.ctypes.data, 1, None, 16) == INV
    assert L.jxlh_frame_save_rects(ctx._ctx, None, None, rect.ctypes.data, 1, None, 0) == INV
    assert L.jxlh_frame_save_rects(None, None, None, rect.ctypes.data, 1, None, 0) == INV
    assert L.jxlh_frame_save_rects_async(None, None, None, rect.ctypes.data, 1, None, 0) == INV
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", np.zeros(16, np.float32))
    colour.transfer = 6
    assert call(d, colour=colour) == INV
    colour.color = 3
    assert call(d, colour=colour) == INV
    ctx.sync()
    assert np.all(out == POISON)
    # accepted: 4096 rects; an empty rect wherever it starts; a rect reaching past the 32-bit edge exactly
    assert call(d, rects=[(i % W, i % H, 1, 1) for i in range(lib.MAX_SAVE_RECTS)]) == lib.OK
    assert call(d, rects=[(W + 9, H + 9, 0, 0), (1, 1, 0xfffffffe, 0xfffffffe)]) == lib.OK


def test_state_errors_write_nothing(ctx, frame):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    BAD = lib.ERR_BAD_STATE
    rng = np.random.default_rng(80)
    w, h = frame.xsize, frame.ysize
    out = np.full((2 * h, 2 * w * 4), POISON, np.uint8)
    rgba = lib.save_desc([0, 1, 2, 3], lib.SAVE_U8)
    rgb = lib.save_desc([0, 1, 2], lib.SAVE_U8)
    rects = [(3, 5, 40, 30)]

    def call(c, desc, rects=rects, **kw):
        return c.try_frame_save_rects(desc, rects, out=out, bytes_per_row=out.strides[0], **kw)[0]
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        fresh.params = ctx.default_params(w, h)
        assert call(fresh, rgb) == BAD                                              # no frame
    finally:
        fresh.close()
    upload_frame(ctx, frame)
    assert call(ctx, rgb) == BAD                                                    # no result yet
    assert call(ctx, rgb, rects=[]) == BAD                                          # ... whatever the list holds
    ctx.frame_run()
    assert call(ctx, rgba) == BAD                                                   # extra channel 0 was never set
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=3)) == BAD
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(1, (0, 0, 0, 1))])) == BAD
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    assert call(ctx, rgba) == BAD                                                   # set, but no run since
    # the list is checked against the RESULT: a rect that starts outside it
    assert call(ctx, rgb, rects=[(w, 0, 1, 1)]) == lib.ERR_INVALID_ARGUMENT
    assert call(ctx, rgb, rects=[(0, h, 1, 1)]) == lib.ERR_INVALID_ARGUMENT
    assert call(ctx, rgb, wait=False, rects=[(0, h, 1, 1)]) == lib.ERR_INVALID_ARGUMENT
    assert np.all(out == POISON)
    ctx.frame_run()
    assert call(ctx, rgba) == lib.OK
    out[:] = POISON
    # an upsampled frame whose extra channel stayed at the frame's own size does not cover the result
    upload_frame(ctx, frame, upsampling=2)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.frame_run()
    assert ctx.out_size == (2 * w, 2 * h)
    assert call(ctx, rgba) == BAD
    assert call(ctx, lib.save_desc([3], lib.SAVE_U8)) == BAD
    assert np.all(out == POISON)
    assert call(ctx, rgb, rects=[(2 * w - 1, 2 * h - 1, 5, 5)]) == lib.OK           # the colour alone is fine, upsampled


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    out = np.full((600, 900), POISON, np.uint8)
    try:
        lib.comm_init_local(peers)
        for c in peers:
            upload_frame(c, wl)
            st, _ = c.try_frame_save_rects(lib.save_desc([0, 1, 2], lib.SAVE_U8), [(0, 0, 10, 10)], out=out)
            assert st == lib.ERR_UNSUPPORTED
            st, _ = c.try_frame_save_rects(lib.save_desc([0, 1, 2], lib.SAVE_U8), [(0, 0, 10, 10)], out=out, wait=False)
            assert st == lib.ERR_UNSUPPORTED
        assert np.all(out == POISON)
    finally:
        for c in peers:
            c.close()
