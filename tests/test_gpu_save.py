"""The save tail on the device (jxlh_stage_save / jxlh_frame_save, k_save.hip) against tests/save_ref.py, bit for bit:
every format, layout and orientation, bands, the in-place stages in the reference's order, the shipped 8 / 16-bit path,
frames with extra channels, patches, upsampling and blending, long axes, and the argument / state errors."""
import json
import os

import numpy as np
import pytest

import save_ref as sr
from helpers import run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = (0.2627, 0.678, 0.0593)
POISON = 0xA5
W, H = 301, 157  # no multiple of 4 or 64 anywhere


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planes():
    """3 colour + 3 extra channels, values in -0.5 .. 1.5"""
    rng = np.random.default_rng(2026)
    return [rng.uniform(-0.5, 1.5, (H, W)).astype(np.float32) for _ in range(6)]


def lib_desc(d):
    from jxl_rs_amd import lib
    return lib.save_desc(d["channels"], d["format"], d["bit_depth"], d["fill_opaque_alpha"], d["big_endian"],
                         d["orientation"], d["f16_clamp"], d["premultiply"], d["spot"])


def sample_bytes(d):
    return sr.SAMPLE_DTYPE[d["format"]]().itemsize


def poisoned(d, w, h, pad, lead):
    """(buffer, view at the image origin, bytes per row): the image's rows `pad` bytes apart beyond their samples, `lead`
    poisoned bytes in front and as many behind"""
    ow, oh = sr.oriented_size(d["orientation"], w, h)
    spp = len(d["channels"]) + (1 if d["fill_opaque_alpha"] else 0)
    row = ow * spp * sample_bytes(d)
    bpr = row + pad
    buf = np.full(lead + oh * bpr + lead, POISON, dtype=np.uint8)
    return buf, buf[lead:], bpr, row, oh


def check_image(buf, lead, bpr, row, oh, want, what):
    """the samples equal `want` ([oh, samples]) and every other byte of the buffer is untouched"""
    body = buf[lead:lead + oh * bpr].reshape(oh, bpr)
    got = np.ascontiguousarray(body[:, :row])
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(oh, row)
    if not np.array_equal(got, wb):
        bad = np.argwhere(got != wb)
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at row {y} byte {x}: got {got[y, x]} want {wb[y, x]}")
    assert np.all(body[:, row:] == POISON), f"{what}: bytes behind a row's samples were written"
    assert np.all(buf[:lead] == POISON) and np.all(buf[lead + oh * bpr:] == POISON), f"{what}: bytes around the image"


def run_stage(ctx, d, pl, want, what, colour=None, origin=(0, 0), pad=0, lead=16, device=False):
    """device: `out` is device memory (the kernel writes the caller's rows itself, at the caller's alignment); else host
    memory, which goes through the staging buffer and a 2-D copy"""
    from jxl_rs_amd import lib
    h, w = pl[0].shape
    bps = sample_bytes(d)
    buf, view, bpr, row, oh = poisoned(d, w, h, pad * bps, lead)
    dev = lib.DeviceArray(buf) if device else None
    st, _ = ctx.try_stage_save(lib_desc(d), pl, colour, origin, out=dev.ptr + lead if device else view, bytes_per_row=bpr)
    if device:
        buf = dev.download(np.uint8, buf.size)
        dev.free()
    assert st == 0, (what, st)
    check_image(buf, lead, bpr, row, oh, want, what)


# ---------------------------------------------------------------- formats x layouts
FORMATS = [
    ("u8", dict(format=sr.U8, bit_depth=8)), ("u8_5", dict(format=sr.U8, bit_depth=5)),
    ("u8_1", dict(format=sr.U8, bit_depth=1)),
    ("u16_le", dict(format=sr.U16, bit_depth=16)), ("u16_be", dict(format=sr.U16, bit_depth=16, big_endian=True)),
    ("u16_10_le", dict(format=sr.U16, bit_depth=10)), ("u16_10_be", dict(format=sr.U16, bit_depth=10, big_endian=True)),
    ("f16_le", dict(format=sr.F16)), ("f16_be", dict(format=sr.F16, big_endian=True)),
    ("f16_le_pq", dict(format=sr.F16, f16_clamp=sr.F16_CLAMP_PQ)),
    ("f16_be_pq", dict(format=sr.F16, f16_clamp=sr.F16_CLAMP_PQ, big_endian=True)),
    ("f16_le_hlg", dict(format=sr.F16, f16_clamp=sr.F16_CLAMP_HLG)),
    ("f16_be_hlg", dict(format=sr.F16, f16_clamp=sr.F16_CLAMP_HLG, big_endian=True)),
    ("f32_le", dict(format=sr.F32)), ("f32_be", dict(format=sr.F32, big_endian=True)),
]


def layouts():
    out = [("gray", [0], False), ("rgb", [0, 1, 2], False), ("rgba_filled", [0, 1, 2], True), ("bgr", [2, 1, 0], False),
           ("gray_filled", [0], True)]
    for ec in (0, 2):  # the alpha's dither phase is that of pipeline channel 3 + ec
        out += [(f"gray_alpha_ec{ec}", [0, 3 + ec], False), (f"rgba_ec{ec}", [0, 1, 2, 3 + ec], False),
                (f"bgra_ec{ec}", [2, 1, 0, 3 + ec], False)]
    return out


@pytest.mark.parametrize("name,fmt", FORMATS, ids=[f[0] for f in FORMATS])
def test_formats_and_layouts(ctx, oracle, planes, name, fmt):
    for i, (lname, channels, fill) in enumerate(layouts()):
        d = sr.desc(channels, fill_opaque_alpha=fill, **fmt)
        want = sr.save(oracle, d, planes)
        run_stage(ctx, d, planes, want, f"{name} {lname}", pad=(0, 3, 4)[i % 3], device=i % 2 == 1)


def test_dither_phase_follows_the_pipeline_channel(oracle, planes):
    """the restatement itself tells alpha from extra channel 2 (channel 5) apart from channel 3"""
    a = sr.f32_to_u8(planes[5], np.arange(W)[None, :], np.arange(H)[:, None], 5)
    b = sr.f32_to_u8(planes[5], np.arange(W)[None, :], np.arange(H)[:, None], 3)
    assert np.any(a != b)


# ---------------------------------------------------------------- orientations
def orientation_sizes():
    from jxl_rs_amd import lib
    sizes = [(1, 1), (1, 67), (67, 1), (3, 5)]
    # the implementation's own tile sides, asked of the library for every pixel size tested below
    tiles = {t for pb in (1, 3, 4, 8, 16) for t in lib.save_tile_layout(pb)}
    sides = sorted({t + d for t in tiles for d in (-1, 0, 1)})
    sizes += [(a, b) for a in sides for b in sides]
    return sizes + [(W, H)]


PIXELS = [("1B", dict(channels=[0], format=sr.U8)), ("3B", dict(channels=[0, 1, 2], format=sr.U8)),
          ("4B", dict(channels=[0, 1, 2, 3], format=sr.U8)), ("8B", dict(channels=[0, 1, 2, 3], format=sr.U16)),
          ("16B", dict(channels=[2, 1, 0, 4], format=sr.F32))]


@pytest.mark.parametrize("name,px", PIXELS, ids=[p[0] for p in PIXELS])
def test_orientations(ctx, oracle, name, px):
    rng = np.random.default_rng(len(name) * 77)
    bps = sr.SAMPLE_DTYPE[px["format"]]().itemsize
    for n, (w, h) in enumerate(orientation_sizes()):
        pl = [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(5)]
        samples = sr.save_samples(oracle, sr.desc(**px), pl)
        for o in range(1, 9):
            d = sr.desc(orientation=o, **px)
            want = sr.orient(samples, o)
            want = want.reshape(want.shape[0], -1)
            # row strides: tight, dword-aligned with padding, and (for samples below 4 bytes) no multiple of four
            pad = (0, 4 // bps * 3, 1 if bps < 4 else 2)[(n + o) % 3]
            run_stage(ctx, d, pl, want, f"{name} {w}x{h} orientation {o} pad {pad}", pad=pad, lead=(16, 16 + bps)[o % 2],
                      device=(n // 3 + o) % 2 == 0)


# ---------------------------------------------------------------- bands
@pytest.mark.parametrize("orientation", [1, 4, 6, 7])
@pytest.mark.parametrize("device_out", [False, True], ids=["host", "device"])
def test_bands_assemble_to_the_whole_image(ctx, oracle, planes, orientation, device_out):
    from jxl_rs_amd import lib
    cuts = [0, 1, 30, 31, 64, 97, 156, H]
    for fmt, channels in ((sr.U8, [0, 1, 2, 3]), (sr.U8, [0]), (sr.F16, [0, 1, 2])):
        d = sr.desc(channels, fmt, orientation=orientation)
        want = sr.save(oracle, d, planes)
        bps = sample_bytes(d)
        buf, view, bpr, row, oh = poisoned(d, W, H, 6 * bps, 16)
        dev = lib.DeviceArray(buf) if device_out else None
        for y0, y1 in zip(cuts[:-1], cuts[1:]):
            out = dev.ptr + 16 if device_out else view
            st, _ = ctx.try_stage_save(lib_desc(d), planes, y0=y0, y1=y1, out=out, bytes_per_row=bpr)
            assert st == 0
        if device_out:
            ctx.sync()
            buf = dev.download(np.uint8, buf.size)
            dev.free()
        check_image(buf, 16, bpr, row, oh, want, f"bands, orientation {orientation}, format {fmt}")


# ---------------------------------------------------------------- the in-place stages in front of the conversion
def test_spot_colours_and_premultiply(ctx, oracle, planes):
    pl = [p.copy() for p in planes]
    pl[3][:8, :8] = np.nan          # a NaN spot sample
    pl[4][:4, :] = 0.0              # alpha 0
    pl[4][4:8, :] = 1.0             # alpha 1
    pl[4][8:12, :] = 1.75           # alpha > 1
    pl[4][12:16, :] = -0.5          # negative alpha
    spots = [(0, (0.9, 0.1, 0.3, 0.7)), (2, (0.2, 0.8, 0.5, 0.0)), (1, (0.05, 0.6, 1.0, 1.6))]  # scale 0, scale > 1
    cases = []
    for n in (1, 2, 3):
        cases.append(sr.desc([0, 1, 2], sr.F32, spot=spots[:n]))
    cases.append(sr.desc([0, 1, 2], sr.F32, spot=list(reversed(spots))))  # the order matters
    cases.append(sr.desc([0, 1, 2, 4], sr.F32, premultiply=4))
    cases.append(sr.desc([0, 4], sr.F16, premultiply=4))
    cases.append(sr.desc([2, 1, 0, 4], sr.U8, premultiply=4, spot=spots[:2]))       # spot + premultiply + U8
    cases.append(sr.desc([0, 1, 2, 4], sr.U16, 10, premultiply=4, spot=spots, orientation=6))
    cases.append(sr.desc([3], sr.F32, premultiply=4, spot=spots))  # an extra-channel save carries neither
    ordered = sr.save(oracle, cases[2], pl)
    assert not np.array_equal(ordered, sr.save(oracle, cases[3], pl))
    for i, d in enumerate(cases):
        run_stage(ctx, d, pl, sr.save(oracle, d, pl), f"stages case {i}", pad=i % 2)


def test_f16_edge_plane(ctx, oracle):
    from test_save_ref_cpu import f16_boundary_values
    v = f16_boundary_values()
    w = 97
    n = (v.size + w - 1) // w * w
    plane = np.zeros(n, np.float32)
    plane[:v.size] = v
    plane = plane.reshape(-1, w)
    pl = [plane, plane[::-1].copy(), plane.copy()]
    for clamp in (None, sr.F16_CLAMP_PQ, sr.F16_CLAMP_HLG):
        for o in (1, 5):
            d = sr.desc([0, 1], sr.F16, f16_clamp=clamp, orientation=o)
            run_stage(ctx, d, pl, sr.save(oracle, d, pl), f"f16 edges clamp {clamp} orientation {o}")
    d = sr.desc([0], sr.F32, big_endian=True)  # NaN payloads and denormals pass f32 untouched
    run_stage(ctx, d, pl, sr.save(oracle, d, pl), "f32 edges")


# ---------------------------------------------------------------- whole frames
def xyb_params(oracle, intensity_target=255.0):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["output_stage"]
    return oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, intensity_target)


@pytest.fixture(scope="module")
def frame():
    from jxl_rs_amd import synth
    return synth.make_vardct(300, 260, mix=synth.MIX_D1, seed=42, epf_iters=2)


@pytest.mark.parametrize("color,tf,param", [("xyb", "srgb", 0.0), ("xyb", "pq", 10000.0), ("ycbcr", "linear", 0.0),
                                            ("none", "linear", 0.0)], ids=["xyb_srgb", "xyb_pq", "ycbcr", "none"])
def test_identity_saves_equal_read_output(ctx, oracle, frame, color, tf, param):
    """RGB and opaque-RGBA 8 / 16-bit identity saves are the shipped path's bytes"""
    from jxl_rs_amd import lib
    upload_frame(ctx, frame)
    ctx.frame_run()
    code = {"xyb": lib.COLOR_XYB, "ycbcr": lib.COLOR_YCBCR, "none": lib.COLOR_NONE}[color]
    params = xyb_params(oracle, param if tf == "pq" else 255.0) if color == "xyb" else None
    colour = ctx.output_desc(code, tf, params, param, LUM)
    for bits, fmt in ((8, lib.SAVE_U8), (16, lib.SAVE_U16)):
        for channels in (3, 4):
            want = ctx.read_output(code, tf, params, param, LUM, bits, channels)
            got = ctx.frame_save(lib.save_desc([0, 1, 2], fmt, fill_opaque_alpha=channels == 4), colour)
            assert np.array_equal(got, want.reshape(got.shape)), (color, tf, bits, channels)
            rows = ctx.frame_save(lib.save_desc([0, 1, 2], fmt, fill_opaque_alpha=channels == 4), colour, y0=33, y1=190)
            assert np.array_equal(rows[33:190], want.reshape(got.shape)[33:190]) and not rows[:33].any()


def colour_tuple(oracle):
    return ("xyb", "srgb", xyb_params(oracle), 0.0, LUM)


def test_frame_with_extra_channels_patches_and_orientation(ctx, oracle, frame):
    """two extra channels, one of them at half size and upsampled 2x to the frame's, patches drawn into colour and extra
    channels: RGBA8 with alpha from the upsampled channel, the colour stage in front, orientation 6"""
    from jxl_rs_amd import lib
    from test_gpu_patches import _frame_dictionary
    rng = np.random.default_rng(77)
    w, h = frame.xsize, frame.ysize
    refs = [rng.uniform(-0.5, 1.5, (256, 512)).astype(np.float32) for _ in range(5)]
    ctx.set_reference(0, refs)
    ctx.set_reference(1, [r[::-1].copy() for r in refs])
    upload_frame(ctx, frame)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.set_extra_channel(1, rng.integers(0, 1 << 16, size=(h // 2, w // 2)).astype(np.int32), 16, 2)
    patches, blendings = _frame_dictionary(rng, w, h, 2, 60)
    ctx.set_patches(patches, blendings, [lib.EC_ALPHA, lib.EC_ALPHA])
    ctx.frame_run()
    pl = ctx.read_planes() + [ctx.read_extra_channel(i, w, h) for i in range(2)]
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    for d in (sr.desc([0, 1, 2, 4], sr.U8, orientation=6), sr.desc([0, 1, 2, 3], sr.U8, orientation=1),
              sr.desc([4], sr.U16, orientation=8), sr.desc([0, 1, 2, 4], sr.F16, premultiply=4, orientation=6)):
        want = sr.save(oracle, d, pl, colour_tuple(oracle))
        got = ctx.frame_save(lib_desc(d), colour)
        assert np.array_equal(got, want), d
    # the planes are untouched: the same bytes again, and read_planes as before
    d = sr.desc([0, 1, 2, 4], sr.U8, orientation=6)
    assert np.array_equal(ctx.frame_save(lib_desc(d), colour), sr.save(oracle, d, pl, colour_tuple(oracle)))
    assert all(np.array_equal(a, b) for a, b in zip(ctx.read_planes(), pl[:3]))
    # _async + sync, into a host band
    full = sr.save(oracle, d, pl, colour_tuple(oracle))
    out = np.zeros_like(full)
    st, _ = ctx.try_frame_save(lib_desc(d), colour, y0=100, y1=200, out=out, wait=False)
    assert st == 0
    ctx.sync()
    lo, hi = (h - 200) * 4, (h - 100) * 4  # rotate 90 cw: source rows 100..199 are columns h-200 .. h-101
    assert np.array_equal(out[:, lo:hi], full[:, lo:hi]) and not out[:, :lo].any() and not out[:, hi:].any()
    for s in (0, 1):
        ctx.clear_reference(s)


def test_blended_frame(ctx, oracle, frame):
    """after jxlh_frame_blend at a negative origin onto a 333 x 281 image: the dither runs at image coordinates, the
    alpha is the canvas channel, and a colour stage other than NONE is a state error"""
    from jxl_rs_amd import lib
    rng = np.random.default_rng(78)
    w, h = frame.xsize, frame.ysize
    iw, ih = 333, 281
    ctx.set_reference(0, [rng.uniform(-0.5, 1.5, (ih, iw)).astype(np.float32) for _ in range(4)])
    upload_frame(ctx, frame)
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.frame_run()
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)
    bd = lib.blend_desc(-17, -9, iw, ih, (lib.BLEND_BLEND, 0, 1, 0), [(lib.BLEND_BLEND, 0, 0, 0)], [lib.EC_ALPHA])
    ctx.blend(bd, colour)
    assert ctx.out_size == (iw, ih)
    pl = ctx.read_planes() + [ctx.read_extra_channel(0, iw, ih)]
    for d in (sr.desc([0, 1, 2, 3], sr.U8), sr.desc([2, 1, 0, 3], sr.U8, 5, orientation=7, premultiply=3)):
        assert np.array_equal(ctx.frame_save(lib_desc(d)), sr.save(oracle, d, pl)), d
    d = sr.desc([0, 1, 2, 3], sr.U8)
    out = np.full(sr.save(oracle, d, pl).shape, POISON, np.uint8)
    st, _ = ctx.try_frame_save(lib_desc(d), colour, out=out)
    assert st == lib.ERR_BAD_STATE and np.all(out == POISON)
    ctx.clear_reference(0)


def test_subsampled_ycbcr_frame(ctx, oracle):
    """a 4:2:0 frame with nothing behind the transforms keeps its chroma sub-sampled until asked: the save materialises it"""
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(150, 130, mix=synth.MIX_8X8, seed=7, epf_iters=0, hshift=(1, 0, 1), vshift=(1, 0, 1))
    upload_frame(ctx, wl, gab=0)
    ctx.frame_run()
    colour = ctx.output_desc(lib.COLOR_YCBCR, "linear", None, 0.0, LUM)
    d = sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True, orientation=5)
    got = ctx.frame_save(lib_desc(d), colour)
    pl = ctx.read_planes()
    assert np.array_equal(got, sr.save(oracle, d, pl, ("ycbcr",)))
    upload_frame(ctx, wl, gab=0)
    ctx.frame_run()
    rgba = ctx.read_ycbcr_rgb8(4)
    upload_frame(ctx, wl, gab=0)
    ctx.frame_run()
    d1 = sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True)
    assert np.array_equal(ctx.frame_save(lib_desc(d1), colour), rgba.reshape(130, -1))


def test_extra_channel_only_save(ctx, oracle, frame):
    rng = np.random.default_rng(79)
    w, h = frame.xsize, frame.ysize
    upload_frame(ctx, frame)
    for i in range(3):
        ctx.set_extra_channel(i, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    ctx.frame_run()
    pl = ctx.read_planes() + [ctx.read_extra_channel(i, w, h) for i in range(3)]
    for d in (sr.desc([5], sr.U8), sr.desc([4], sr.U16, 12, big_endian=True, orientation=2), sr.desc([3], sr.F32)):
        assert np.array_equal(ctx.frame_save(lib_desc(d)), sr.save(oracle, d, pl)), d


# ---------------------------------------------------------------- axes longer than 65 535
@pytest.mark.parametrize("w,h", [(3, 65537), (65537, 3)])
def test_long_axes(ctx, oracle, w, h):
    rng = np.random.default_rng(w)
    pl = [rng.uniform(-0.5, 1.5, (h, w)).astype(np.float32) for _ in range(3)]
    samples = sr.save_samples(oracle, sr.desc([0, 1, 2], sr.U8), pl)
    for o in (1, 5):
        want = sr.orient(samples, o)
        run_stage(ctx, sr.desc([0, 1, 2], sr.U8, orientation=o), pl, want.reshape(want.shape[0], -1), f"{w}x{h} o{o}")


# ---------------------------------------------------------------- errors
def test_argument_errors_write_nothing(ctx, planes):
    from jxl_rs_amd import lib
    INV = lib.ERR_INVALID_ARGUMENT
    out = np.full((W + 8, (W + 8) * 16), POISON, np.uint8)  # large enough for every oriented image below
    good = dict(channels=[0, 1, 2], format=lib.SAVE_U8)

    def call(desc, pl=planes, out=out, bpr=None, **kw):
        st, _ = ctx.try_stage_save(desc, pl, out=out, bytes_per_row=out.strides[0] if bpr is None else bpr, **kw)
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
    assert call(d, y0=5, y1=5) == INV and call(d, y0=H, y1=H + 4) == INV            # no rows
    assert call(d, pl=planes[:2]) == INV                                            # fewer than three planes
    L = lib.load()
    assert L.jxlh_stage_save(ctx._ctx, None, None, None, 3, 4, 4, 4, 0, 0, 0, 4, None, 16) == INV
    assert L.jxlh_frame_save(ctx._ctx, None, None, 0, 1, None, 0) == INV
    assert L.jxlh_frame_save(None, None, None, 0, 1, None, 0) == INV
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", np.zeros(16, np.float32))
    colour.transfer = 6
    assert call(d, colour=colour) == INV
    colour.color = 3
    assert call(d, colour=colour) == INV
    assert np.all(out == POISON)


def test_state_errors_write_nothing(ctx, frame):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    BAD = lib.ERR_BAD_STATE
    rng = np.random.default_rng(80)
    w, h = frame.xsize, frame.ysize
    out = np.full((2 * h, 2 * w * 4), POISON, np.uint8)
    rgba = lib.save_desc([0, 1, 2, 3], lib.SAVE_U8)

    def call(c, desc, **kw):
        return c.try_frame_save(desc, out=out, bytes_per_row=out.strides[0], **kw)[0]
    fresh = jxl_rs_amd.Context(0, 1)
    try:
        fresh.params = ctx.default_params(w, h)
        assert call(fresh, lib.save_desc([0, 1, 2], lib.SAVE_U8)) == BAD            # no frame
    finally:
        fresh.close()
    upload_frame(ctx, frame)
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8)) == BAD                  # no result yet
    ctx.frame_run()
    assert call(ctx, rgba) == BAD                                                   # extra channel 0 was never set
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=3)) == BAD
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(1, (0, 0, 0, 1))])) == BAD
    ctx.set_extra_channel(0, rng.integers(0, 1 << 16, size=(h, w)).astype(np.int32), 16)
    assert call(ctx, rgba) == BAD                                                   # set, but no run since
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
    assert call(ctx, lib.save_desc([0, 1, 2], lib.SAVE_U8)) == lib.OK               # the colour alone is fine


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
            st, _ = c.try_frame_save(lib.save_desc([0, 1, 2], lib.SAVE_U8), out=out)
            assert st == lib.ERR_UNSUPPORTED
        assert np.all(out == POISON)
    finally:
        for c in peers:
            c.close()
