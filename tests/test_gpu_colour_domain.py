"""The colour stage (csrc/color_device.h) held to the oracle over the whole binary32 domain, through each consumer's own
dispatch over the mode: the save kernel (k_save.hip, f32 out: the stage's result with no quantisation in front of the
comparison), frame blending (k_blend.hip), the 8-bit read-out (k_output.hip) and the integer / half conversions behind
it.  Run with -m gpu on an MI355X.  The LF preview runs all its curves on its own inputs in test_gpu_lf_preview.py.

Inputs are the planes of tests/colour_domain_cases.py: exact +-0, denormals, both sides of every curve's branch point,
out-of-gamut negatives, values far above 1, overflow to inf / inf, +-inf and NaN.  test_colour_domain_cpu.py proves on the
oracle that they reach those places.  The expectation always comes from the oracle (save_ref.colour_stage, save_ref.save),
never from another device path.

THE COMPARISON RULE (colour_domain_cases.float_bits_mismatch).  Float outputs (f32, and f16 as bits): where the wanted
value is not NaN the bits are equal, the sign of zero and +-inf included; where it is NaN the device value is NaN, with
payload and sign free -- x86 and the GPU make different default NaNs and propagate different operands' payloads, and so
do the reference's own scalar and SIMD back ends.  Nothing is masked out.  Integer outputs: every byte is equal (the
conversions send NaN to 0 and +inf to the maximum on both sides: convert.rs:603, :757 clamp as max(0) then min(top), and
so do jxlo_f32_to_u8 / _u16 and convert_sample of csrc/save_device.h, as selects that let a NaN fall to 0)."""
import numpy as np
import pytest

import colour_domain_cases as cd
import save_ref as sr

pytestmark = pytest.mark.gpu

F32_MODULAR = 32 | 8 << 8  # a float Modular frame: binary32 samples, widened exactly


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    for s in range(4):
        c.clear_reference(s)
    yield c
    c.close()


@pytest.fixture(scope="module")
def planes():
    """every set of input planes, made once and never written"""
    out = {"main": cd.main_planes(), "tail": cd.tail_planes(), "threshold": cd.threshold_planes()[0],
           "display": cd.display_planes()}
    for pl in out.values():
        for p in pl:
            p.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def wanted(oracle, planes):
    """wanted(plane set, label, colour) -> the oracle's colour stage on it, computed once and shared by the tests"""
    cache = {}

    def get(which, label, colour):
        if (which, label) not in cache:
            rgb = sr.colour_stage(oracle, planes[which], colour)
            for p in rgb:
                p.setflags(write=False)
            cache[which, label] = rgb
        return cache[which, label]
    return get


def _lib_colour(ctx, colour):
    from jxl_rs_amd import lib
    if colour[0] != "xyb":
        return ctx.output_desc(lib.COLOR_YCBCR if colour[0] == "ycbcr" else lib.COLOR_NONE, "linear", None, 0.0, cd.LUM)
    _, transfer, params, param, lum = colour
    return ctx.output_desc(lib.COLOR_XYB, transfer, params, param, lum)


def _lib_save_desc(d):
    from jxl_rs_amd import lib
    return lib.save_desc(d["channels"], d["format"], d["bit_depth"], d["fill_opaque_alpha"], d["big_endian"],
                         d["orientation"], d["f16_clamp"], d["premultiply"], d["spot"])


def _pixel(pl, y, x):
    return " ".join(f"{n}={p[y, x]!r}/{int(p.view(np.uint32)[y, x]):#010x}" for n, p in zip("XYB", pl))


def _assert_float_image(got, want, spp, pl, what):
    """got, want: [h, w * spp] bit images (uint32 / uint16) under the comparison rule"""
    got = np.asarray(got).reshape(want.shape)
    bad = cd.float_bits_mismatch(got, want)
    if bad.any():
        at = np.argwhere(bad)
        y, s = at[0]
        raise AssertionError(f"{what}: {len(at)} of {bad.size} samples break the rule; first at row {y} pixel {s // spp} "
                             f"channel {s % spp}: got {int(got[y, s]):#x} want {int(want[y, s]):#x}; input {_pixel(pl, y, s // spp)}")


def _assert_bytes(got, want, spp, pl, what):
    got = np.asarray(got).reshape(want.shape)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    bad = got != want
    if bad.any():
        at = np.argwhere(bad)
        y, s = at[0]
        raise AssertionError(f"{what}: {len(at)} of {bad.size} samples differ; first at row {y} pixel {s // spp} channel "
                             f"{s % spp}: got {int(got[y, s])} want {int(want[y, s])}; input {_pixel(pl, y, s // spp)}")


def _interleaved_bits(rgb):
    h, w = rgb[0].shape
    return np.ascontiguousarray(np.stack(rgb, axis=-1)).view(np.uint32).reshape(h, w * 3)


# ---------------------------------------------------------------- a. the save kernel, f32 out
EXACT_PLANES = ("main", "tail", "threshold")

@pytest.mark.parametrize("which", EXACT_PLANES)
@pytest.mark.parametrize("case", cd.colour_cases(), ids=cd.case_id)
def test_save_kernel_f32_is_the_oracles_colour_stage(ctx, oracle, planes, wanted, case, which):
    """jxlh_stage_save, SAVE_F32, every curve x every XYB parameter set on the main sweep, the tail and the threshold rows.
    The tail with the identity matrix is where opsin_fma of csrc/color_device.h shows: a pixel whose B is a NaN
    while X + Y cubes to +-inf runs fma(0, +-inf, NaN) in XybStage's matrix (xyb.rs:231-233), and gamma and HLG make a
    number of the NaN that comes out (30 of the plane's 5328 samples differed before the device handed on the addend)."""
    from jxl_rs_amd import lib
    label, colour = cd.colour_of(oracle, case)
    got = ctx.stage_save(lib.save_desc([0, 1, 2], lib.SAVE_F32), planes[which], _lib_colour(ctx, colour))
    _assert_float_image(got, _interleaved_bits(wanted(which, label, colour)), 3, planes[which], f"save f32, {which}, {label}")


# ---------------------------------------------------------------- the Modular frame the other consumers read
def _render(ctx, pl):
    """the planes as a float Modular frame without filters: the frame's result is the bit patterns themselves"""
    h, w = pl[0].shape
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = 0, 0
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*[np.ascontiguousarray(a).view(np.int32) for a in pl], F32_MODULAR)
    ctx.frame_run()


def test_modular_frame_carries_every_bit_pattern(ctx, planes):
    for which, pl in planes.items():
        _render(ctx, pl)
        ctx.sync()
        for c, (g, e) in enumerate(zip(ctx.read_planes(), pl)):
            assert np.array_equal(g.view(np.uint32), e.view(np.uint32)), (which, c)


# ---------------------------------------------------------------- b. the blend kernel
@pytest.mark.parametrize("which", EXACT_PLANES)
@pytest.mark.parametrize("case", cd.colour_cases((cd.IDENTITY_XYB, "default_255")), ids=cd.case_id)
def test_blend_kernel_colour_stage(ctx, oracle, planes, wanted, case, which):
    """jxlh_frame_blend, Replace over the full frame with the colour stage in front: the image's planes are the oracle's
    colour stage.  The identity and the default parameters at 255: the subject is k_blend.hip's dispatch, and with it
    BT.709, HLG, gamma and non-finite samples through that kernel."""
    from jxl_rs_amd import lib
    pl = planes[which]
    h, w = pl[0].shape
    label, colour = cd.colour_of(oracle, case)
    _render(ctx, pl)
    ctx.blend(lib.blend_desc(0, 0, w, h, (lib.BLEND_REPLACE, 0, 0, 0)), _lib_colour(ctx, colour))
    assert ctx.out_size == (w, h)
    _assert_float_image(_interleaved_bits(ctx.read_planes()), _interleaved_bits(wanted(which, label, colour)), 3, pl,
                        f"blend, {which}, {label}")


# ---------------------------------------------------------------- c. read-outs and the integer / half formats
SAVES = [("u8", sr.U8, 8), ("u8_5", sr.U8, 5), ("u16", sr.U16, 16), ("u16_10", sr.U16, 10), ("f16", sr.F16, 0)]


@pytest.mark.parametrize("name", cd.ONE_EACH)
def test_read_outs_and_integer_formats(ctx, oracle, planes, name):
    """On the float Modular frame: jxlh_frame_read_output at 8 bits (k_output.hip's own kernel and dispatch) and 16 bits
    with 3 and 4 channels, jxlh_frame_save as U8 (8, 5 bits), U16 (16, 10 bits) and F16 -- on the display-range plane
    (many code values inside the range) and on the tail (NaN -> 0, +inf -> max, -inf -> 0; f16 keeps NaN and inf), and at
    16 bits on the main sweep."""
    from jxl_rs_amd import lib
    _, kind, transfer, param = cd.curve(name)
    label, colour = cd.colour_tuples(oracle, name, ["default_255"])[0]
    code = {"xyb": lib.COLOR_XYB, "ycbcr": lib.COLOR_YCBCR, "none": lib.COLOR_NONE}[kind]
    params = colour[2] if kind == "xyb" else None
    for which in ("display", "tail", "main"):
        pl = planes[which]
        _render(ctx, pl)
        for bits, fmt in ((8, sr.U8), (16, sr.U16)):
            if which == "main" and bits == 8:
                continue
            for channels in (3, 4):
                want = sr.save(oracle, sr.desc([0, 1, 2], fmt, fill_opaque_alpha=channels == 4), pl, colour)
                got = ctx.read_output(code, transfer, params, param, cd.LUM, bits, channels)
                _assert_bytes(got, want, channels, pl, f"read_output {bits} bits x {channels}, {which}, {label}")
        for sname, fmt, depth in SAVES:
            if which == "main" and sname != "u16":
                continue
            d = sr.desc([0, 1, 2], fmt, depth)
            want = sr.save(oracle, d, pl, colour)
            got = ctx.frame_save(_lib_save_desc(d), _lib_colour(ctx, colour))
            what = f"frame_save {sname}, {which}, {label}"
            if fmt == sr.F16:
                _assert_float_image(got, want, 3, pl, what)
            else:
                _assert_bytes(got, want, 3, pl, what)
