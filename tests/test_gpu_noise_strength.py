"""Noise::strength on the device (noise_strength of csrc/k_noise.hip), held to the CPU oracle bit for bit over the
planes of tests/noise_strength_cases.py: every interval of the LUT, exactly on each integer, the saturation branch up
to +inf, negatives, -0.0 and NaN, from the in_g side and from the in_r side, under LUTs that make a wrong index show
and make both clamps fire.  Through the stage hook (k_noise_add) and through a float Modular frame with noise on
(the frame path's fused k_noise_apply<0>).  Run with -m gpu on an MI355X.

Where the oracle's value is a NaN (a non-finite X or Y) the device value is a NaN; everywhere else, the finite B plane
of those pixels included, the bits are equal (noise_strength_cases.float_bits_mismatch)."""
import numpy as np
import pytest

import noise_strength_cases as N

pytestmark = pytest.mark.gpu
F = np.float32
F32_MODULAR = 32 | 8 << 8  # a float Modular frame: binary32 samples, widened exactly


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def _hold(got, want, planes, lut_name, what):
    with np.errstate(all="ignore"):
        fi_g, _, sat_g = N.interval((planes[1] - planes[0]) * F(0.5))
        fi_r, _, sat_r = N.interval((planes[1] + planes[0]) * F(0.5))
    for c in range(3):
        bad = N.float_bits_mismatch(got[c], want[c])
        if bad.any():
            y, x = np.argwhere(bad)[0].tolist()
            pytest.fail(f"{what}, LUT {lut_name}, plane {c}: {int(bad.sum())} of {bad.size} samples differ; first at "
                        f"(x {x}, y {y}): got {got[c][y, x]!r} want {want[c][y, x]!r}; X {planes[0][y, x]!r} Y "
                        f"{planes[1][y, x]!r}: in_g interval {fi_g[y, x]} saturated {bool(sat_g[y, x])}, in_r interval "
                        f"{fi_r[y, x]} saturated {bool(sat_r[y, x])}")


@pytest.mark.parametrize("lut_name", list(N.LUTS))
@pytest.mark.parametrize("ytox_lf,ytob_lf", [(0, 0), (7, -3)])
def test_stage_noise_add(ctx, oracle, lut_name, ytox_lf, ytob_lf):
    lut = N.LUTS[lut_name]
    w, h = 40, 17
    planes, rnd = N.planes(w, h), N.random_planes(w, h)
    p = ctx.default_params(8, 8)
    for i in range(8):
        p.noise_lut[i] = float(lut[i])
    p.ytox_lf, p.ytob_lf = ytox_lf, ytob_lf
    ytox = float(F(p.base_correlation_x) + F(ytox_lf) / F(p.color_factor))
    ytob = float(F(p.base_correlation_b) + F(ytob_lf) / F(p.color_factor))
    with np.errstate(all="ignore"):
        got = ctx.stage_noise_add(p, planes, rnd)
        want = oracle.noise_add(lut, ytox, ytob, planes, rnd)
    _hold(got, want, planes, lut_name, "stage_noise_add")
    if lut_name == "zero":
        assert all(np.array_equal(g.view(np.uint32), a.view(np.uint32)) for g, a in zip(got, planes)), "planes left alone"
    else:
        assert not np.array_equal(got[2].view(np.uint32), planes[2].view(np.uint32))


@pytest.mark.parametrize("lut_name", list(N.LUTS))
@pytest.mark.parametrize("size", [(40, 17), (300, 258)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_modular_frame_with_noise(ctx, oracle, lut_name, size):
    """a Modular frame of binary32 samples, no filters, noise = 1: generation, ConvolveNoise x3 and AddNoise in the
    fused kernel; 300 x 258 is more than one 256 x 256 noise tile each way"""
    w, h = size
    lut = N.LUTS[lut_name]
    planes = N.planes(w, h)
    chans = [np.ascontiguousarray(a).view(np.int32) for a in planes]
    for c in range(3):  # the intake widens binary32 exactly: the planes are the samples
        back = oracle.modular_to_f32(chans[c], 32, 8)
        assert np.array_equal(back.view(np.uint32), planes[c].view(np.uint32))
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = 0, 0
    p.noise, p.visible_frame_index = 1, 1
    for i in range(8):
        p.noise_lut[i] = float(lut[i])
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*chans, F32_MODULAR)
    ctx.frame_run()
    ctx.sync()
    got = ctx.read_planes()
    rnd = [oracle.noise_convolve(r) for r in oracle.noise_generate(1, 0, w, h)]
    with np.errstate(all="ignore"):
        want = oracle.noise_add(lut, 0.0, 1.0, planes, rnd)
    _hold(got, want, planes, lut_name, f"Modular frame {w}x{h}")
