"""The LF-frame preview on the device (jxlh_lf_preview, k_lf_preview.hip; run with -m gpu on an MI355X) against
tests/lf_preview_ref.py, bit for bit: sizes at which the mirror folds more than once and past 256 columns, rects, every
format and orientation, transfer functions and custom weights, host and device destinations, containment, partial
updates, a long axis, and every documented error."""
import json
import os

import numpy as np
import pytest

import lf_preview_ref as lp
import save_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUM = (0.2627, 0.678, 0.0593)
POISON = 0xA5
BACKGROUND = {sr.U8: 0xA5, sr.U16: 0xA5A5, sr.F16: 0xA5A5, sr.F32: 0xA5A5A5A5}  # the same bytes in either byte order
SLOT = 0


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


def colours(ctx, oracle, tf="srgb", param=0.0):
    """(the reference's colour tuple, the library's descriptor)"""
    from jxl_rs_amd import lib
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")))["output_stage"]
    params = oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, param if tf == "pq" else 255.0)
    return ("xyb", tf, params, param, LUM), ctx.output_desc(lib.COLOR_XYB, tf, params, param, LUM)


def slot_planes(seed, image_w, image_h):
    """a non-constant XYB image with values that leave [0, 1] after the colour stage"""
    sw, sh = lp.slot_size(image_w, image_h)
    rng = np.random.default_rng([seed, image_w, image_h])
    x = rng.uniform(-0.02, 0.02, (sh, sw)).astype(np.float32)
    y = rng.uniform(0.0, 0.9, (sh, sw)).astype(np.float32)
    b = (y + rng.uniform(-0.1, 0.1, (sh, sw))).astype(np.float32)
    y.flat[0], y.flat[-1] = 1.6, -0.3
    return [x, y, b]


def lib_desc(d):
    from jxl_rs_amd import lib
    return lib.save_desc(d["channels"], d["format"], d["bit_depth"], d["fill_opaque_alpha"], d["big_endian"],
                         d["orientation"], d["f16_clamp"])


def check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=None, device=False, pad=0, lead=16, weights8=None,
                  what="", wait=True):
    """previews `rects` (default: the whole slot) into a poisoned buffer: the rects' display pixels hold the reference's
    samples, every other byte of the buffer its poison"""
    from jxl_rs_amd import lib
    bps = sr.SAMPLE_DTYPE[d["format"]]().itemsize
    spp = 3 + (1 if d["fill_opaque_alpha"] else 0)
    ow, oh = sr.oriented_size(d["orientation"], iw, ih)
    row = ow * spp * bps
    bpr = row + pad * bps
    buf = np.full(lead + oh * bpr + lead, POISON, dtype=np.uint8)
    dev = lib.DeviceArray(buf) if device else None
    sw, sh = lp.slot_size(iw, ih)
    for r in ([(0, 0, sw, sh)] if rects is None else rects):
        st, _ = ctx.try_lf_preview(SLOT, iw, ih, lib_desc(d), colour[1], rect=r, out=dev.ptr + lead if device else buf[lead:],
                                   bytes_per_row=bpr, wait=wait)
        assert st == 0, (what, r, st)
    ctx.sync()
    if device:
        buf = dev.download(np.uint8, buf.size)
        dev.free()
    want = lp.lf_preview_ref(oracle, d, planes, iw, ih, colour[0], rects, weights8, background=BACKGROUND[d["format"]])
    body = buf[lead:lead + oh * bpr].reshape(oh, bpr)
    got = np.ascontiguousarray(body[:, :row])
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(oh, row)
    if not np.array_equal(got, wb):
        bad = np.argwhere(got != wb)
        y, x = bad[0]
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at row {y} byte {x}: got {got[y, x]} want {wb[y, x]}")
    assert np.all(body[:, row:] == POISON), f"{what}: bytes behind a row's samples were written"
    assert np.all(buf[:lead] == POISON) and np.all(buf[lead + oh * bpr:] == POISON), f"{what}: bytes around the image"


FORMATS = [
    ("u8", dict(format=sr.U8, bit_depth=8)), ("u8_5", dict(format=sr.U8, bit_depth=5)),
    ("u16_le", dict(format=sr.U16, bit_depth=16)), ("u16_be", dict(format=sr.U16, bit_depth=16, big_endian=True)),
    ("u16_10_le", dict(format=sr.U16, bit_depth=10)), ("u16_10_be", dict(format=sr.U16, bit_depth=10, big_endian=True)),
    ("f16_clamp_set", dict(format=sr.F16, f16_clamp=sr.F16_CLAMP_PQ)), ("f16_be", dict(format=sr.F16, big_endian=True)),
    ("f32_le", dict(format=sr.F32)), ("f32_be", dict(format=sr.F32, big_endian=True)),
]
LAYOUTS = [([0, 1, 2], False), ([2, 1, 0], True), ([0, 1, 2], True), ([2, 1, 0], False)]
# image sizes: slot 8 x 6; slots 1 x 1, 2 x 1 and 1 x 2, where the 5x5 window's mirror folds more than once; slot 257 x 3
SIZES = [(61, 45), (8, 8), (5, 3), (13, 7), (7, 12), (2050, 20)]


@pytest.mark.parametrize("iw,ih", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes_formats_and_layouts(ctx, oracle, iw, ih):
    planes = slot_planes(1, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    n = 0
    for name, fmt in FORMATS:  # every format with every layout
        for channels, fill in LAYOUTS:
            d = sr.desc(channels, fill_opaque_alpha=fill, **fmt)
            check_preview(ctx, oracle, d, planes, iw, ih, colour, device=n % 2 == 1, pad=(0, 3, 4)[n % 3],
                          what=f"{iw}x{ih} {name} {channels} fill={fill}")
            n += 1


@pytest.mark.parametrize("orientation", range(1, 9))
def test_orientations(ctx, oracle, orientation):
    iw, ih = 61, 45
    planes = slot_planes(2, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    cases = [(sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True, orientation=orientation), None, False),
             (sr.desc([2, 1, 0], sr.U8, orientation=orientation), [(3, 1, 4, 3)], True),
             (sr.desc([0, 1, 2], sr.F16, orientation=orientation, big_endian=True), [(3, 1, 5, 5)], False),
             (sr.desc([0, 1, 2], sr.F32, fill_opaque_alpha=True, orientation=orientation), None, True)]
    for n, (d, rects, device) in enumerate(cases):
        bps = sr.SAMPLE_DTYPE[d["format"]]().itemsize
        check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=rects, device=device, pad=(0, 1, 3)[(n + orientation) % 3],
                      lead=(16, 16 + bps)[orientation % 2], what=f"orientation {orientation} case {n}")


def test_rects(ctx, oracle):
    iw, ih = 61, 45
    sw, sh = lp.slot_size(iw, ih)
    planes = slot_planes(3, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    corners = [(0, 0, 1, 1), (sw - 1, 0, 1, 1), (0, sh - 1, 1, 1), (sw - 1, sh - 1, 1, 1)]
    for d in (sr.desc([0, 1, 2], sr.U8), sr.desc([2, 1, 0], sr.U16, fill_opaque_alpha=True, orientation=6)):
        check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=[(3, 1, sw - 3, sh - 1)], what="rect at (3, 1)")
        check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=[(3, 1, 2, 4)], device=True, what="inner rect")
        for r in corners:
            check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=[r], what=f"corner {r}")
        check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=[(2, 2, 0, 3), (2, 2, 3, 0)], what="zero-sized rects")


def test_partial_updates_assemble_to_the_whole_preview(ctx, oracle):
    iw, ih = 61, 45
    sw, sh = lp.slot_size(iw, ih)
    planes = slot_planes(4, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    four = [(0, 0, 3, 2), (3, 0, sw - 3, 2), (0, 2, 5, sh - 2), (5, 2, sw - 5, sh - 2)]
    for o in (1, 7):
        d = sr.desc([0, 1, 2], sr.U16, orientation=o)
        whole = lp.lf_preview_ref(oracle, d, planes, iw, ih, colour[0])
        assert np.array_equal(lp.lf_preview_ref(oracle, d, planes, iw, ih, colour[0], four), whole)
        check_preview(ctx, oracle, d, planes, iw, ih, colour, rects=four, wait=False, what=f"four rects, orientation {o}")


@pytest.mark.parametrize("tf,param", [("srgb", 0.0), ("pq", 10000.0), ("bt709", 0.0), ("hlg", 1.2), ("gamma", 0.45)])
def test_transfer_functions_and_custom_weights(ctx, oracle, tf, param):
    iw, ih = 61, 45
    planes = slot_planes(5, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle, tf, param)
    w8 = np.random.default_rng(6).uniform(-0.05, 0.25, 210).astype(np.float32)
    try:
        for weights in (None, w8):
            ctx.set_upsampling_weights(w8=weights)
            for d in (sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True), sr.desc([2, 1, 0], sr.F32)):
                check_preview(ctx, oracle, d, planes, iw, ih, colour, weights8=weights, what=f"{tf} custom={weights is not None}")
    finally:
        ctx.set_upsampling_weights()
    # the upsampling is the stage's: the f32 preview of a constant colour curve aside, the taps are those of jxlh_stage_upsample
    up = ctx.stage_upsample(8, planes[1])
    assert np.array_equal(up.view(np.uint32), oracle.upsample(8, planes[1]).view(np.uint32))


def test_inside_a_frame_and_after_save_lf(ctx, oracle):
    """the preview of what jxlh_frame_save_lf put into the slot, called inside the frame"""
    iw, ih = 70, 37
    sw, sh = lp.slot_size(iw, ih)
    chans = lp.modular_xyb(np.random.default_rng(7), sw, sh)
    planes = oracle.modular_xyb_to_f32(*chans, np.float32(lp.XYB_FACTORS))
    lp.render_modular_xyb(ctx, chans)
    ctx.save_lf(SLOT)
    colour = colours(ctx, oracle)
    check_preview(ctx, oracle, sr.desc([0, 1, 2], sr.U8, fill_opaque_alpha=True), planes, iw, ih, colour, what="after save_lf")


def test_long_axis(ctx, oracle):
    iw, ih = 65593, 8  # slot 8200 x 1
    planes = slot_planes(8, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    colour = colours(ctx, oracle)
    check_preview(ctx, oracle, sr.desc([0, 1, 2], sr.U8), planes, iw, ih, colour, device=True, what="65593 x 8")
    check_preview(ctx, oracle, sr.desc([0, 1, 2], sr.U8, orientation=5), planes, iw, ih, colour, what="65593 x 8 transposed")


def test_errors_write_nothing(ctx, oracle):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    INV, UNS = lib.ERR_INVALID_ARGUMENT, lib.ERR_UNSUPPORTED
    iw, ih = 61, 45
    sw, sh = lp.slot_size(iw, ih)
    planes = slot_planes(9, iw, ih)
    ctx.set_lf_frame(SLOT, *planes)
    ctx.clear_lf_frame(3)
    _, colour = colours(ctx, oracle)
    out = np.full((iw + 8, (iw + 8) * 16), POISON, np.uint8)  # room for every oriented image below
    good = lib.save_desc([0, 1, 2], lib.SAVE_U8)

    def call(desc=good, slot=SLOT, size=(iw, ih), rect=(0, 0, sw, sh), colour=colour, out=out, bpr=None):
        return ctx.try_lf_preview(slot, size[0], size[1], desc, colour, rect=rect, out=out,
                                  bytes_per_row=out.strides[0] if bpr is None else bpr)[0]
    assert call() == lib.OK
    out[:] = POISON
    assert call(rect=(2, 2, 0, 0)) == lib.OK and np.all(out == POISON)  # a zero-sized rect writes nothing
    L = ctx.L
    assert L.jxlh_lf_preview(ctx._ctx, SLOT, iw, ih, 0, 0, sw, sh, colour, None, out.ctypes.data, out.strides[0]) == INV
    assert L.jxlh_lf_preview(ctx._ctx, SLOT, iw, ih, 0, 0, sw, sh, colour, good, None, out.strides[0]) == INV
    assert call(slot=4) == INV and call(slot=3) == INV                              # no such slot, an unset slot
    assert call(size=(iw + 8, ih)) == INV and call(size=(iw, ih - 8)) == INV        # the slot is not ceil(image / 8)
    assert call(size=(0, ih)) == INV
    assert call(rect=(1, 0, sw, sh)) == INV and call(rect=(0, 2, sw, sh - 1)) == INV  # the rect leaves the slot
    assert call(rect=(0xFFFFFFFF, 0, 2, 1)) == INV
    bad = [
        lib.save_desc([0, 1], lib.SAVE_U8), lib.save_desc([0], lib.SAVE_U8), lib.save_desc([0, 1, 2, 3], lib.SAVE_U8),
        lib.save_desc([0, 2, 1], lib.SAVE_U8), lib.save_desc([0, 0, 0], lib.SAVE_U8), lib.save_desc([1, 2, 0], lib.SAVE_U8),
        lib.save_desc([0, 1, 3], lib.SAVE_U8),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=3), lib.save_desc([0, 1, 2], lib.SAVE_U8, spot=[(0, (0, 0, 0, 1))]),
        lib.save_desc([0, 1, 2], 4), lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=0),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=9), lib.save_desc([0, 1, 2], lib.SAVE_U8, bit_depth=0),
        lib.save_desc([0, 1, 2], lib.SAVE_U8, bit_depth=9), lib.save_desc([0, 1, 2], lib.SAVE_U16, bit_depth=17),
    ]
    for i, d in enumerate(bad):
        assert call(d) == INV, i
    assert call(bpr=iw * 3 - 1) == INV
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_U8, orientation=5), bpr=ih * 3 - 1) == INV  # the ORIENTED row
    d16 = lib.save_desc([0, 1, 2], lib.SAVE_U16)
    assert call(d16, bpr=iw * 6 + 1) == INV and call(d16, out=out.reshape(-1)[1:], bpr=iw * 6) == INV
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_F32), out=out.reshape(-1)[2:], bpr=iw * 12) == INV
    # where the reference shows no preview
    assert call(colour=None) == UNS
    assert call(colour=ctx.output_desc(lib.COLOR_XYB, "linear", np.zeros(16, np.float32))) == UNS
    assert call(colour=ctx.output_desc(lib.COLOR_YCBCR, "srgb")) == UNS
    assert call(colour=ctx.output_desc(lib.COLOR_NONE, "srgb")) == UNS
    wrong = ctx.output_desc(lib.COLOR_XYB, "srgb", np.zeros(16, np.float32))
    wrong.transfer = 6
    assert call(colour=wrong) == INV
    assert np.all(out == POISON)
    # f16_clamp is not read, not even checked
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_F16, f16_clamp=(0.0, 1.0))) == lib.OK
    assert call(lib.save_desc([0, 1, 2], lib.SAVE_F16, f16_clamp=(1.0, float("nan")))) == lib.OK
    # a sharded context
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            st, _ = c.try_lf_preview(SLOT, iw, ih, good, colour, out=out, bytes_per_row=out.strides[0])
            assert st == UNS
    finally:
        for c in peers:
            c.close()


def test_image_of_2_to_the_31_pixels_is_unsupported(ctx, oracle):
    """image_w * image_h >= 2^31 with a slot that exists: 2^20 x 2^11 pixels, slot 131072 x 256 (3 x 134 MB)"""
    from jxl_rs_amd import lib
    iw, ih = 1 << 20, 1 << 11
    sw, sh = lp.slot_size(iw, ih)
    dev = lib.DeviceArray(nbytes=sw * sh * 4)
    ctx.set_lf_frame(SLOT, dev.ptr, dev.ptr, dev.ptr, w=sw, h=sh, stride=sw)
    dev.free()
    _, colour = colours(ctx, oracle)
    out = np.full(64, POISON, np.uint8)
    st, _ = ctx.try_lf_preview(SLOT, iw, ih, lib.save_desc([0, 1, 2], lib.SAVE_U8), colour, rect=(0, 0, 1, 1), out=out,
                               bytes_per_row=iw * 3)
    assert st == lib.ERR_UNSUPPORTED and np.all(out == POISON)
    ctx.clear_lf_frame(SLOT)
