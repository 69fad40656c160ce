"""Extra channels by rect on the device (include/jxl_hip_extra_rects.h; run with -m gpu on an MI355X):
jxlh_frame_begin_extra_channel + jxlh_frame_set_extra_channel_rects[_async] + the k_ec_finish launches of a run or a
re-render.  The expected channel is ALWAYS the oracle's -- modular_to_f32 (+ upsample, cropped) of the plane assembled
in numpy from the rects in call order -- never the library's own whole-plane path, and every comparison is bit for bit.
Where a consumer (save, blend, patches) is checked, the other side is a fresh context that gets the final planes whole."""
import numpy as np
import pytest

from helpers import bit_equal, diff_report, run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu

POISON = 0x7fffffff
FORMATS = [(1, 0), (8, 0), (12, 0), (16, 0), (31, 0), (16, 5), (32, 8)]  # (bits, exponent bits)


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other():
    """the context of the whole-plane route"""
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames():
    """size -> (workload, the oracle's colour planes): computed once, never modified"""
    from jxl_rs_amd import synth
    from oracle.oracle import Oracle
    o = Oracle(fused=True)
    out = {}
    for w, h in ((264, 200), (301, 157), (1040, 24)):
        wl = synth.make_vardct(w, h, mix=synth.MIX_DCT8, seed=w + h, epf_iters=1)
        out[(w, h)] = (wl, run_oracle_frame(o, wl)[0])
    return out


def samples(rng, w, h, bits, exp_bits=0, finite=False):
    """i32 samples of a format.  Float formats carry +-0, subnormals, inf and NaN patterns unless `finite`: then no inf /
    NaN, and binary32 stays below 2^20 in magnitude -- the 25 taps of an upsampling must not overflow into NaNs, whose
    payload nothing specifies"""
    if not exp_bits:
        return rng.integers(0, 1 << bits, size=(h, w), dtype=np.int64).astype(np.int32)
    a = rng.integers(0, 1 << bits, size=(h, w), dtype=np.int64)
    mant = bits - exp_bits - 1
    emax = (1 << exp_bits) - 1
    if finite:
        e = (a >> mant) & emax
        cap = min(emax - 1, (1 << (exp_bits - 1)) - 1 + 19)
        a = (a & ~(emax << mant)) | (np.minimum(e, cap) << mant)
    else:
        inf = emax << mant
        special = [0, 1 << (bits - 1), 1, (1 << mant) - 1, (1 << (bits - 1)) | 3, inf, inf | 1 << (bits - 1), inf | 1,
                   inf | (1 << (mant - 1)) | 1 << (bits - 1), 1 << mant]
        a.reshape(-1)[:len(special)] = special[:a.size]
    return a.astype(np.uint32).view(np.int32)


def finished(oracle, plane, bits, exp_bits, up, res_w, res_h):
    f = oracle.modular_to_f32(plane, bits, exp_bits)
    return oracle.upsample(up, f)[:res_h, :res_w].copy() if up > 1 else f


def ragged_tiling(rng, w, h):
    """(x0, y0, w, h) rects that tile a w x h channel: a strip of full rows on top, then a ragged grid at odd origins
    with a one-sample column, a 1 x 1 rect and rects that end at the last sample"""
    top = min(h - 1, 3) if h > 1 else 0
    rects = [(0, 0, w, top)] if top else []
    xs = sorted(set([0, w] + ([1] if w > 1 else []) + [int(v) | 1 for v in rng.integers(1, w, size=min(6, w // 7 + 1)) if w > 2]))
    xs = [x for x in xs if x <= w]
    ys = sorted(set([top, h] + ([top + 1] if top + 1 < h else []) +
                    [int(v) | 1 for v in rng.integers(top + 1, h, size=min(5, h // 7 + 1)) if h - top > 2]))
    ys = [y for y in ys if top <= y <= h]
    for ya, yb in zip(ys[:-1], ys[1:]):
        for xa, xb in zip(xs[:-1], xs[1:]):
            rects.append((xa, ya, xb - xa, yb - ya))
    cover = np.zeros((h, w), np.int32)
    for x0, y0, rw, rh in rects:
        cover[y0:y0 + rh, x0:x0 + rw] += 1
    assert np.all(cover == 1) and any(r[2:] == (1, 1) for r in rects)
    return rects


def hand_over(ctx, pieces, route, stride_pad):
    """one call: pieces = (ec, x0, y0, samples) -- from a host block (blocking or _async) or a device block"""
    from jxl_rs_amd import lib
    block, descs = lib.pack_ec_rects(pieces, stride_pad=stride_pad, fill=POISON)
    if route == "device":
        dev = lib.DeviceArray(block) if block.size else lib.DeviceArray(nbytes=16)
        ctx.set_extra_channel_rects(descs, block=dev, n_samples=block.size)
        dev.free()  # the blocking form has returned: the block may be reused
    else:
        ctx.set_extra_channel_rects(descs, block=block, wait=(route == "host"))
        if route == "async":
            ctx.sync()  # (the block stays alive and untouched until here)


def assemble(ctx, rng, chans, calls=4):
    """begin every channel, then its ragged tiling, shuffled over all channels and split into `calls` calls"""
    pieces = []
    for ec, (plane, bits, eb, up) in enumerate(chans):
        h, w = plane.shape
        ctx.begin_extra_channel(ec, w, h, bits, up, exp_bits=eb)
        pieces += [(ec, x0, y0, plane[y0:y0 + rh, x0:x0 + rw]) for x0, y0, rw, rh in ragged_tiling(rng, w, h)]
    order = rng.permutation(len(pieces))
    for i, part in enumerate(np.array_split(order, calls)):
        hand_over(ctx, [pieces[j] for j in part], ("host", "device", "async")[i % 3], (0, 3, 5)[i % 3])


def check_channels(ctx, oracle, chans, res_w, res_h, what):
    for ec, (plane, bits, eb, up) in enumerate(chans):
        want = finished(oracle, plane, bits, eb, up, res_w, res_h)
        got = ctx.read_extra_channel(ec, want.shape[1], want.shape[0])
        assert bit_equal(got, want), f"{what}: extra channel {ec} ({bits}|{eb}, x{up}): {diff_report(got, want)}"


CASES = [((264, 200), (1, 2, 4, 8)), ((301, 157), (2, 8)), ((1040, 24), (1, 2))]


@pytest.mark.parametrize("size,factors", CASES, ids=["%dx%d" % c[0] for c in CASES])
def test_assembled_channels_equal_the_oracle(ctx, oracle, frames, size, factors):
    """begin, a shuffled ragged tiling over several calls (host blocking, device, host _async; padded strides with
    poisoned padding), one frame_run: every channel is the oracle's, and the colour is untouched"""
    w, h = size
    wl, colour = frames[size]
    rng = np.random.default_rng(w * 7 + h)
    upload_frame(ctx, wl)
    chans = []
    for i, up in enumerate(factors):
        bits, eb = FORMATS[(i + w) % 5]
        chans.append((samples(rng, -(-w // up), -(-h // up), bits, eb), bits, eb, up))
    assemble(ctx, rng, chans)
    ctx.frame_run()
    ctx.sync()
    check_channels(ctx, oracle, chans, w, h, f"{w}x{h}")
    got = ctx.read_planes()
    for c in range(3):
        assert bit_equal(got[c], colour[c]), c


@pytest.mark.parametrize("bits,exp_bits", FORMATS, ids=["%d_%d" % f for f in FORMATS])
def test_sample_formats(ctx, oracle, frames, bits, exp_bits):
    """every format at factor 1 (float formats with +-0, subnormals, inf, NaN) and at factors 2 and 8 (finite values)"""
    wl, _ = frames[(264, 200)]
    rng = np.random.default_rng(bits * 11 + exp_bits)
    upload_frame(ctx, wl)
    chans = [(samples(rng, 264, 200, bits, exp_bits), bits, exp_bits, 1),
             (samples(rng, 132, 100, bits, exp_bits, finite=True), bits, exp_bits, 2),
             (samples(rng, 33, 25, bits, exp_bits, finite=True), bits, exp_bits, 8)]
    assemble(ctx, rng, chans, calls=3)
    ctx.frame_run()
    ctx.sync()
    check_channels(ctx, oracle, chans, 264, 200, "formats")


def test_untouched_and_partly_covered_channels_read_zero(ctx, oracle, frames):
    wl, _ = frames[(264, 200)]
    rng = np.random.default_rng(5)
    upload_frame(ctx, wl)
    # a plane of garbage first, so that "zero" is the begin's doing
    ctx.set_extra_channel(0, samples(rng, 264, 200, 16), 16)
    ctx.set_extra_channel(1, samples(rng, 66, 50, 16), 16, 4)
    ctx.frame_run()
    upload_frame(ctx, wl)
    part = samples(rng, 132, 100, 12)
    ctx.begin_extra_channel(0, 264, 200, 16, 1)
    ctx.begin_extra_channel(1, 66, 50, 16, 4)
    ctx.begin_extra_channel(2, 132, 100, 12, 2)
    plane = np.zeros((100, 132), np.int32)
    for x0, y0, rw, rh in ((0, 0, 5, 7), (61, 13, 9, 8), (131, 99, 1, 1)):
        plane[y0:y0 + rh, x0:x0 + rw] = part[y0:y0 + rh, x0:x0 + rw]
        ctx.set_extra_channel_rects([(2, x0, y0, part[y0:y0 + rh, x0:x0 + rw])])
    ctx.frame_run()
    ctx.sync()
    check_channels(ctx, oracle, [(np.zeros((200, 264), np.int32), 16, 0, 1), (np.zeros((50, 66), np.int32), 16, 0, 4),
                                 (plane, 12, 0, 2)], 264, 200, "zero planes")


def test_modular_frame_band(ctx, oracle):
    """a Modular frame of 264 x 200, run as a band, with rect-fed channels at factor 1 and 4"""
    rng = np.random.default_rng(17)
    w, h = 264, 200
    p = ctx.default_params(w, h)
    p.gab, p.epf_iters = 0, 0
    col = [samples(rng, w, h, 8) for _ in range(3)]
    ctx.modular_frame_begin(p)
    ctx.set_modular_channels(*col, 8)
    chans = [(samples(rng, w, h, 16), 16, 0, 1), (samples(rng, 66, 50, 8), 8, 0, 4)]
    assemble(ctx, rng, chans)
    ctx.frame_run(0, 1)
    ctx.sync()
    check_channels(ctx, oracle, chans, w, h, "modular frame")
    got = ctx.read_planes()
    for c in range(3):
        assert bit_equal(got[c], oracle.modular_to_f32(col[c], 8)), c


# ---------------------------------------------------------------- incremental updates
# 264 x 200 has two groups (columns 0..255, 256..263).  In source samples of the factor-1 channel: a corner, a rect
# across the tile seams (x = 64, y = 16), and one next to the group boundary x = 256; the factor-2 channel gets the
# same three at half the coordinates (its seams are at x = 64, y = 16 of ITS samples)
UPDATES = {1: [(0, 0, 3, 2), (60, 13, 9, 7), (250, 90, 9, 5)], 2: [(129, 97, 3, 3), (62, 14, 5, 4), (124, 40, 6, 7)]}


@pytest.mark.parametrize("start", ["begin", "whole"])
def test_rect_updates_then_rerender(ctx, oracle, frames, start):
    from jxl_rs_amd import JxlHipError, lib
    w, h = 264, 200
    wl, colour = frames[(w, h)]
    rng = np.random.default_rng(23)
    upload_frame(ctx, wl)
    chans = [(samples(rng, w, h, 16), 16, 0, 1), (samples(rng, 132, 100, 8), 8, 0, 2)]
    if start == "begin":
        assemble(ctx, rng, chans)
    else:
        for ec, (plane, bits, eb, up) in enumerate(chans):
            ctx.set_extra_channel(ec, plane, bits, up)
    ctx.frame_run()
    ctx.sync()
    first = [ctx.read_extra_channel(ec, w, h) for ec in range(2)]
    check_channels(ctx, oracle, chans, w, h, "first run")
    new, pieces = [], []
    for ec, (plane, bits, eb, up) in enumerate(chans):
        q = plane.copy()
        for x0, y0, rw, rh in UPDATES[up]:
            q[y0:y0 + rh, x0:x0 + rw] = samples(rng, rw, rh, bits) ^ 1
            pieces.append((ec, x0, y0, q[y0:y0 + rh, x0:x0 + rw]))
        new.append((q, bits, eb, up))
    ctx.set_extra_channel_rects(pieces, stride_pad=2)
    # handed over, not rendered: the read-out and a save that names the channel refuse
    with pytest.raises(JxlHipError) as e:
        ctx.read_extra_channel(0, w, h)
    assert e.value.status == lib.ERR_BAD_STATE
    assert ctx.try_frame_save(lib.save_desc([0, 1, 2, 3], lib.SAVE_U8))[0] == lib.ERR_BAD_STATE
    assert ctx.try_frame_save(lib.save_desc([0, 1, 2], lib.SAVE_U8, premultiply=4))[0] == lib.ERR_BAD_STATE
    ctx.rerender_groups([1])
    ctx.sync()
    check_channels(ctx, oracle, new, w, h, "after the re-render")
    for ec, (plane, bits, eb, up) in enumerate(new):
        got = ctx.read_extra_channel(ec, w, h)
        rects = lib.extra_channel_changed_rects(plane.shape[1], plane.shape[0], up, w, h, UPDATES[up])
        outside = np.ones((h, w), bool)
        for x0, y0, rw, rh in rects.tolist():
            outside[y0:y0 + rh, x0:x0 + rw] = False
        assert np.array_equal(got.view(np.uint32)[outside], first[ec].view(np.uint32)[outside]), ec
        assert not np.array_equal(got.view(np.uint32), first[ec].view(np.uint32)), ec
    got = ctx.read_planes()
    for c in range(3):
        assert bit_equal(got[c], colour[c]), c


def test_launches(ctx, frames):
    """what a re-render issues: k_ec_finish alone for a rect-fed channel, the old labels for a channel that never saw
    a rect call, nothing when nothing is new"""
    wl, _ = frames[(264, 200)]
    rng = np.random.default_rng(29)
    labels = ("k_ec_finish", "k_modular_to_f32", "k_upsample")

    def seen():
        ctx.sync()
        t = ctx.kernel_times()
        ctx.kernel_timing_reset()
        return {k for k in labels + ("k_ec_scatter",) if k in t and t[k][1] > 0}
    upload_frame(ctx, wl)
    ctx.begin_extra_channel(0, 264, 200, 8, 1)
    ctx.begin_extra_channel(1, 132, 100, 8, 2)
    ctx.frame_run()
    ctx.kernel_timing(True)
    try:
        ctx.kernel_timing_reset()
        ctx.set_extra_channel_rects([(0, 5, 5, samples(rng, 9, 9, 8)), (1, 60, 10, samples(rng, 9, 9, 8))])
        assert seen() == {"k_ec_scatter"}
        ctx.rerender_groups([0])
        assert seen() == {"k_ec_finish"}
        ctx.rerender_groups([0])
        assert seen() == set()
        ctx.frame_run()  # a whole run: nothing of a rect-fed channel is new either
        assert seen() == set()
        # a channel that never saw a rect call: the whole-plane launches, as ever
        upload_frame(ctx, wl)
        ctx.set_extra_channel(0, samples(rng, 132, 100, 8), 8, 2)
        ctx.frame_run()
        assert seen() == {"k_modular_to_f32", "k_upsample"}
        ctx.set_extra_channel(0, samples(rng, 132, 100, 8), 8, 2)
        ctx.rerender_groups([0])
        assert seen() == {"k_modular_to_f32", "k_upsample"}
    finally:
        ctx.kernel_timing(False)


# ---------------------------------------------------------------- consumers
def xyb_colour(c, oracle):
    from jxl_rs_amd import lib
    from test_gpu_save import LUM, xyb_params
    return c.output_desc(lib.COLOR_XYB, "srgb", xyb_params(oracle), 0.0, LUM)


@pytest.mark.parametrize("up", [1, 2])
def test_save_and_save_rects_read_the_rect_fed_alpha(ctx, other, oracle, frames, up):
    """RGBA8 saves (premultiplied and not, orientations 1 and 6) of a frame whose alpha arrived by rects, and the
    repaint of changed_rects U extra_channel_changed_rects after an update: a fresh context that got the planes whole"""
    from jxl_rs_amd import lib
    w, h = 264, 200
    wl, _ = frames[(w, h)]
    rng = np.random.default_rng(31 + up)
    aw, ah = w // up, h // up
    alpha = samples(rng, aw, ah, 8)
    descs = [lib.save_desc([0, 1, 2, 3], lib.SAVE_U8, orientation=o, premultiply=pm) for o in (1, 6) for pm in (None, 3)]
    upload_frame(ctx, wl)
    assemble(ctx, rng, [(alpha, 8, 0, up)], calls=2)
    ctx.frame_run()
    upload_frame(other, wl)
    other.set_extra_channel(0, alpha, 8, up)
    other.frame_run()
    held = []
    for d in descs:
        a = ctx.frame_save(d, xyb_colour(ctx, oracle))
        assert np.array_equal(a, other.frame_save(d, xyb_colour(other, oracle))), (d.orientation, d.premultiply)
        held.append(a)
    # group 1 arrives again with its alpha samples (and one rect elsewhere)
    upd = [(250 // up, 20 // up, aw - 250 // up, 60 // up), (3, 5, 9, 4)]
    new = alpha.copy()
    for x0, y0, rw, rh in upd:
        new[y0:y0 + rh, x0:x0 + rw] = samples(rng, rw, rh, 8) ^ 1
    ctx.submit_group(1, wl.coeffs[1])
    ctx.slot_wait(0)
    ctx.set_extra_channel_rects([(0, x0, y0, new[y0:y0 + rh, x0:x0 + rw]) for x0, y0, rw, rh in upd])
    ctx.rerender_groups([1])
    rects = np.concatenate([ctx.changed_rects([1]), lib.extra_channel_changed_rects(aw, ah, up, w, h, upd)])
    other.set_extra_channel(0, new, 8, up)
    other.frame_run()
    for d, a in zip(descs, held):
        before = a.copy()
        ctx.frame_save_rects(d, rects, xyb_colour(ctx, oracle), out=a)
        assert not np.array_equal(a, before)
        assert np.array_equal(a, other.frame_save(d, xyb_colour(other, oracle))), (d.orientation, d.premultiply)


def test_blend_reads_the_rect_fed_alpha(ctx, other, oracle, frames):
    from jxl_rs_amd import lib
    w, h = 264, 200
    wl, _ = frames[(w, h)]
    rng = np.random.default_rng(37)
    alpha = samples(rng, w, h, 16)
    canvas = [rng.uniform(-0.5, 1.5, (240, 300)).astype(np.float32) for _ in range(4)]
    bd = lib.blend_desc(-17, 9, 300, 240, (lib.BLEND_BLEND, 0, 1, 0), [(lib.BLEND_BLEND, 0, 0, 0)], [lib.EC_ALPHA])
    got = []
    for c in (ctx, other):
        c.set_reference(0, canvas)
        upload_frame(c, wl)
        if c is ctx:
            assemble(c, rng, [(alpha, 16, 0, 1)], calls=3)
        else:
            c.set_extra_channel(0, alpha, 16)
        c.frame_run()
        c.blend(bd, xyb_colour(c, oracle))
        got.append(c.read_planes() + [c.read_extra_channel(0, 300, 240)])
        c.clear_reference(0)
    for a, b in zip(*got):
        assert bit_equal(a, b)
    assert not bit_equal(got[0][3], canvas[3])


def test_patches_read_the_rect_fed_channel(ctx, other, frames):
    """a frame with a patch dictionary that has one extra channel, whole run: the patched channel is the whole-plane
    route's"""
    from jxl_rs_amd import lib
    w, h = 264, 200
    wl, _ = frames[(w, h)]
    rng = np.random.default_rng(41)
    alpha = samples(rng, w, h, 16)
    ref = [rng.uniform(-0.5, 1.5, (64, 96)).astype(np.float32) for _ in range(4)]
    patches, blendings = [], []
    for _ in range(40):
        xs, ys = int(rng.integers(8, 48)), int(rng.integers(8, 40))
        patches.append((int(rng.integers(0, w - xs + 1)), int(rng.integers(0, h - ys + 1)), 0,
                        int(rng.integers(0, 96 - xs + 1)), int(rng.integers(0, 64 - ys + 1)), xs, ys))
        blendings += [(int(rng.integers(0, 8)), 0, bool(rng.integers(0, 2))) for _ in range(2)]
    got = []
    for c in (ctx, other):
        c.set_reference(0, ref)
        upload_frame(c, wl)
        if c is ctx:
            assemble(c, rng, [(alpha, 16, 0, 1)], calls=3)
        else:
            c.set_extra_channel(0, alpha, 16)
        c.set_patches(patches, blendings, [lib.EC_ALPHA])
        c.frame_run()
        c.sync()
        got.append(c.read_planes() + [c.read_extra_channel(0, w, h)])
        c.clear_reference(0)
    for a, b in zip(*got):
        assert bit_equal(a, b)
    plain = np.float32(alpha) * np.float32(1.0 / 65535.0)
    assert not bit_equal(got[0][3], plain)  # the patches did reach the channel


# ---------------------------------------------------------------- states and arguments
def test_refusals_launch_nothing_and_change_nothing(ctx, oracle, frames):
    import jxl_rs_amd
    from jxl_rs_amd import lib
    INV, BAD = lib.ERR_INVALID_ARGUMENT, lib.ERR_BAD_STATE
    wl, _ = frames[(264, 200)]
    rng = np.random.default_rng(43)
    plane = samples(rng, 66, 50, 12)
    fresh = jxl_rs_amd.Context(0, 1)
    try:  # outside a frame
        block, descs = lib.pack_ec_rects([(0, 0, 0, plane[:2, :2])])
        assert fresh.try_set_extra_channel_rects(block, descs) == (BAD, None)
        assert fresh.L.jxlh_frame_begin_extra_channel(fresh._ctx, 0, 4, 4, 8, 1) == BAD
    finally:
        fresh.close()
    upload_frame(ctx, wl)
    L = ctx.L
    for args in ((8, 4, 4, 8, 1), (0, 0, 4, 8, 1), (0, 4, 0, 8, 1), (0, 4, 4, 0, 1), (0, 4, 4, 32, 1), (0, 4, 4, 8, 3),
                 (0, 4, 4, 8, 16), (0, 4, 4, 8, 0), (0, 4, 4, 16 | 9 << 8, 1)):
        assert L.jxlh_frame_begin_extra_channel(ctx._ctx, *args) == INV, args
    assert L.jxlh_frame_begin_extra_channel(ctx._ctx, 0, 1 << 16, 1 << 15, 8, 1) == lib.ERR_UNSUPPORTED
    ctx.begin_extra_channel(0, 66, 50, 12, 4)
    assert L.jxlh_frame_begin_extra_channel(ctx._ctx, 0, 66, 50, 12, 4) == BAD      # begun already
    ctx.set_extra_channel(1, plane, 12, 4)
    assert L.jxlh_frame_begin_extra_channel(ctx._ctx, 1, 66, 50, 12, 4) == BAD      # handed over whole already
    ctx.set_extra_channel_rects([(0, 0, 0, plane)])
    ctx.frame_run()
    ctx.sync()
    before = [ctx.read_extra_channel(ec, 264, 200) for ec in (0, 1)]
    ctx.kernel_timing(True)
    ctx.kernel_timing_reset()
    try:
        blk = np.full(4096, POISON, np.int32)

        def call(rows, n_samples=blk.size, block=blk, wait=True):
            d = np.zeros(len(rows), dtype=lib.EC_RECT_DTYPE)
            for i, r in enumerate(rows):
                d[i] = r
            return ctx.try_set_extra_channel_rects(block, d, n_samples=n_samples, wait=wait)
        good = (0, 1, 1, 4, 4, 0, 4)  # (ec, x0, y0, w, h, offset, stride)
        for wait in (True, False):
            assert call([good, (8, 0, 0, 1, 1, 0, 1)], wait=wait) == (INV, 1)            # no such channel
            assert call([(8, 0, 0, 0, 0, 0, 0)], wait=wait) == (INV, 0)                   # ... on an empty rect too
            assert call([good, good, (2, 0, 0, 1, 1, 0, 1)], wait=wait) == (BAD, 2)       # channel 2 is not set
            assert call([(0, 0, 0, 4, 4, 0, 3)], wait=wait) == (INV, 0)                   # stride < w
            assert call([(0, 63, 0, 4, 1, 0, 4)], wait=wait) == (INV, 0)                  # leaves the channel
            assert call([(0, 0, 47, 1, 4, 0, 1)], wait=wait) == (INV, 0)
            assert call([(0, 0xffffffff, 0, 2, 1, 0, 2)], wait=wait) == (INV, 0)          # x0 + w wraps 32 bits
            assert call([(0, 0, 0xffffffff, 1, 2, 0, 1)], wait=wait) == (INV, 0)
            assert call([(0, 0, 0, 4, 4, blk.size - 15, 4)], wait=wait) == (INV, 0)       # one sample beyond n_samples
            assert call([(0, 0, 0, 4, 4, 0, 1366)], wait=wait) == (INV, 0)                # ... by its stride
            assert call([(0, 0, 0, 4, 4, 0xffffffffffffffff, 4)], wait=wait) == (INV, 0)  # offset + extent wraps 64 bits
            assert call([(0, 0, 0, 4, 4, 0, 4)], n_samples=0xffffffffffffffff, block=None, wait=wait)[0] == INV  # no block
            assert call([good] * (lib.MAX_EC_RECTS + 1), wait=wait)[0] == INV
            assert ctx.try_set_extra_channel_rects(blk, None, n=1, wait=wait)[0] == INV   # rects == NULL with n > 0
        assert L.jxlh_frame_set_extra_channel_rects(None, None, 0, None, 0, None) == INV
        assert L.jxlh_frame_set_extra_channel_rects_async(None, None, 0, None, 0, None) == INV
        # accepted with nothing to do: n == 0, and rects that are all empty (wherever they start)
        assert ctx.try_set_extra_channel_rects(None, None, n=0)[0] == lib.OK
        assert call([(0, 500, 500, 0, 3, 1 << 40, 0), (1, 0, 0, 3, 0, 0, 0)]) == (lib.OK, None)
        ctx.sync()
        assert "k_ec_scatter" not in ctx.kernel_times()
    finally:
        ctx.kernel_timing(False)
    # nothing changed: the channels are still rendered, and read back as they did
    for ec in (0, 1):
        assert bit_equal(ctx.read_extra_channel(ec, 264, 200), before[ec]), ec
    # accepted: rects that end at the last sample of the block and of the channel; the last stride is not needed
    assert call([(0, 62, 46, 4, 4, blk.size - 16, 4), (1, 65, 49, 1, 1, 4095, 0xffffffff)]) == (lib.OK, None)
    want = plane.copy()
    want[46:50, 62:66] = POISON
    ctx.frame_run()
    got = ctx.read_extra_channel(0, 264, 200)
    assert bit_equal(got, finished(oracle, want, 12, 0, 4, 264, 200))


def test_sharded_context_is_unsupported():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    wl = synth.make_vardct(300, 600, mix=synth.MIX_D1, seed=11, epf_iters=2)
    peers = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    try:
        lib.comm_init_local(peers)
        for c in peers:
            upload_frame(c, wl)
            assert c.L.jxlh_frame_begin_extra_channel(c._ctx, 0, 8, 8, 8, 1) == lib.ERR_UNSUPPORTED
            c.set_extra_channel(0, np.zeros((8, 8), np.int32), 8)
            block, descs = lib.pack_ec_rects([(0, 0, 0, np.ones((2, 2), np.int32))])
            for wait in (True, False):
                assert c.try_set_extra_channel_rects(block, descs, wait=wait)[0] == lib.ERR_UNSUPPORTED
    finally:
        for c in peers:
            c.close()


def test_frame_begin_clears_the_rect_state(ctx, oracle, frames):
    from jxl_rs_amd import lib
    wl, colour = frames[(264, 200)]
    rng = np.random.default_rng(47)

    def plain():
        upload_frame(ctx, wl)
        ctx.frame_run()
        ctx.sync()
        return ctx.read_planes()
    a = plain()
    upload_frame(ctx, wl)
    assemble(ctx, rng, [(samples(rng, 132, 100, 8), 8, 0, 2)], calls=2)
    ctx.frame_run()
    b = plain()
    for c in range(3):
        assert bit_equal(a[c], colour[c]) and bit_equal(b[c], colour[c]), c
    # the channel of the frame before is gone: not set, so a rect for it is a state error, and a begin is fine again
    block, descs = lib.pack_ec_rects([(0, 0, 0, np.ones((2, 2), np.int32))])
    assert ctx.try_set_extra_channel_rects(block, descs) == (lib.ERR_BAD_STATE, 0)
    ctx.begin_extra_channel(0, 33, 25, 8, 8)
    ctx.frame_run()
    check_channels(ctx, oracle, [(np.zeros((25, 33), np.int32), 8, 0, 8)], 264, 200, "a new frame's channel")
