"""The integer read-outs (jxlh_frame_read_rgb8/16, _ycbcr_rgb8/16, jxlh_frame_read_output) across destination layouts:
which stores a launch issues depends on the destination's alignment and pitch, and the other read-out tests only use
host destinations with tight rows.  Every byte is held to the oracle, and every byte the call does not own (row padding,
rows outside a band, the bytes in front of and behind the image) to the poison the buffer was filled with."""
import ctypes as C

import numpy as np
import pytest

from helpers import DeviceArray, run_oracle_frame, upload_frame

pytestmark = pytest.mark.gpu

POISON = 0xA5
TAIL = 32  # bytes behind the last row that must stay poison
LUM = (0.2627, 0.678, 0.0593)
PQ_TARGET = 4000.0
SUB420 = (1, 0, 1)

# name -> (w, h, band): 9 x 9 and 67 x 5 end every row in a partial lane (4 pixels per lane); 1030 x 3 crosses the
# 1024-pixel workgroup of the row kernel; the 4:2:0 frame has nothing between the transforms and the output, so its
# YCbCr read-out runs the chroma-fused kernel (the band starts on an odd row: the vertical neighbour is the row below)
FRAMES = {"9x9": (9, 9, (3, 6)), "67x5": (67, 5, (1, 4)), "1030x3": (1030, 3, (1, 2)), "420_34x18": (34, 18, (5, 12))}


@pytest.fixture(scope="module")
def ctx():
    import jxl_rs_amd
    c = jxl_rs_amd.Context(0, 1)
    yield c
    c.close()


_frames = {}


def _frame(oracle, name):
    """the workload and the oracle's planes, once per module"""
    if name not in _frames:
        from jxl_rs_amd import synth
        w, h, _ = FRAMES[name]
        if name.startswith("420"):
            wl = synth.make_vardct(w, h, mix=synth.MIX_8X8, seed=w ^ h, epf_iters=0, gab=False, lf_smoothing=False,
                                   hshift=SUB420, vshift=SUB420)
            wl.lf_q[0] = wl.lf_q[0] // 3  # keep Y + 128/255 inside [0, 1] so the clamps are not the whole story
        else:
            wl = synth.make_vardct(w, h, mix=synth.MIX_D1, seed=w * 7 + h, epf_iters=2)
        planes, _ = run_oracle_frame(oracle, wl)
        _frames[name] = (wl, [np.ascontiguousarray(p) for p in planes], {})
    return _frames[name]


def _xyb_params(oracle, kat, intensity_target):
    k = kat["output_stage"]
    return oracle.xyb_params(k["opsin_inverse_matrix"], [k["opsin_bias"]] * 3, intensity_target)


def _want(oracle, kat, name, mode, bits, ch):
    """the oracle's image [h, w, ch] of frame `name`, once per (mode, bits, channels)"""
    _, planes, cache = _frame(oracle, name)
    key = (mode, bits, ch)
    if key not in cache:
        w, h, _ = FRAMES[name]
        if mode == "srgb":
            f = oracle.xyb_to_rgb8 if bits == 8 else oracle.xyb_to_rgb16
            cache[key] = f(_xyb_params(oracle, kat, 255.0), planes, w, h, ch)
        elif mode == "pq":
            cache[key] = oracle.xyb_to_rgb_tf(_xyb_params(oracle, kat, PQ_TARGET), "pq", planes, w, h, ch, bits, PQ_TARGET, LUM)
        elif mode == "ycbcr":
            f = oracle.ycbcr_to_rgb8 if bits == 8 else oracle.ycbcr_to_rgb16
            cache[key] = f(planes, w, h, ch)
        else:  # COLOR_NONE: the planes are taken as R, G, B -- the integer conversion alone
            out = np.full((h, w, ch), 255 if bits == 8 else 65535, dtype=np.uint8 if bits == 8 else np.uint16)
            for c in range(3):
                if bits == 16:
                    out[:, :, c] = np.rint(np.clip(planes[c][:h, :w], 0, 1) * np.float32(65535)).astype(np.uint16)
                else:  # the dithered conversion, sample by sample
                    for y in range(h):
                        for x in range(w):
                            out[y, x, c] = oracle.f32_to_u8(float(planes[c][y, x]), x, y, c)
            cache[key] = out
    return cache[key]


def _render(ctx, wl):
    upload_frame(ctx, wl)
    ctx.frame_run()
    ctx.sync()


def _read(ctx, oracle, kat, mode, bits, ch, y0, y1, ptr, pitch):
    """one read-out of rows [y0, y1) into the memory at `ptr` (which is row y0), through the entry point of `mode`"""
    from jxl_rs_amd import lib
    L, out = ctx.L, C.c_void_p(ptr)
    if mode == "srgb":
        pr = np.ascontiguousarray(_xyb_params(oracle, kat, 255.0), dtype=np.float32)
        f = L.jxlh_frame_read_rgb8 if bits == 8 else L.jxlh_frame_read_rgb16
        st = f(ctx._ctx, pr.ctypes.data_as(C.c_void_p), ch, y0, y1, out, pitch)
    elif mode == "ycbcr":
        f = L.jxlh_frame_read_ycbcr_rgb8 if bits == 8 else L.jxlh_frame_read_ycbcr_rgb16
        st = f(ctx._ctx, ch, y0, y1, out, pitch)
    else:
        if mode == "pq":
            d = ctx.output_desc(lib.COLOR_XYB, "pq", _xyb_params(oracle, kat, PQ_TARGET), PQ_TARGET, LUM, bits, ch)
        else:
            d = ctx.output_desc(lib.COLOR_NONE, "linear", None, 0.0, LUM, bits, ch)
        st = L.jxlh_frame_read_output(ctx._ctx, C.byref(d), y0, y1, out, pitch)
    ctx._chk(st, f"read-out {mode} {bits} bit x{ch}")
    ctx.sync()  # (a device destination is only queued)


def _check(buf, off, pitch, want_rows, tag):
    """buf: the whole poisoned buffer after the call, as bytes; the rows of want_rows sit from `off` on at `pitch`"""
    rows = np.ascontiguousarray(want_rows).view(np.uint8).reshape(want_rows.shape[0], -1)
    n, row_bytes = rows.shape
    expect = np.full(buf.size, POISON, dtype=np.uint8)
    for r in range(n):
        expect[off + r * pitch: off + r * pitch + row_bytes] = rows[r]
    bad = np.flatnonzero(buf != expect)
    if bad.size:
        b = int(bad[0])
        r, col = divmod(b - off, pitch)
        where = f"row {r} byte {col} of {row_bytes}" if 0 <= b - off and r < n else "outside the rows"
        raise AssertionError(f"{tag}: {bad.size} bytes differ, first at byte {b} ({where}): got {buf[b]:#x}, "
                             f"want {expect[b]:#x}")


def _layouts(ctx, oracle, kat, name, mode, bits, ch):
    """the five destination layouts of one (mode, bits, channels) on the frame the context holds"""
    w, h, (b0, b1) = FRAMES[name]
    want = _want(oracle, kat, name, mode, bits, ch)
    bps = bits // 8
    row = w * ch * bps
    padded = row + (5 if bits == 8 else 6)
    lead = bps  # the device destination starts 1 byte (8 bit) / 2 bytes (16 bit) into its allocation
    tag = f"{name} {mode} {bits} bit x{ch}"

    def host(pitch, y0, y1, off, size):
        buf = np.full(size, POISON, dtype=np.uint8)
        _read(ctx, oracle, kat, mode, bits, ch, y0, y1, buf.ctypes.data + off, pitch)
        return buf

    def device(pitch, off, size):
        d = DeviceArray(np.full(size, POISON, dtype=np.uint8))
        try:
            _read(ctx, oracle, kat, mode, bits, ch, 0, h, d.ptr + off, pitch)
            return d.download(np.uint8, size)
        finally:
            d.free()

    _check(host(row, 0, h, 0, row * h + TAIL), 0, row, want, tag + ", host, tight")
    _check(host(padded, 0, h, 0, padded * h + TAIL), 0, padded, want, tag + ", host, padded")
    _check(device(row, 0, row * h + TAIL), 0, row, want, tag + ", device, tight")
    _check(device(padded, lead, lead + padded * h + TAIL), lead, padded, want, tag + ", device, padded + offset")
    # a band strictly inside the frame, into the whole image: `out` is the band's first row
    _check(host(row, b0, b1, b0 * row, row * h + TAIL), b0 * row, row, want[b0:b1], tag + f", host, rows {b0}:{b1}")


def _launches(ctx, label):
    return ctx.kernel_times().get(label, (0.0, 0))[1]


@pytest.mark.parametrize("name", ["9x9", "67x5", "1030x3"])
def test_readout_layouts(ctx, oracle, kat, name):
    wl, _, _ = _frame(oracle, name)
    _render(ctx, wl)
    for mode in ("srgb", "pq", "none", "ycbcr"):
        for bits in (8, 16):
            for ch in (3, 4):
                _layouts(ctx, oracle, kat, name, mode, bits, ch)


def test_readout_layouts_subsampled(ctx, oracle, kat):
    """a 4:2:0 frame without filters: the YCbCr read-outs straight from the sub-sampled channels, then -- once
    read_planes() has built the full-resolution chroma -- the same layouts from the planes"""
    name = "420_34x18"
    wl, planes, _ = _frame(oracle, name)
    _render(ctx, wl)
    ctx.kernel_timing_reset()
    ctx.kernel_timing(True)
    try:
        for bits in (8, 16):
            for ch in (3, 4):
                _layouts(ctx, oracle, kat, name, "ycbcr", bits, ch)
        ctx.sync()
        # the timer labels of the read-outs say which path ran
        assert _launches(ctx, "k_ycbcr_sub_to_rgb") == 20 and _launches(ctx, "k_xyb_to_rgb8") == 0
        got = ctx.read_planes()
        for c in range(3):
            assert np.array_equal(got[c].view(np.uint32), planes[c][:got[c].shape[0], :got[c].shape[1]].view(np.uint32))
        for mode in ("ycbcr", "none"):
            for bits in (8, 16):
                for ch in (3, 4):
                    _layouts(ctx, oracle, kat, name, mode, bits, ch)
        ctx.sync()
        assert _launches(ctx, "k_ycbcr_sub_to_rgb") == 20
        assert _launches(ctx, "k_xyb_to_rgb8") == 20 and _launches(ctx, "k_xyb_to_rgb16") == 20
    finally:
        ctx.kernel_timing(False)
