"""ctypes binding of the C ABI in include/jxl_hip.h (libjxl_hip.so, built in-tree by
jxl_rs_amd/csrc/Makefile).  This is the same surface a Rust `extern "C"` block binds
(INTEGRATION.md); Python is only the test / bench harness language here.

There is no fallback: if the shared library is missing, importing this module raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# JXLH_LIBRARY: developer override used to A/B kernel build variants (tools/build_variant.sh)
LIB_PATH = os.environ.get("JXLH_LIBRARY") or os.path.join(_HERE, "libjxl_hip.so")

# The constants (JXLH_X -> X), the structs (jxlh_frame_params -> FrameParams), ABI_SYMBOLS / DEV_SYMBOLS and every entry
# point's signature come from the headers by way of tools/gen_py_binding.py; below is only what the headers do not say.
from . import _abi  # noqa: E402
from ._abi import *  # noqa: E402,F401,F403

MODULAR_XYB = 1 << 16  # jxlh_frame_set_modular_channels: sample_format | MODULAR_XYB (a parenthesised #define)
PATCH_AWA_ABOVE, PATCH_AWA_BELOW = PATCH_ALPHA_WEIGHTED_ADD_ABOVE, PATCH_ALPHA_WEIGHTED_ADD_BELOW
TF = {"linear": TF_LINEAR, "srgb": TF_SRGB, "bt709": TF_BT709, "pq": TF_PQ, "hlg": TF_HLG, "gamma": TF_GAMMA}


def blend_desc(x0, y0, image_w, image_h, color, ec=(), ec_flags=(), num_ec=None):
    """jxlh_blend_desc from (mode, alpha_channel, clamp, source) tuples: `color`, and one per extra channel in `ec`"""
    d = BlendDesc()
    d.x0, d.y0, d.image_w, d.image_h = int(x0), int(y0), int(image_w), int(image_h)
    d.color = BlendingInfo(*[int(v) for v in color])
    d.num_ec = len(ec) if num_ec is None else int(num_ec)
    for i, b in enumerate(list(ec)[:8]):
        d.ec[i] = BlendingInfo(*[int(v) for v in b])
    for i, f in enumerate(list(ec_flags)[:8]):
        d.ec_flags[i] = int(f)
    return d


SAVE_SAMPLE_BYTES = {SAVE_U8: 1, SAVE_U16: 2, SAVE_F16: 2, SAVE_F32: 4}  # the save tail (jxlh_frame_save)


def save_tile_layout(pixel_bytes):
    """jxlh_save_tile_layout (jxl_hip_dev.h, host only): (columns, rows) in source pixels of the transposing save kernel's
    tile for a pixel of that many bytes -- what sizes around a tile edge mean in tests"""
    c, r = C.c_uint32(), C.c_uint32()
    st = load().jxlh_save_tile_layout(C.c_uint32(pixel_bytes), C.byref(c), C.byref(r))
    if st != OK:
        raise JxlHipError(st, "jxlh_save_tile_layout")
    return c.value, r.value


def _rect_array(rects):
    """rects as the C ABI takes them: (x0, y0, w, h) rows as a contiguous uint32 array [n, 4] (the layout of jxlh_rect)"""
    r = np.ascontiguousarray(rects, dtype=np.uint32).reshape(-1, 4)
    return r, len(r)


def try_changed_rects(params, group_ids, cap=None):
    """jxlh_changed_rects (host only), returning (status, rects [n, 4] as (x0, y0, w, h) or None, n needed).  cap: room
    offered (None: as many as needed -- asked for first, as a C caller would)"""
    ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
    L, n = load(), C.c_uint32(0)
    if cap is None:
        st = L.jxlh_changed_rects(C.byref(params), _addr(ids), len(ids), None, 0, C.byref(n))
        if st != OK and n.value == 0:
            return st, None, 0
        cap = n.value
    out = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
    st = L.jxlh_changed_rects(C.byref(params), _addr(ids), len(ids), _addr(out) if cap else None, int(cap), C.byref(n))
    return st, (out[:n.value].copy() if st == OK else None), n.value


def changed_rects(params, group_ids):
    """the rectangles of the frame's result that re-rendering `group_ids` can change, [n, 4] rows (x0, y0, w, h)"""
    st, rects, _ = try_changed_rects(params, group_ids)
    if st != OK:
        raise JxlHipError(st, "jxlh_changed_rects")
    return rects


def try_repaint_changed_rects(params, group_ids, cap=None):
    """jxlh_repaint_changed_rects (host only), returning (status, rects [n, 4] as (x0, y0, w, h) or None, n needed), as
    try_changed_rects does"""
    ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
    L, n = load(), C.c_uint32(0)
    if cap is None:
        st = L.jxlh_repaint_changed_rects(C.byref(params), _addr(ids), len(ids), None, 0, C.byref(n))
        if st != OK and n.value == 0:
            return st, None, 0
        cap = n.value
    out = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
    st = L.jxlh_repaint_changed_rects(C.byref(params), _addr(ids), len(ids), _addr(out) if cap else None, int(cap),
                                      C.byref(n))
    return st, (out[:n.value].copy() if st == OK else None), n.value


def repaint_changed_rects(params, group_ids):
    """the rectangles of the frame's result (upsampled size) that repainting `group_ids` can change, on any kind of
    frame: [n, 4] rows (x0, y0, w, h)"""
    st, rects, _ = try_repaint_changed_rects(params, group_ids)
    if st != OK:
        raise JxlHipError(st, "jxlh_repaint_changed_rects")
    return rects


def try_blend_image_rects(desc, frame_w, frame_h, rects, cap=None):
    """jxlh_blend_image_rects (host only), returning (status, rects [n, 4] as (x0, y0, w, h) or None, n needed).  rects:
    rows (x0, y0, w, h) of the frame_w x frame_h result; cap: room offered (None: as many as needed -- asked for first)"""
    r, n_in = _rect_array(rects)
    L, n = load(), C.c_uint32(0)
    src = _addr(r) if n_in else None
    if cap is None:
        st = L.jxlh_blend_image_rects(C.byref(desc), int(frame_w), int(frame_h), src, n_in, None, 0, C.byref(n))
        if st != OK and n.value == 0:
            return st, None, 0
        cap = n.value
    out = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
    st = L.jxlh_blend_image_rects(C.byref(desc), int(frame_w), int(frame_h), src, n_in, _addr(out) if cap else None, int(cap),
                                  C.byref(n))
    return st, (out[:n.value].copy() if st == OK else None), n.value


def blend_image_rects(desc, frame_w, frame_h, rects):
    """rects of a frame's result (what the *_changed_rects functions return) as rects of the image `desc` composes the
    frame onto: shifted by the frame's origin, clipped to the image, empty ones dropped -- the list blend_rects and,
    after it, frame_save_rects take"""
    st, out, _ = try_blend_image_rects(desc, frame_w, frame_h, rects)
    if st != OK:
        raise JxlHipError(st, "jxlh_blend_image_rects")
    return out


def try_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, rects, cap=None):
    """jxlh_extra_channel_changed_rects (host only), returning (status, rects [n, 4] as (x0, y0, w, h) or None, n needed).
    cap: room offered (None: as many as needed -- asked for first, as a C caller would)"""
    src, n_src = _rect_array(rects)
    L, n = load(), C.c_uint32(0)
    if cap is None:
        st = L.jxlh_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, _addr(src), n_src, None, 0, C.byref(n))
        if st != OK and n.value == 0:
            return st, None, 0
        cap = n.value
    out = np.zeros((max(int(cap), 1), 4), dtype=np.uint32)
    st = L.jxlh_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, _addr(src), n_src,
                                            _addr(out) if cap else None, int(cap), C.byref(n))
    return st, (out[:n.value].copy() if st == OK else None), n.value


def extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, rects):
    """the rectangles of the finished extra channel (w x h samples, factor ec_upsampling, cut to res_w x res_h) outside
    which new samples in `rects` (source samples, rows (x0, y0, w, h)) change nothing: one per input rect"""
    st, out, _ = try_extra_channel_changed_rects(w, h, ec_upsampling, res_w, res_h, rects)
    if st != OK:
        raise JxlHipError(st, "jxlh_extra_channel_changed_rects")
    return out


# jxlh_ec_rect as a numpy record (the C layout: `offset` is 8-byte aligned)
EC_RECT_DTYPE = np.dtype([("ec", np.uint32), ("x0", np.uint32), ("y0", np.uint32), ("w", np.uint32), ("h", np.uint32),
                          ("offset", np.uint64), ("stride", np.uint32)], align=True)


def pack_ec_rects(rects, stride_pad=0, fill=0):
    """(ec, x0, y0, samples [h, w]) rects -> (block, descs): one contiguous i32 block with every rect's rows `w +
    stride_pad` samples apart (the padding holds `fill`), and the jxlh_ec_rect records (EC_RECT_DTYPE) that name them"""
    descs = np.zeros(len(rects), dtype=EC_RECT_DTYPE)
    parts, off = [], 0
    for i, (ec, x0, y0, a) in enumerate(rects):
        a = np.asarray(a, dtype=np.int32)
        a = a.reshape(a.shape if a.ndim == 2 else (0, 0))
        h, w = a.shape
        stride = w + int(stride_pad)
        blk = np.full((h, stride), fill, dtype=np.int32)
        blk[:, :w] = a
        descs[i] = (ec, x0, y0, w, h, off, stride)
        parts.append(blk.reshape(-1))
        off += blk.size
    block = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(block, dtype=np.int32), descs


class SaveDesc(_abi.SaveDesc):
    """jxlh_save_desc, with the sizes callers allocate by."""

    @property
    def samples_per_pixel(self):
        return self.n_channels + (1 if self.fill_opaque_alpha else 0)

    @property
    def pixel_bytes(self):
        return self.samples_per_pixel * SAVE_SAMPLE_BYTES.get(self.format, 1)


def save_desc(channels, format=SAVE_U8, bit_depth=None, fill_opaque_alpha=False, big_endian=False, orientation=1,
              f16_clamp=None, premultiply=None, spot=(), n_channels=None, n_spot=None):
    """jxlh_save_desc.  channels: pipeline channels in output order (0..2 colour, 3 + ec extra channel ec);
    f16_clamp: (min, max) or None; premultiply: the alpha's pipeline channel or None; spot: [(ec, (r, g, b, a)), ...]"""
    d = SaveDesc()
    ch = list(channels)
    d.n_channels = len(ch) if n_channels is None else int(n_channels)
    for i, c in enumerate(ch[:4]):
        d.channels[i] = int(c)
    d.fill_opaque_alpha = 1 if fill_opaque_alpha else 0
    d.format = int(format)
    d.bit_depth = int({SAVE_U8: 8, SAVE_U16: 16}.get(format, 0) if bit_depth is None else bit_depth)
    d.big_endian = 1 if big_endian else 0
    d.orientation = int(orientation)
    if f16_clamp is not None:
        d.f16_clamp, d.f16_clamp_min, d.f16_clamp_max = 1, float(f16_clamp[0]), float(f16_clamp[1])
    if premultiply is not None:
        d.premultiply, d.premultiply_alpha_channel = 1, int(premultiply)
    sp = list(spot)
    d.n_spot = len(sp) if n_spot is None else int(n_spot)
    for i, (ec, rgba) in enumerate(sp[:8]):
        d.spot[i].ec = int(ec)
        for k in range(4):
            d.spot[i].rgba[k] = float(rgba[k])
    return d


def local_rct(begin_c, rct_type):
    """one RCT of a group's transform list, for pack_local_groups"""
    return {"kind": LOCAL_RCT, "begin_c": int(begin_c), "rct_type": int(rct_type)}


def local_palette(begin_c, num_c, table, num_deltas=0, predictor=0):
    """one palette of a group's transform list; table: the meta channel, i32 [num_c, num_colors + num_deltas]"""
    t = np.ascontiguousarray(table, dtype=np.int32).reshape(int(num_c), -1)
    return {"kind": LOCAL_PALETTE, "begin_c": int(begin_c), "num_c": int(num_c), "table": t,
            "num_colors": t.shape[1] - int(num_deltas), "num_deltas": int(num_deltas), "predictor": int(predictor)}


def pack_local_groups(specs, align=4, skew=0, stride_pad=0, fill=0):
    """Packs the coded channels and palettes of many groups into one arena.  specs: dicts with x0, y0, n_channels,
    steps (local_rct / local_palette, bitstream order) and coded (the 2-D i32 channels as decoded, one shape).  Every
    block starts on a multiple of `align` samples plus `skew`, rows are stride_pad samples longer than a multiple of
    `align`; the gaps hold `fill`.  Returns (arena, groups): an i32 array and a (LocalGroup * n) array."""
    groups = (LocalGroup * max(len(specs), 1))()
    blocks, pos = [], 0

    def place(a):
        nonlocal pos
        pos = -(-pos // align) * align + skew
        at = pos
        blocks.append((at, a))
        pos += a.size
        return at

    for g, sp in zip(groups, specs):
        coded = [np.asarray(c, dtype=np.int32) for c in sp["coded"]]
        h, w = coded[0].shape
        g.x0, g.y0, g.w, g.h = int(sp["x0"]), int(sp["y0"]), w, h
        g.n_channels, g.n_steps, g.n_coded = int(sp["n_channels"]), len(sp["steps"]), len(coded)
        if g.n_steps > LOCAL_MAX_STEPS or g.n_coded > LOCAL_MAX_CHANNELS:
            raise ValueError("a group holds at most 4 steps and 4 coded channels")
        for st, d in zip(g.steps, sp["steps"]):
            st.kind, st.begin_c, st.rct_type = d["kind"], d["begin_c"], d.get("rct_type", 0)
            if d["kind"] == LOCAL_PALETTE:
                st.num_c, st.num_colors, st.num_deltas, st.predictor = d["num_c"], d["num_colors"], d["num_deltas"], d["predictor"]
                st.palette_offset = place(d["table"].reshape(-1))
        stride = -(-w // align) * align + stride_pad
        g.coded_stride = stride
        for i, c in enumerate(coded):
            rows = np.full((h, stride), fill, dtype=np.int32)
            rows[:, :w] = c
            g.coded_offset[i] = place(rows.reshape(-1))
    arena = np.full(max(pos, 1), fill, dtype=np.int32)
    for at, a in blocks:
        arena[at:at + a.size] = a
    return arena, groups


def modular_local_lower(groups, bit_depth, arena_samples, n=None):
    """jxlh_modular_local_lower: (status, programs, first_bad); first_bad is None when no group was refused"""
    L = _lib()
    n = len(groups) if n is None else n
    progs = (LocalProgram * max(n, 1))()
    bad = C.c_size_t(2 ** 64 - 1)
    st = L.jxlh_modular_local_lower(groups, n, bit_depth, arena_samples, progs, C.byref(bad))
    return st, progs, (None if bad.value == 2 ** 64 - 1 else bad.value)


def wp_headers(headers):
    """a (WpHeader * n) array from n tuples (p1c, p2c, p3ca, p3cb, p3cc, p3cd, p3ce, w0, w1, w2, w3); None stays None"""
    if headers is None or isinstance(headers, C.Array):
        return headers
    arr = (WpHeader * max(len(headers), 1))()
    for dst, h in zip(arr, headers):
        (dst.p1c, dst.p2c, dst.p3ca, dst.p3cb, dst.p3cc, dst.p3cd, dst.p3ce, dst.w0, dst.w1, dst.w2, dst.w3) = [int(v) for v in h]
    return arr


def modular_local_lower_general(groups, bit_depth, arena_samples, wp=None, n=None):
    """jxlh_modular_local_lower_general: (status, programs, first_bad); wp: None, or one header per group (wp_headers)"""
    L = _lib()
    n = len(groups) if n is None else n
    progs = (LocalGeneralProgram * max(n, 1))()
    bad = C.c_size_t(2 ** 64 - 1)
    st = L.jxlh_modular_local_lower_general(groups, wp_headers(wp), n, bit_depth, arena_samples, progs, C.byref(bad))
    return st, progs, (None if bad.value == 2 ** 64 - 1 else bad.value)


def local_squeeze(params=()):
    """the squeeze of a group's transform list, for pack_local_squeeze_groups; params: (horizontal, in_place, begin_c,
    num_c) tuples -- none: default_squeeze"""
    return [tuple(int(v) for v in p) for p in params]


def default_squeeze(sizes, n_meta=0):
    """jxlh_modular_local_default_squeeze: the default list, as (horizontal, in_place, begin_c, num_c) tuples, for n_meta
    palette meta channels followed by image channels of sizes[i] = (w, h)"""
    L = _lib()
    w = (C.c_uint32 * len(sizes))(*[int(s[0]) for s in sizes])
    h = (C.c_uint32 * len(sizes))(*[int(s[1]) for s in sizes])
    out = (SqueezeParams * 80)()
    n = C.c_uint32(0)
    st = L.jxlh_modular_local_default_squeeze(w, h, len(sizes), n_meta, out, 80, C.byref(n))
    if st != OK:
        raise JxlHipError(st, "jxlh_modular_local_default_squeeze")
    return [(p.horizontal, p.in_place, p.begin_c, p.num_c) for p in list(out)[:n.value]]


def pack_local_squeeze_groups(specs, align=4, skew=0, stride_pad=0, fill=0):
    """pack_local_groups for the squeeze calls.  specs: dicts with x0, y0, w, h, n_channels, steps (local_rct /
    local_palette in front of the squeeze), squeeze (None: the group has none; else local_squeeze(...)) and coded: the
    2-D i32 channels as decoded, in list order, each of its own shape (a zero side: no samples).  Returns (arena, batch)
    with batch = (groups, coded, params): a (LocalSqueezeGroup * n), a (LocalCodedChannel * m) and a (SqueezeParams * k)
    array."""
    groups = (LocalSqueezeGroup * max(len(specs), 1))()
    n_coded = sum(len(sp["coded"]) for sp in specs)
    n_params = sum(len(sp["squeeze"] or ()) for sp in specs)
    coded = (LocalCodedChannel * max(n_coded, 1))()
    params = (SqueezeParams * max(n_params, 1))()
    blocks, pos, ci, pi = [], 0, 0, 0

    def place(a):
        nonlocal pos
        pos = -(-pos // align) * align + skew
        at = pos
        blocks.append((at, a))
        pos += a.size
        return at

    for g, sp in zip(groups, specs):
        g.x0, g.y0, g.w, g.h = int(sp["x0"]), int(sp["y0"]), int(sp["w"]), int(sp["h"])
        g.n_channels, g.n_steps = int(sp["n_channels"]), len(sp["steps"])
        if g.n_steps > LOCAL_MAX_STEPS:
            raise ValueError("a group holds at most 4 steps")
        for st, d in zip(g.steps, sp["steps"]):
            st.kind, st.begin_c, st.rct_type = d["kind"], d["begin_c"], d.get("rct_type", 0)
            if d["kind"] == LOCAL_PALETTE:
                st.num_c, st.num_colors, st.num_deltas, st.predictor = d["num_c"], d["num_colors"], d["num_deltas"], d["predictor"]
                st.palette_offset = place(d["table"].reshape(-1))
        sq = sp.get("squeeze")
        g.has_squeeze = 0 if sq is None else 1
        g.squeeze_pos = int(sp.get("squeeze_pos", g.n_steps)) if g.has_squeeze else 0
        g.params_first, g.n_params = pi, len(sq or ())
        for q in sq or ():
            params[pi].horizontal, params[pi].in_place, params[pi].begin_c, params[pi].num_c = q
            pi += 1
        g.coded_first, g.n_coded = ci, len(sp["coded"])
        for c in sp["coded"]:
            c = np.asarray(c, dtype=np.int32)
            h, w = c.shape
            stride = -(-w // align) * align + stride_pad
            coded[ci].w, coded[ci].h, coded[ci].stride = w, h, stride
            if w > 0 and h > 0:
                rows = np.full((h, stride), fill, dtype=np.int32)
                rows[:, :w] = c
                coded[ci].offset = place(rows.reshape(-1))
            ci += 1
    arena = np.full(max(pos, 1), fill, dtype=np.int32)
    for at, a in blocks:
        arena[at:at + a.size] = a
    return arena, (groups, coded, params)


def modular_local_lower_squeeze(batch, bit_depth, arena_samples, wp=None, n=None):
    """jxlh_modular_local_lower_squeeze: (status, programs, first_bad); batch: pack_local_squeeze_groups'"""
    L = _lib()
    groups, coded, params = batch
    n = len(groups) if n is None else n
    progs = (LocalSqueezeProgram * max(n, 1))()
    bad = C.c_size_t(2 ** 64 - 1)
    st = L.jxlh_modular_local_lower_squeeze(groups, n, coded, len(coded), params, len(params), wp_headers(wp), bit_depth,
                                            arena_samples, progs, C.byref(bad))
    return st, progs, (None if bad.value == 2 ** 64 - 1 else bad.value)


def local_dest(n_colour, ec=(), bit_depth=0, n_ec=None):
    """jxlh_local_dest: the leading n_colour (0, 1 or 3) channels of every group are the frame's colour channels, channel
    n_colour + k is extra channel ec[k]; bit_depth: the palettes', without colour only"""
    d = LocalDest()
    ec = [int(e) for e in ec]
    d.n_colour, d.n_ec, d.bit_depth = int(n_colour), len(ec) if n_ec is None else int(n_ec), int(bit_depth)
    for k, e in enumerate(ec[:4]):
        d.ec[k] = e
    return d


class JxlHipError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        super().__init__(f"{where}: status {status} {detail}")


_LOADED = None


def _lib():
    global _LOADED
    if _LOADED is None:
        _LOADED = load()
    return _LOADED


def load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C jxl_rs_amd/csrc` (or __graft_entry__.build()); "
            "there is no CPU fallback for the device path")
    return _abi.bind(C.CDLL(LIB_PATH))


def splines_bin_layout():
    """jxlh_splines_bin_layout (jxl_hip_dev.h, host only): (columns, rows) of the splines draw's bin"""
    cols, rows = C.c_uint32(0), C.c_uint32(0)
    st = _lib().jxlh_splines_bin_layout(C.byref(cols), C.byref(rows))
    if st != OK:
        raise JxlHipError(st, "splines_bin_layout")
    return cols.value, rows.value


def try_build_spline_segments(splines, quantization_adjustment, y_to_x_lf, y_to_b_lf, image_xsize, image_ysize,
                              high_precision=False, count_only=False):
    """jxlh_splines_build_segments (host only).  splines: (control point deltas [(dx, dy)], color_dct 3 x 32,
    sigma_dct 32, (start_x, start_y)) each.  Returns (status, segments as a float32 [n, 8] array in the field order of
    jxlh_spline_segment, or the count alone with count_only)."""
    L = _lib()
    n = len(splines)
    qs = (QuantizedSpline * max(n, 1))()
    keep = []
    for i, (deltas, color, sigma, start) in enumerate(splines):
        d = np.ascontiguousarray(np.asarray(deltas, dtype=np.int64).reshape(-1, 2))
        keep.append(d)
        qs[i].control_points = d.ctypes.data if d.size else None
        qs[i].n_points = d.shape[0]
        qs[i].color_dct[:] = [int(v) for v in np.asarray(color).reshape(96)]
        qs[i].sigma_dct[:] = [int(v) for v in np.asarray(sigma).reshape(32)]
        qs[i].start_x, qs[i].start_y = float(start[0]), float(start[1])
    count = C.c_size_t(0)
    args = (C.byref(qs), n, int(quantization_adjustment), C.c_float(y_to_x_lf), C.c_float(y_to_b_lf),
            int(image_xsize), int(image_ysize), 1 if high_precision else 0)
    st = L.jxlh_splines_build_segments(*args, None, 0, C.byref(count))
    if st != OK or count_only:
        return st, (count.value if st == OK else None)
    out = np.zeros((count.value, 8), np.float32)
    st = L.jxlh_splines_build_segments(*args, out.ctypes.data if out.size else None, count.value, C.byref(count))
    return st, out


def _squeeze_levels(levels, n_planes):
    """[(horizontal, out_w, out_h, [res planes], res_stride)] as a jxlh_squeeze_level array; a level whose planes are
    all None is a missing one (progressive previews)"""
    arr = (SqueezeLevel * max(len(levels), 1))()
    for i, (hz, ow, oh, res, rstride) in enumerate(levels):
        arr[i].horizontal = 1 if hz else 0
        arr[i].out_w, arr[i].out_h = ow, oh
        for p in range(3):
            arr[i].res[p] = _addr(res[p]).value if p < n_planes and p < len(res) and res[p] is not None else None
        arr[i].res_stride = rstride
    return arr


def squeeze_preview_kinds(levels, base_w, base_h, n_planes=1):
    """jxlh_squeeze_preview_kinds (host only): what each level of a preview chain runs (PREVIEW_REGULAR / _SMOOTH_1D /
    _SMOOTH_2D) and whether the final planes depend on it -> (kinds, live), two uint8 arrays.  levels as for
    Context.unsqueeze_chain; any non-zero integer stands for a present plane."""
    arr = _squeeze_levels(levels, n_planes)
    kinds, live = np.zeros(max(len(levels), 1), np.uint8), np.zeros(max(len(levels), 1), np.uint8)
    st = _lib().jxlh_squeeze_preview_kinds(n_planes, len(levels), C.cast(arr, C.c_void_p), base_w, base_h, _addr(kinds),
                                           _addr(live))
    if st != OK:
        raise JxlHipError(st, "squeeze_preview_kinds")
    return kinds[:len(levels)], live[:len(levels)]


def _squeeze_tiles(levels, tiles):
    """[(tile_w, tile_h, present)] per level as a jxlh_squeeze_tiles array (+ what keeps the masks alive): present is
    None or a [tiles_y, tiles_x] array, non-zero where the cell's residuals have arrived; (0, 0, ...) is one cell"""
    assert len(tiles) == len(levels), "one grid per level"
    arr, keep = (SqueezeTiles * max(len(levels), 1))(), []
    for i, ((_, ow, oh, _, _), (tw, th, present)) in enumerate(zip(levels, tiles)):
        arr[i].tile_w, arr[i].tile_h = tw, th
        if present is not None:
            m = np.ascontiguousarray(present, dtype=np.uint8)
            if tw and th:
                assert m.shape == (-(-oh // th), -(-ow // tw)), f"level {i}: the mask is [tiles_y, tiles_x]"
            keep.append(m)
            arr[i].present = m.ctypes.data
    return arr, keep


def squeeze_tile_grid(level, tile):
    """(tiles_x, tiles_y) of a level (horizontal, out_w, out_h, ...) under a grid (tile_w, tile_h, ...)"""
    tw, th = (tile[0], tile[1]) if tile[0] and tile[1] else (level[1], level[2])
    return -(-level[1] // tw), -(-level[2] // th)


def squeeze_tile_kinds(levels, tiles, base_w, base_h, level, n_planes=1):
    """jxlh_squeeze_tile_kinds (host only): the kind of every grid cell of `level` (PREVIEW_REGULAR / _SMOOTH_1D /
    _SMOOTH_2D) -> uint8 [tiles_y, tiles_x].  levels as for squeeze_preview_kinds, tiles as for
    Context.unsqueeze_chain_preview_tiles."""
    arr = _squeeze_levels(levels, n_planes)
    tarr, keep = _squeeze_tiles(levels, tiles)
    nx, ny = squeeze_tile_grid(levels[level], tiles[level]) if 0 <= level < len(levels) else (1, 1)
    kinds = np.zeros((ny, nx), np.uint8)
    st = _lib().jxlh_squeeze_tile_kinds(n_planes, len(levels), C.cast(arr, C.c_void_p), C.cast(tarr, C.c_void_p), base_w, base_h,
                                        level, _addr(kinds))
    if st != OK:
        raise JxlHipError(st, "squeeze_tile_kinds")
    return kinds


WORKLIST_REGIONS = 42  # jxlh_worklist_layout: counters, 11 class lists, 9 + 9 + 9 DCT-class regions, fb_any, units, LLF


def worklist_layout(xblocks, yblocks):
    """jxlh_worklist_layout (jxl_hip_dev.h, host only): (bytes allocated, [(offset, length)] of the 42 regions of the
    transform stage's work-list memory in memory order)"""
    L = _lib()
    out = np.zeros(1 + 2 * WORKLIST_REGIONS, np.uint64)
    st = L.jxlh_worklist_layout(C.c_int32(xblocks), C.c_int32(yblocks), _addr(out), C.c_int32(out.size))
    if st != 0:
        raise JxlHipError(st, "worklist_layout")
    return int(out[0]), [(int(out[1 + 2 * r]), int(out[2 + 2 * r])) for r in range(WORKLIST_REGIONS)]


def live_resources():
    """jxlh_live_resources (jxl_hip_dev.h, host only): (device buffers, pinned blocks, events, streams) the library
    holds right now over all contexts of the process"""
    out = (C.c_uint64 * 4)()
    st = _lib().jxlh_live_resources(out)
    if st != 0:
        raise JxlHipError(st, "live_resources")
    return tuple(int(v) for v in out)


def host_pack_slots(group_coeffs, group_id=0, bits12=False, entries=None, slot_counts=None, wide_capacity=4096):
    """jxlh_host_pack_slots: one group's dense slab (3 x 65536 i32) -> (entries, slot_counts [3, 1024] u8, n [3] u32,
    wide [k, 2] u32) -- the arguments of Context.submit_groups_slots.  Values outside the entries' range are split into
    repeated in-range entries (they add up on the device); `wide` only holds what no slot has room for.  entries /
    slot_counts: optional preallocated outputs (numpy arrays, e.g. views of pinned memory)."""
    L = _lib()
    g = np.ascontiguousarray(group_coeffs, dtype=np.int32).reshape(-1)
    assert g.size == 3 * 65536
    cap = 3 * 65536 + 64 * 1024  # room for split values
    if entries is None:
        entries = np.empty(cap * 3 // 2 if bits12 else cap, np.uint8 if bits12 else np.uint16)
    else:
        cap = entries.size * 2 // 3 if bits12 else entries.size
    if slot_counts is None:
        slot_counts = np.empty((3, 1024), np.uint8)
    n = np.zeros(3, np.uint32)
    wide = np.zeros((max(wide_capacity, 1), 2), np.uint32)
    nw = C.c_uint32(0)
    st = L.jxlh_host_pack_slots(_addr(g), group_id, GROUP_ENTRIES12 if bits12 else 0, _addr(entries), cap, _addr(slot_counts),
                                _addr(n), _addr(wide), wide_capacity, C.byref(nw))
    if st != 0:
        raise JxlHipError(st, "host_pack_slots")
    total = int(n.sum())
    return entries[: total * 3 // 2 if bits12 else total], slot_counts, n, wide[: nw.value]


def host_pack_slots_many(coeffs, group_ids, bits12=False, entries=None, slot_counts=None, n=None, wide_capacity=4096):
    """jxlh_host_pack_slots_many: the dense slabs of a batch of groups (coeffs [k, 3 x 65536] i32, C-contiguous rows) ->
    (entries, slot_counts [k, 3, 1024] u8, n [k, 3] u32, wide [m, 2] u32): the arrays of ONE Context.submit_groups_slots
    call for group_ids.  One C call for the whole batch (no per-group Python): what a decoder thread does for its share
    of a frame.  entries / slot_counts / n: optional preallocated outputs."""
    L = _lib()
    coeffs = np.asarray(coeffs)
    k = int(coeffs.shape[0])
    assert coeffs.dtype == np.int32 and coeffs[0].size == 3 * 65536 and all(coeffs[i].flags.c_contiguous for i in (0, k - 1))
    ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
    assert ids.size == k
    ptrs = np.array([coeffs[i].ctypes.data for i in range(k)], dtype=np.uint64)
    cap = k * (3 * 65536 + 64 * 1024)
    if entries is None:
        entries = np.empty(cap * 3 // 2 if bits12 else cap, np.uint8 if bits12 else np.uint16)
    else:
        cap = entries.size * 2 // 3 if bits12 else entries.size
    if slot_counts is None:
        slot_counts = np.empty((k, 3, 1024), np.uint8)
    if n is None:
        n = np.zeros((k, 3), np.uint32)
    wide = np.zeros((max(wide_capacity, 1), 2), np.uint32)
    nw, used = C.c_uint32(0), C.c_size_t(0)
    st = L.jxlh_host_pack_slots_many(_addr(ptrs), _addr(ids), k, GROUP_ENTRIES12 if bits12 else 0, _addr(entries), cap,
                                     _addr(slot_counts), _addr(n), _addr(wide), wide_capacity, C.byref(nw), C.byref(used))
    if st != 0:
        raise JxlHipError(st, "host_pack_slots_many")
    total = int(used.value)
    return entries[: total * 3 // 2 if bits12 else total], slot_counts, n, wide[: nw.value]


class SlotWriter:
    """jxlh_slot_writer_*: the slot-bucketed form written the way the entropy loop produces coefficients
    (frame/group.rs:557-575): varblock by varblock, `coeffs[c][offset + pos] += v` one update at a time."""

    def __init__(self):
        self.L = _lib()
        p = C.c_void_p()
        st = self.L.jxlh_slot_writer_create(C.byref(p))
        if st != 0:
            raise JxlHipError(st, "slot_writer_create")
        self._w = p

    def close(self):
        if self._w:
            self.L.jxlh_slot_writer_destroy(self._w)
            self._w = None

    __del__ = close

    def _chk(self, st, where):
        if st != 0:
            raise JxlHipError(st, where)

    def begin_group(self, group_id=0, bits12=False, capacity=3 * 65536 + 65536, wide_capacity=4096):
        self._bits12 = bits12
        self._entries = np.empty(capacity * 3 // 2 if bits12 else capacity, np.uint8 if bits12 else np.uint16)
        self._counts = np.empty((3, 1024), np.uint8)
        self._wide = np.zeros((max(wide_capacity, 1), 2), np.uint32)
        self._chk(self.L.jxlh_slot_writer_begin_group(self._w, group_id, GROUP_ENTRIES12 if bits12 else 0, _addr(self._entries),
                                                      capacity, _addr(self._counts), _addr(self._wide), wide_capacity),
                  "slot_writer_begin_group")

    def begin_varblock(self, first_slot, num_slots):
        self._chk(self.L.jxlh_slot_writer_begin_varblock(self._w, first_slot, num_slots), "slot_writer_begin_varblock")

    def add(self, channel, pos, value):
        self._chk(self.L.jxlh_slot_writer_add(self._w, channel, pos, value), "slot_writer_add")

    def add_many(self, channel, pos, value):
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        value = np.ascontiguousarray(value, dtype=np.int32)
        self._chk(self.L.jxlh_slot_writer_add_many(self._w, channel, _addr(pos), _addr(value), len(pos)), "slot_writer_add_many")

    def end_group(self):
        n = np.zeros(3, np.uint32)
        nw = C.c_uint32(0)
        self._chk(self.L.jxlh_slot_writer_end_group(self._w, _addr(n), C.byref(nw)), "slot_writer_end_group")
        total = int(n.sum())
        return self._entries[: total * 3 // 2 if self._bits12 else total], self._counts, n, self._wide[: nw.value]


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it, the launcher broadcasts it to every rank)"""
    buf = (C.c_uint8 * 128)()
    st = load().jxlh_comm_unique_id(buf)
    if st != OK:
        raise JxlHipError(st, "jxlh_comm_unique_id")
    return bytes(buf)


def _ctx_array(ctxs):
    arr = (C.c_void_p * len(ctxs))(*[c._ctx for c in ctxs])
    return arr


def comm_init_local(ctxs):
    """contexts of this process become ranks 0..n-1 of an in-process group (direct device copies)"""
    st = ctxs[0].L.jxlh_comm_init_local(_ctx_array(ctxs), len(ctxs))
    if st != OK:
        raise JxlHipError(st, "jxlh_comm_init_local")


def frames_run_sharded_local(ctxs):
    st = ctxs[0].L.jxlh_frames_run_sharded_local(_ctx_array(ctxs), len(ctxs))
    if st != OK:
        raise JxlHipError(st, "jxlh_frames_run_sharded_local", ctxs[0].L.jxlh_last_error(ctxs[0]._ctx).decode())


def frames_allgather_output_local(ctxs, desc, out_ptrs, bytes_per_row):
    arr = _ctx_array(ctxs)
    outs = (C.c_void_p * len(ctxs))(*out_ptrs)
    st = load().jxlh_frames_allgather_output_local(arr, len(ctxs), C.byref(desc), outs, bytes_per_row)
    if st != 0:
        raise JxlHipError(st, "frames_allgather_output_local")


def frames_allgather_local(ctxs):
    st = ctxs[0].L.jxlh_frames_allgather_local(_ctx_array(ctxs), len(ctxs))
    if st != OK:
        raise JxlHipError(st, "jxlh_frames_allgather_local", ctxs[0].L.jxlh_last_error(ctxs[0]._ctx).decode())


def comm_allgather_local(ctxs, bufs, bytes_per_rank):
    """in-place all-gather of one buffer per in-process rank (bufs[i]: device pointer / tensor of rank i)"""
    arr = (C.c_void_p * len(bufs))(*[_addr(b).value for b in bufs])
    st = ctxs[0].L.jxlh_comm_allgather_local(_ctx_array(ctxs), len(ctxs), arr, bytes_per_rank)
    if st != OK:
        raise JxlHipError(st, "jxlh_comm_allgather_local")


def _addr(a):
    """Address of a numpy array or a raw integer device pointer."""
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    if hasattr(a, "data_ptr"):  # torch tensor (device memory plumbing only)
        return C.c_void_p(a.data_ptr())
    if isinstance(a, DeviceArray):
        return C.c_void_p(a.ptr)
    return C.c_void_p(a.ctypes.data)


class DeviceArray:
    """A device buffer for harness code (tests, bench) that hands DEVICE pointers to the C ABI.  Allocated through the
    HIP runtime the library itself is linked against (ctypes on the already-loaded libamdhip64), not through torch: a second HIP
    runtime in the process (torch bundles its own) does not see the GPU once the first one holds it."""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            import ctypes as C
            cls._hip = C.CDLL("libamdhip64.so")
            cls._hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            cls._hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            cls._hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            cls._hip.hipFree.argtypes = [C.c_void_p]
            cls._hip.hipSetDevice.argtypes = [C.c_int]
            cls._hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        return cls._hip

    @classmethod
    def _settle(cls):
        """hipMemset returns before the fill has run, and a hipMemcpy from pageable memory may return once the data sits in
        the runtime's staging buffer: both are ordered on the NULL stream only, and the library's streams are non-blocking
        ones -- a kernel enqueued right behind such a call could run before it (seen as a 0.2 % flake of
        tests/soak_squeeze.py: an output plane zeroed after the kernel had written it).  Wait for the NULL stream."""
        cls._chk(cls.hip().hipStreamSynchronize(None), "hipStreamSynchronize(NULL)")

    @classmethod
    def _chk(cls, rc, what):
        # explicit checks, not asserts: under `python -O` an assert (and the HIP call inside it) would vanish
        if rc != 0:
            raise JxlHipError(ERR_DEVICE, what, f"hip error {rc}")

    def __init__(self, array=None, nbytes=None, device=None):
        """device: HIP device ordinal the buffer lives on (default: the calling thread's current device -- device 0
        unless something set another one; pass the Context's ordinal on multi-GPU hosts)"""
        import ctypes as C
        self.nbytes = array.nbytes if array is not None else nbytes
        self.ptr = 0
        if device is not None:
            self._chk(self.hip().hipSetDevice(int(device)), "hipSetDevice")
        p = C.c_void_p()
        self._chk(self.hip().hipMalloc(C.byref(p), max(self.nbytes, 16)), "hipMalloc")
        self.ptr = p.value
        if array is not None:
            a = np.ascontiguousarray(array)
            self._chk(self.hip().hipMemcpy(self.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
        else:
            self._chk(self.hip().hipMemset(self.ptr, 0, self.nbytes), "hipMemset")
        self._settle()

    def upload(self, array, byte_offset=0):
        a = np.ascontiguousarray(array)
        self._chk(self.hip().hipMemcpy(self.ptr + byte_offset, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
        self._settle()

    def download(self, dtype, count, byte_offset=0):
        out = np.empty(count, dtype=dtype)
        self._chk(self.hip().hipMemcpy(out.ctypes.data, self.ptr + byte_offset, out.nbytes, 2), "hipMemcpy D2H")
        return out

    def free(self):
        if self.ptr:
            self.hip().hipFree(self.ptr)
            self.ptr = 0


def _is_pointer(a):
    return isinstance(a, (int, np.integer, DeviceArray)) or hasattr(a, "data_ptr")


def _row_pitch(a):
    """Row pitch in elements of a 2-D array whose rows are contiguous, or None when it cannot be passed as it is (rows
    not contiguous, wrong byte order, negative or unaligned pitch)."""
    isz = a.dtype.itemsize
    if a.ndim != 2 or not a.dtype.isnative:
        return None
    h, w = a.shape
    if w > 1 and a.strides[1] != isz:
        return None
    if h <= 1:
        return max(w, 1)
    st = a.strides[0]
    if st < w * isz or st % isz:
        return None
    return st // isz


def _rect_planes_mixed(arrs, dtypes):
    """Host planes of one rect that share a row pitch in elements (their element types may differ).  Returns
    (arrays, w, h, pitch): the arrays as they are when every one has contiguous rows and they agree on the pitch,
    tight copies otherwise."""
    arrs = [np.asarray(a) for a in arrs]
    arrs = [a if a.dtype == np.dtype(dt) else a.astype(dt) for a, dt in zip(arrs, dtypes)]
    if any(a.ndim != 2 for a in arrs) or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("the planes of a rect are 2-D arrays of one shape: " + ", ".join(str(a.shape) for a in arrs))
    h, w = arrs[0].shape
    pitches = [_row_pitch(a) for a in arrs]
    if None in pitches or len(set(pitches)) != 1:
        arrs = [np.ascontiguousarray(a) for a in arrs]
        pitches = [max(w, 1)]
    return arrs, w, h, pitches[0]


def _rect_planes(arrs, dtype, w, h, stride):
    """Three planes of one element type: host arrays (see _rect_planes_mixed) or device pointers with explicit
    w, h, stride."""
    if any(_is_pointer(a) for a in arrs):
        if not all(_is_pointer(a) for a in arrs) or None in (w, h, stride):
            raise ValueError("device pointers need all three planes as pointers and explicit w, h, stride")
        return list(arrs), int(w), int(h), int(stride)
    if not (w is None and h is None and stride is None):
        raise ValueError("w, h and stride of host arrays come from the arrays themselves")
    return _rect_planes_mixed(arrs, (dtype,) * len(arrs))


class Context:
    """jxlh_ctx wrapper; raises JxlHipError on any non-zero status."""

    def __init__(self, device=0, n_slots=1):
        self.L = load()
        self.device = int(device)
        self._ctx = C.c_void_p()
        st = self.L.jxlh_ctx_create(device, n_slots, C.byref(self._ctx))
        if st != OK:
            raise JxlHipError(st, "jxlh_ctx_create", self.L.jxlh_status_string(st).decode())
        self._keep = {}  # slot -> host arrays an asynchronous H2D copy of that slot may still read

    def close(self):
        if self._ctx:
            for addr in getattr(self, "_pinned", []):
                self.L.jxlh_free_pinned(self._ctx, C.c_void_p(addr))
            self._pinned = []
            self.L.jxlh_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, where):
        if st != OK:
            raise JxlHipError(st, where, self.L.jxlh_status_string(st).decode() + " / " +
                              self.L.jxlh_last_error(self._ctx).decode())

    def default_params(self, xsize, ysize):
        p = FrameParams()
        self._chk(self.L.jxlh_default_frame_params(C.byref(p), xsize, ysize), "default_frame_params")
        return p

    # ---- frame ----
    def frame_begin(self, params):
        self.params = params
        self._blend_size = None
        # FrameHeader::size_blocks: whole blocks of the coarsest (sub-sampled) channel
        mh, mv = max(params.hshift), max(params.vshift)
        self.xblocks = -(-params.xsize // (8 << mh)) << mh
        self.yblocks = -(-params.ysize // (8 << mv)) << mv
        self._chk(self.L.jxlh_frame_begin(self._ctx, C.byref(params)), "frame_begin")

    def modular_frame_begin(self, params):
        """jxlh_frame_begin of a Modular frame: params.xsize x params.ysize coded samples, handed over with
        set_modular_channels; run, blend, save and the read-outs as for a VarDCT frame"""
        p = FrameParams.from_buffer_copy(params)  # the caller's params stay what they were
        p.flags |= FRAME_MODULAR
        self.frame_begin(p)

    def set_modular_channels(self, c0, c1, c2, sample_format, x0=0, y0=0, w=None, h=None, stride=None):
        """One rect of the three colour channels as the inverse transforms left them (sample_format: bits | exponent bits
        << 8, | MODULAR_XYB for coded Y, X, B).  Host arrays as in set_lf_quantized (a grey frame passes one array three
        times); DeviceArrays / raw device pointers: give w, h and stride (samples).  With chroma subsampling pass
        pointers or call the ABI directly: the three planes of a rect then differ in size."""
        if not hasattr(self.L, "jxlh_frame_set_modular_channels"):
            raise JxlHipError(ERR_UNSUPPORTED, "set_modular_channels", f"{LIB_PATH} predates Modular frames (no jxlh_frame_set_modular_channels)")
        (c0, c1, c2), w, h, stride = _rect_planes((c0, c1, c2), np.int32, w, h, stride)
        self._chk(self.L.jxlh_frame_set_modular_channels(self._ctx, x0, y0, w, h, _addr(c0), _addr(c1), _addr(c2), stride,
                                                         sample_format), "set_modular_channels")

    def set_modular_groups(self, arena, groups, sample_format, n=None, arena_samples=None, wait=True):
        """jxlh_frame_set_modular_groups (wait=False: the _async form, the arena stays valid until the next sync): every
        group's coded channels and transform list (pack_local_groups) -> the frame's sample planes in one launch.  arena:
        an i32 array, or a DeviceArray / raw device pointer with arena_samples."""
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
            if not wait:
                self._keep["local_arena"] = arena
        fn = self.L.jxlh_frame_set_modular_groups if wait else self.L.jxlh_frame_set_modular_groups_async
        self._chk(fn(self._ctx, _addr(arena), arena_samples, groups, n, sample_format, None), "set_modular_groups")

    def modular_local_transforms(self, arena, groups, bit_depth, out, out_w, out_h, out_stride, n=None, arena_samples=None):
        """jxlh_modular_local_transforms: the same launch into caller DEVICE planes (out: DeviceArrays / pointers)"""
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
        ptrs = (C.c_void_p * len(out))(*[_addr(o) for o in out])
        self._chk(self.L.jxlh_modular_local_transforms(self._ctx, _addr(arena), arena_samples, groups, n, bit_depth, ptrs,
                                                       len(out), out_w, out_h, out_stride, None), "modular_local_transforms")

    def set_modular_groups_general(self, arena, groups, sample_format, wp=None, n=None, arena_samples=None, wait=True):
        """jxlh_frame_set_modular_groups_general[_async]: set_modular_groups with every local palette (delta entries, all
        14 predictors); wp: None, or one weighted-predictor header per group (wp_headers)"""
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
            if not wait:
                self._keep["local_arena"] = arena
        fn = self.L.jxlh_frame_set_modular_groups_general if wait else self.L.jxlh_frame_set_modular_groups_general_async
        self._chk(fn(self._ctx, _addr(arena), arena_samples, groups, wp_headers(wp), n, sample_format, None),
                  "set_modular_groups_general")

    def modular_local_transforms_general(self, arena, groups, bit_depth, out, out_w, out_h, out_stride, wp=None, n=None,
                                         arena_samples=None):
        """jxlh_modular_local_transforms_general: modular_local_transforms with every local palette"""
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
        ptrs = (C.c_void_p * len(out))(*[_addr(o) for o in out])
        self._chk(self.L.jxlh_modular_local_transforms_general(self._ctx, _addr(arena), arena_samples, groups, wp_headers(wp), n,
                                                               bit_depth, ptrs, len(out), out_w, out_h, out_stride, None),
                  "modular_local_transforms_general")

    def set_modular_groups_squeeze(self, arena, batch, sample_format, wp=None, n=None, arena_samples=None, wait=True):
        """jxlh_frame_set_modular_groups_squeeze[_async]: set_modular_groups_general for groups with a local squeeze;
        batch: (groups, coded, params) of pack_local_squeeze_groups"""
        groups, coded, params = batch
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
            if not wait:
                self._keep["local_arena"] = arena
        fn = self.L.jxlh_frame_set_modular_groups_squeeze if wait else self.L.jxlh_frame_set_modular_groups_squeeze_async
        self._chk(fn(self._ctx, _addr(arena), arena_samples, groups, n, coded, len(coded), params, len(params), wp_headers(wp),
                     sample_format, None), "set_modular_groups_squeeze")

    def try_set_modular_groups_extra(self, arena, batch, sample_format, dest, wp=None, n=None, arena_samples=None, wait=True):
        """jxlh_frame_set_modular_groups_extra[_async], returning (status, first_bad); first_bad is None unless the
        refusal names a group"""
        if not hasattr(self.L, "jxlh_frame_set_modular_groups_extra"):
            raise JxlHipError(ERR_UNSUPPORTED, "set_modular_groups_extra",
                              f"{LIB_PATH} predates group-local transforms with extra channels")
        groups, coded, params = batch
        n = len(groups) if n is None else n
        if arena is not None and not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
            if not wait:
                self._keep["local_arena"] = arena
        bad = C.c_size_t(2 ** 64 - 1)
        fn = self.L.jxlh_frame_set_modular_groups_extra if wait else self.L.jxlh_frame_set_modular_groups_extra_async
        st = fn(self._ctx, None if arena is None else _addr(arena), arena_samples or 0, groups, n, coded, len(coded), params,
                len(params), wp_headers(wp), sample_format, None if dest is None else C.byref(dest), C.byref(bad))
        return st, (None if bad.value == 2 ** 64 - 1 else bad.value)

    def set_modular_groups_extra(self, arena, batch, sample_format, dest, wp=None, n=None, arena_samples=None, wait=True):
        """jxlh_frame_set_modular_groups_extra[_async]: set_modular_groups_squeeze for groups whose channels are the
        frame's colour channels followed by extra channels, or extra channels only (dest: local_dest(...)).  Every
        finished channel goes straight where the frame keeps it: colour into the sample planes, the others into the
        extra channels' sample stores, which are then "not rendered" until the next run, rerender or repaint."""
        st, _ = self.try_set_modular_groups_extra(arena, batch, sample_format, dest, wp, n, arena_samples, wait)
        self._chk(st, "set_modular_groups_extra")

    def modular_local_transforms_squeeze(self, arena, batch, bit_depth, out, out_w, out_h, out_stride, wp=None, n=None,
                                         arena_samples=None):
        """jxlh_modular_local_transforms_squeeze: modular_local_transforms_general for groups with a local squeeze"""
        groups, coded, params = batch
        n = len(groups) if n is None else n
        if not _is_pointer(arena):
            arena = np.ascontiguousarray(arena, dtype=np.int32)
            arena_samples = arena.size if arena_samples is None else arena_samples
        ptrs = (C.c_void_p * len(out))(*[_addr(o) for o in out])
        self._chk(self.L.jxlh_modular_local_transforms_squeeze(self._ctx, _addr(arena), arena_samples, groups, n, coded, len(coded),
                                                               params, len(params), wp_headers(wp), bit_depth, ptrs, len(out),
                                                               out_w, out_h, out_stride, None),
                  "modular_local_transforms_squeeze")

    def set_dequant_tables(self, tables):
        tabs = [np.ascontiguousarray(t, dtype=np.float32) for t in tables]
        ptrs = (C.c_void_p * NUM_QUANT_TABLES)(*[t.ctypes.data for t in tabs])
        sizes = (C.c_size_t * NUM_QUANT_TABLES)(*[t.size // 3 for t in tabs])
        self._chk(self.L.jxlh_frame_set_dequant_tables(self._ctx, ptrs, sizes), "set_dequant_tables")

    def set_lf_quantized(self, qy, qx, qb, x0=0, y0=0, extra_precision=0, w=None, h=None, stride=None):
        """One rect of the quantised LF (coded order Y, X, B).  Host arrays: 2-D, rows contiguous, any row pitch (a slice
        `big[y0:y1, x0:x1]` is passed as it is).  DeviceArrays / raw device pointers: give w, h and stride (samples)."""
        (qy, qx, qb), w, h, stride = _rect_planes((qy, qx, qb), np.int32, w, h, stride)
        self._chk(self.L.jxlh_frame_set_lf_quantized(self._ctx, x0, y0, w, h, _addr(qy), _addr(qx), _addr(qb), stride,
                                                     extra_precision), "set_lf_quantized")

    def set_lf(self, x, y, b, x0=0, y0=0, w=None, h=None, stride=None):
        """One rect of the LF the host has already dequantised (X, Y, B); arrays and pointers as in set_lf_quantized."""
        (x, y, b), w, h, stride = _rect_planes((x, y, b), np.float32, w, h, stride)
        self._chk(self.L.jxlh_frame_set_lf(self._ctx, x0, y0, w, h, _addr(x), _addr(y), _addr(b), stride), "set_lf")

    def set_hf_meta(self, transform_map, raw_quant, epf_map, ytox, ytob, x0=0, y0=0, w=None, h=None, map_stride=None,
                    cmap_stride=None):
        """One rect of the HfMetadata maps.  The three block maps share one row pitch (in elements), ytox and ytob
        another; host arrays as in set_lf_quantized.  DeviceArrays / raw device pointers: give w, h, map_stride and
        cmap_stride."""
        maps = (transform_map, raw_quant, epf_map)
        if any(_is_pointer(a) for a in maps + (ytox, ytob)):
            if not all(_is_pointer(a) for a in maps + (ytox, ytob)) or None in (w, h, map_stride, cmap_stride):
                raise ValueError("device pointers need all five maps as pointers and explicit w, h, map_stride, cmap_stride")
            tm, rq, em, yx, yb = maps + (ytox, ytob)
        else:
            if not (w is None and h is None and map_stride is None and cmap_stride is None):
                raise ValueError("w, h and the strides of host arrays come from the arrays themselves")
            (tm, rq, em), w, h, map_stride = _rect_planes_mixed(maps, (np.uint8, np.int32, np.uint8))
            (yx, yb), cw, ch, cmap_stride = _rect_planes_mixed((ytox, ytob), (np.int8, np.int8))
        self._chk(self.L.jxlh_frame_set_hf_meta(self._ctx, x0, y0, w, h, _addr(tm), _addr(rq), _addr(em), map_stride,
                                                _addr(yx), _addr(yb), cmap_stride), "set_hf_meta")

    def submit_group(self, group_id, coeffs, slot=0, flags=GROUP_COMPLETE):
        if isinstance(coeffs, np.ndarray):
            coeffs = np.ascontiguousarray(coeffs, dtype=np.int32)
            assert coeffs.size == 3 * 65536
            self._keep.setdefault(slot, []).append(coeffs)  # async H2D: keep alive until the slot is waited on
        self._chk(self.L.jxlh_submit_group(self._ctx, slot, group_id, _addr(coeffs), flags), "submit_group")

    def submit_group_sparse(self, group_id, pairs, n, wide=None, slot=0, flags=GROUP_COMPLETE):
        """pairs: uint32 array of little-endian {u16 pos; i16 val} (X run, Y run, B run); n: 3 counts;
        wide: uint32 array [k, 2] of (channel*65536 + pos, value) for values outside i16."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        nw = 0 if wide is None else len(wide)
        wide = None if nw == 0 else np.ascontiguousarray(wide, dtype=np.uint32)
        self._keep.setdefault(slot, []).append((pairs, n, wide))
        self._chk(self.L.jxlh_submit_group_sparse(self._ctx, slot, group_id, _addr(pairs) if pairs.size else None,
                                                  _addr(n), None if wide is None else _addr(wide), nw, flags),
                  "submit_group_sparse")

    def submit_groups_sparse(self, group_ids, pairs, n, wide=None, slot=0, flags=GROUP_COMPLETE):
        """Batched form; pairs may be a numpy array or a raw host address (pinned memory)."""
        group_ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        nw = 0 if wide is None else len(wide)
        wide = None if nw == 0 else np.ascontiguousarray(wide, dtype=np.uint32)
        addr = pairs if isinstance(pairs, int) else _addr(np.ascontiguousarray(pairs, dtype=np.uint32))
        self._keep.setdefault(slot, []).append((group_ids, pairs, n, wide))
        self._chk(self.L.jxlh_submit_groups_sparse(self._ctx, slot, len(group_ids), _addr(group_ids), addr, _addr(n),
                                                   None if wide is None else _addr(wide), nw, flags),
                  "submit_groups_sparse")

    def submit_groups_sparse8(self, group_ids, pos, val, n, wide=None, slot=0, flags=GROUP_COMPLETE):
        """3-byte form: pos (uint16) and val (int8) arrays, or raw host addresses (pinned memory)."""
        group_ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        nw = 0 if wide is None else len(wide)
        wide = None if nw == 0 else np.ascontiguousarray(wide, dtype=np.uint32)
        if not isinstance(pos, int):
            pos = np.ascontiguousarray(pos, dtype=np.uint16)
            val = np.ascontiguousarray(val, dtype=np.int8)
        pa = pos if isinstance(pos, int) else _addr(pos)
        va = val if isinstance(val, int) else _addr(val)
        self._keep.setdefault(slot, []).append((group_ids, pos, val, n, wide))
        self._chk(self.L.jxlh_submit_groups_sparse8(self._ctx, slot, len(group_ids), _addr(group_ids), pa, va, _addr(n),
                                                    None if wide is None else _addr(wide), nw, flags),
                  "submit_groups_sparse8")

    def submit_groups_sparse4(self, group_ids, entries, seg_counts, pos8=None, val8=None, n8=None, wide=None, slot=0,
                              flags=GROUP_COMPLETE):
        """2-byte form (synth.to_sparse4): arrays, or raw host addresses (pinned memory) for entries / seg_counts /
        pos8 / val8."""
        group_ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        nw = 0 if wide is None else len(wide)
        wide = None if nw == 0 else np.ascontiguousarray(wide, dtype=np.uint32)

        def prep(a, dt):
            if a is None or isinstance(a, int):
                return a, (a if a else None)
            a = np.ascontiguousarray(a, dtype=dt)
            return a, (_addr(a) if a.size else None)
        entries, ea = prep(entries, np.uint16)
        seg_counts, ca = prep(seg_counts, np.uint16)
        pos8, pa = prep(pos8, np.uint16)
        val8, va = prep(val8, np.int8)
        n8 = None if n8 is None else np.ascontiguousarray(n8, dtype=np.uint32)
        self._keep.setdefault(slot, []).append((group_ids, entries, seg_counts, pos8, val8, n8, wide))
        self._chk(self.L.jxlh_submit_groups_sparse4(self._ctx, slot, len(group_ids), _addr(group_ids), ea, ca, pa, va,
                                                    None if n8 is None else _addr(n8),
                                                    None if wide is None else _addr(wide), nw, flags),
                  "submit_groups_sparse4")

    def submit_groups_slots(self, group_ids, entries, slot_counts, n, wide=None, slot=0, flags=GROUP_COMPLETE):
        """slot-bucketed 2-byte form (synth.to_slots): arrays, or raw host addresses (pinned memory) for entries /
        slot_counts"""
        group_ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        nw = 0 if wide is None else len(wide)
        wide = None if nw == 0 else np.ascontiguousarray(wide, dtype=np.uint32)
        if not isinstance(entries, int):
            entries = np.ascontiguousarray(entries, dtype=np.uint8 if (flags & GROUP_ENTRIES12) else np.uint16)
        if not isinstance(slot_counts, int):
            slot_counts = np.ascontiguousarray(slot_counts, dtype=np.uint8)
        ea = entries if isinstance(entries, int) else (_addr(entries) if entries.size else None)
        ca = slot_counts if isinstance(slot_counts, int) else _addr(slot_counts)
        self._keep.setdefault(slot, []).append((group_ids, entries, slot_counts, n, wide))
        self._chk(self.L.jxlh_submit_groups_slots(self._ctx, slot, len(group_ids), _addr(group_ids), ea, ca, _addr(n),
                                                  None if wide is None else _addr(wide), nw, flags),
                  "submit_groups_slots")

    def alloc_pinned(self, nbytes):
        """Pinned host buffer (jxlh_alloc_pinned) as a uint8 numpy view; freed with the context."""
        p = C.c_void_p()
        self._chk(self.L.jxlh_alloc_pinned(self._ctx, nbytes, C.byref(p)), "alloc_pinned")
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        self._pinned = getattr(self, "_pinned", []) + [p.value]
        return np.frombuffer(buf, dtype=np.uint8), p.value

    def slot_wait(self, slot=0):
        self._chk(self.L.jxlh_slot_wait(self._ctx, slot), "slot_wait")
        self._keep.pop(slot, None)

    def slot_after(self, slot, after_ctx, after_slot):
        """submissions on (self, slot) from now on start when the uploads enqueued so far on (after_ctx, after_slot) have
        landed (jxlh_slot_after): device-side ordering across contexts, the host does not block"""
        self._chk(self.L.jxlh_slot_after(self._ctx, slot, after_ctx._ctx, after_slot), "slot_after")

    def coeff_buffer(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self.L.jxlh_frame_coeff_buffer(self._ctx, C.byref(p), C.byref(n)), "frame_coeff_buffer")
        return p.value, n.value

    def frame_run(self, group_row0=0, group_row1=0xFFFFFFFF):
        self._blend_size = None  # a render discards the composition
        self._chk(self.L.jxlh_frame_run(self._ctx, group_row0, group_row1), "frame_run")

    def rerender_groups(self, group_ids):
        ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        if len(ids):
            self._blend_size = None
        self._chk(self.L.jxlh_frame_rerender_groups(self._ctx, _addr(ids), len(ids)), "frame_rerender_groups")

    def try_repaint_groups(self, group_ids):
        """jxlh_frame_repaint_groups, returning the status: rerender_groups for every kind of unsharded frame (upsampled
        and Modular frames included).  group_ids None: a null pointer with count 1 (the argument check)"""
        if group_ids is None:
            return self.L.jxlh_frame_repaint_groups(self._ctx, None, 1)
        ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        st = self.L.jxlh_frame_repaint_groups(self._ctx, _addr(ids), len(ids))
        if st == OK and len(ids):
            self._blend_size = None
        return st

    def repaint_groups(self, group_ids):
        self._chk(self.try_repaint_groups(group_ids), "frame_repaint_groups")

    def try_set_groups_lf_only(self, group_ids):
        ids = np.ascontiguousarray(group_ids, dtype=np.uint32)
        return self.L.jxlh_frame_set_groups_lf_only(self._ctx, _addr(ids), len(ids))

    def set_groups_lf_only(self, group_ids):
        """jxlh_frame_set_groups_lf_only: the listed groups have no HF yet -- the next frame_run / rerender_groups fills
        them from the LF image upsampled 8x instead of transforming them (upsample_lf_group of the reference); a later
        submission of a group clears its mark, frame_begin clears them all"""
        self._chk(self.try_set_groups_lf_only(group_ids), "frame_set_groups_lf_only")

    def sync(self):
        self._chk(self.L.jxlh_ctx_sync(self._ctx), "ctx_sync")
        self._keep.clear()

    def wait_stream(self, hip_stream=None):
        """jxlh_ctx_wait_stream: whatever is enqueued so far on the caller's stream (None = the NULL stream) happens before
        what this context enqueues from now on (device-side; the hand-over of caller-filled device buffers)"""
        self._chk(self.L.jxlh_ctx_wait_stream(self._ctx, hip_stream), "ctx_wait_stream")

    def wait_event(self, hip_event):
        self._chk(self.L.jxlh_ctx_wait_event(self._ctx, hip_event), "ctx_wait_event")

    def record_event(self, hip_event):
        self._chk(self.L.jxlh_ctx_record_event(self._ctx, hip_event), "ctx_record_event")

    def mark(self):
        """a point in the main stream (jxlh_ctx_mark): everything enqueued so far"""
        m = C.c_uint32(0)
        self._chk(self.L.jxlh_ctx_mark(self._ctx, C.byref(m)), "ctx_mark")
        return m.value

    def wait_mark(self, mark):
        """blocks until that point is reached -- not for work enqueued after it (jxlh_ctx_wait_mark)"""
        self._chk(self.L.jxlh_ctx_wait_mark(self._ctx, mark), "ctx_wait_mark")

    def probe_copy_bandwidth(self, nbytes, reps=10):
        """GB/s (read + written) of a float4 device-to-device copy of nbytes"""
        v = C.c_float()
        self._chk(self.L.jxlh_probe_copy_bandwidth(self._ctx, nbytes, reps, C.byref(v)), "probe_copy_bandwidth")
        return v.value

    def set_extra_channel(self, ec, samples, bits_per_sample, ec_upsampling=1, exp_bits=0):
        """hands Modular channel 3 + ec over as decoded (i32 [h, w]); processed by the next frame_run"""
        a = np.ascontiguousarray(samples, dtype=np.int32)
        h, w = a.shape
        self._chk(self.L.jxlh_frame_set_extra_channel(self._ctx, ec, _addr(a), w, w, h, bits_per_sample | exp_bits << 8,
                                                      ec_upsampling),
                  "frame_set_extra_channel")

    def begin_extra_channel(self, ec, w, h, bits_per_sample, ec_upsampling=1, exp_bits=0):
        """jxlh_frame_begin_extra_channel: declares extra channel `ec` of w x h samples, all zero until rects set them"""
        self._chk(self.L.jxlh_frame_begin_extra_channel(self._ctx, ec, w, h, bits_per_sample | exp_bits << 8, ec_upsampling),
                  "frame_begin_extra_channel")

    def try_set_extra_channel_rects(self, block, descs, n_samples=None, n=None, wait=True):
        """jxlh_frame_set_extra_channel_rects (wait=False: the _async form), returning (status, first_bad or None).  block: an
        i32 array, or a DeviceArray / raw device pointer with n_samples; descs: EC_RECT_DTYPE records (or None with n)"""
        if block is not None and not _is_pointer(block):
            block = np.ascontiguousarray(block, dtype=np.int32)
            n_samples = block.size if n_samples is None else n_samples
            if not wait:
                self._keep["ec_block"] = block
        if descs is not None:
            descs = np.ascontiguousarray(descs, dtype=EC_RECT_DTYPE)
            n = len(descs) if n is None else n
        bad = C.c_uint32(0xFFFFFFFF)
        fn = self.L.jxlh_frame_set_extra_channel_rects if wait else self.L.jxlh_frame_set_extra_channel_rects_async
        st = fn(self._ctx, None if block is None else _addr(block), int(n_samples or 0),
                None if descs is None else _addr(descs), int(n or 0), C.byref(bad))
        return st, (None if bad.value == 0xFFFFFFFF else bad.value)

    def set_extra_channel_rects(self, rects, wait=True, block=None, n_samples=None, stride_pad=0):
        """Samples of extra channels as they arrive: rects = (ec, x0, y0, samples [h, w]) tuples, packed into one block
        and handed over in one call; converted by the next frame_run / rerender_groups.  With `block` (an i32 array, a
        DeviceArray or a raw device pointer with n_samples) rects are EC_RECT_DTYPE records that name samples of it."""
        if block is None:
            block, descs = pack_ec_rects(rects, stride_pad=stride_pad)
        else:
            descs = rects
        st, bad = self.try_set_extra_channel_rects(block, descs, n_samples=n_samples, wait=wait)
        self._chk(st, "frame_set_extra_channel_rects" + ("" if bad is None else f" (rect {bad})"))

    def read_extra_channel(self, ec, out_w, out_h):
        out = np.zeros((out_h, out_w), dtype=np.float32)
        pl = Plane(out.ctypes.data, out_w * 4, out_h, out_w * 4)
        self._chk(self.L.jxlh_frame_read_extra_channel(self._ctx, ec, C.byref(pl)), "frame_read_extra_channel")
        return out

    # ---- patches ----
    def set_reference(self, slot, planes):
        """jxlh_ctx_set_reference: reference slot `slot` <- the 3 + num_ec f32 planes [h, w] (host arrays)"""
        pl = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
        h, w = pl[0].shape
        assert all(a.shape == (h, w) for a in pl)
        pp = (C.c_void_p * len(pl))(*[a.ctypes.data for a in pl])
        self._chk(self.L.jxlh_ctx_set_reference(self._ctx, slot, len(pl), w, h, pp, w), "ctx_set_reference")

    def save_reference(self, slot):
        self._chk(self.L.jxlh_frame_save_reference(self._ctx, slot), "frame_save_reference")

    def clear_reference(self, slot):
        self._chk(self.L.jxlh_ctx_clear_reference(self._ctx, slot), "ctx_clear_reference")

    @staticmethod
    def _patch_arrays(patches, blendings, ec_flags):
        n = len(patches)
        pa = (Patch * max(n, 1))()
        for i, p in enumerate(patches):
            pa[i] = Patch(*[int(v) for v in p])
        bl = list(blendings)
        ba = (PatchBlending * max(len(bl), 1))()
        for i, b in enumerate(bl):
            ba[i] = PatchBlending(*[int(v) for v in b])
        fl = (C.c_uint32 * max(len(ec_flags), 1))(*[int(v) for v in ec_flags])
        return n, pa, ba, fl

    def set_patches(self, patches, blendings, ec_flags=(), num_ec=None):
        """jxlh_frame_set_patches.  patches: (x, y, ref_slot, ref_x0, ref_y0, xsize, ysize) each, in order of
        application; blendings: len(patches) * (1 + num_ec) (mode, alpha_channel, clamp) triples, the colour blending of
        each patch first; ec_flags: EC_ALPHA / EC_ALPHA_ASSOCIATED per extra channel (try_set_patches: the same,
        returning the status instead of raising)"""
        self._chk(self.try_set_patches(patches, blendings, ec_flags, num_ec), "frame_set_patches")

    def try_set_patches(self, patches, blendings, ec_flags=(), num_ec=None):
        n, pa, ba, fl = self._patch_arrays(patches, blendings, ec_flags)
        nec = len(ec_flags) if num_ec is None else num_ec
        return self.L.jxlh_frame_set_patches(self._ctx, C.byref(pa), n, C.byref(ba), nec, C.byref(fl))

    def stage_patches(self, planes):
        """jxlh_stage_patches: the current dictionary applied to copies of the 3 + num_ec f32 planes [h, w]"""
        pl = [np.ascontiguousarray(a, dtype=np.float32).copy() for a in planes]
        h, w = pl[0].shape
        pp = (C.c_void_p * len(pl))(*[a.ctypes.data for a in pl])
        self._chk(self.L.jxlh_stage_patches(self._ctx, pp, len(pl), w, h, w), "stage_patches")
        return pl

    # ---- splines ----
    def try_set_splines(self, segments):
        """jxlh_frame_set_splines, returning the status.  segments: float32 [n, 8] in the field order of
        jxlh_spline_segment (center_x, center_y, maximum_distance, inv_sigma, sigma_over_4_times_intensity, color[3])"""
        seg = np.ascontiguousarray(np.asarray(segments, dtype=np.float32).reshape(-1, 8))
        return self.L.jxlh_frame_set_splines(self._ctx, seg.ctypes.data if seg.size else None, seg.shape[0])

    def set_splines(self, segments):
        self._chk(self.try_set_splines(segments), "frame_set_splines")

    def stage_splines(self, planes, w=None):
        """jxlh_stage_splines: the current segments drawn onto copies of the three f32 planes [h, row]; the image is
        their first w columns (all of them by default), the row stride is `row`"""
        pl = [np.ascontiguousarray(a, dtype=np.float32).copy() for a in planes]
        h, row = pl[0].shape
        w = row if w is None else w
        pp = (C.c_void_p * 3)(*[a.ctypes.data for a in pl])
        self._chk(self.L.jxlh_stage_splines(self._ctx, pp, w, h, row), "stage_splines")
        return pl

    def set_spline_batch_budget(self, entries):
        """jxlh_splines_set_batch_budget (jxl_hip_dev.h): bin entries per batch of the splines draw, 0 = default"""
        self._chk(self.L.jxlh_splines_set_batch_budget(self._ctx, int(entries)), "splines_set_batch_budget")

    # ---- frame blending ----
    def try_blend(self, desc, colour=None):
        """jxlh_frame_blend, returning the status.  desc: blend_desc(...); colour: output_desc(...) naming the colour
        stage to run in front (None: the planes are in the output colour space already)"""
        st = self.L.jxlh_frame_blend(self._ctx, C.byref(desc), None if colour is None else C.byref(colour))
        if st == OK:
            self._blend_size = (desc.image_w, desc.image_h)
        return st

    def blend(self, desc, colour=None):
        """jxlh_frame_blend: the rendered frame composed onto the image from the reference slots; the image becomes what
        read_planes / read_extra_channel / save_reference / read_output(COLOR_NONE) see"""
        self._chk(self.try_blend(desc, colour), "frame_blend")

    def try_stage_blend(self, desc, planes):
        pl = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
        h, w = pl[0].shape
        out = [np.zeros((desc.image_h, desc.image_w), dtype=np.float32) for _ in pl]
        pp = (C.c_void_p * len(pl))(*[a.ctypes.data for a in pl])
        po = (C.c_void_p * len(pl))(*[a.ctypes.data for a in out])
        return self.L.jxlh_stage_blend(self._ctx, C.byref(desc), pp, len(pl), w, h, w, po, desc.image_w), out

    def stage_blend(self, desc, planes):
        """jxlh_stage_blend: the 3 + num_ec f32 planes [h, w] blended onto the image; returns the image's planes"""
        st, out = self.try_stage_blend(desc, planes)
        self._chk(st, "stage_blend")
        return out

    # ---- blend rectangles ----
    def try_blend_rects(self, desc, rects, colour=None):
        """jxlh_frame_blend_rects, returning the status.  rects: rows (x0, y0, w, h) of the IMAGE (blend_image_rects)"""
        r, n = _rect_array(rects)
        st = self.L.jxlh_frame_blend_rects(self._ctx, C.byref(desc), None if colour is None else C.byref(colour),
                                           _addr(r) if n else None, n)
        if st == OK:
            self._blend_size = (desc.image_w, desc.image_h)
        return st

    def blend_rects(self, desc, rects, colour=None):
        """jxlh_frame_blend_rects: after a re-render, only the pixels of `rects` of the composition blend() left are
        composed again; the image is the frame's result again, as after blend()"""
        self._chk(self.try_blend_rects(desc, rects, colour), "frame_blend_rects")

    def try_stage_blend_rects(self, desc, planes, rects, out, out_stride=None):
        """jxlh_stage_blend_rects, returning the status.  planes: the 3 + num_ec f32 frame planes [h, w]; out: as many
        image planes that hold a composition -- float32 arrays [image_h, image_w], rewritten in the rects, or device
        pointers with out_stride (floats)"""
        pl = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
        h, w = pl[0].shape
        r, n = _rect_array(rects)
        if out_stride is None:
            out_stride = out[0].strides[0] // 4
        pp = (C.c_void_p * len(pl))(*[a.ctypes.data for a in pl])
        po = (C.c_void_p * len(out))(*[_addr(a).value for a in out])
        return self.L.jxlh_stage_blend_rects(self._ctx, C.byref(desc), pp, len(pl), w, h, w, _addr(r) if n else None, n, po,
                                             int(out_stride))

    def stage_blend_rects(self, desc, planes, rects, out, out_stride=None):
        """jxlh_stage_blend_rects: the rects of the image planes `out` composed again, in place; returns `out`"""
        self._chk(self.try_stage_blend_rects(desc, planes, rects, out, out_stride), "stage_blend_rects")
        return out

    # ---- the save tail ----
    @staticmethod
    def save_shape(desc, w, h):
        """(rows, samples per row) of the oriented image a w x h source is saved as"""
        ow, oh = (h, w) if desc.orientation >= 5 else (w, h)
        return oh, ow * desc.samples_per_pixel

    @staticmethod
    def _save_dtype(desc):
        return {SAVE_U8: np.uint8, SAVE_U16: np.uint16, SAVE_F16: np.uint16, SAVE_F32: np.uint32}[desc.format]

    def try_frame_save(self, desc, colour=None, y0=0, y1=None, out=None, bytes_per_row=None, wait=True):
        """jxlh_frame_save (_async when not `wait`), returning (status, out).  out: None (a zeroed array of the oriented
        image's samples -- f16 as uint16 bits, f32 as uint32 bits -- is made), a numpy array, or a device pointer /
        DeviceArray with bytes_per_row given"""
        w, h = self.out_size
        if out is None:
            out = np.zeros(self.save_shape(desc, w, h), dtype=self._save_dtype(desc))
        if bytes_per_row is None:
            bytes_per_row = out.strides[0]
        fn = self.L.jxlh_frame_save if wait else self.L.jxlh_frame_save_async
        st = fn(self._ctx, None if colour is None else C.byref(colour), C.byref(desc), int(y0), int(h if y1 is None else y1),
                _addr(out), int(bytes_per_row))
        return st, out

    def frame_save(self, desc, colour=None, y0=0, y1=None, out=None, bytes_per_row=None, wait=True):
        """jxlh_frame_save: the frame's result through spot colours, premultiplication, conversion and orientation into
        the interleaved image `desc` (save_desc(...)) names; colour: output_desc(...) of the colour stage in front"""
        st, out = self.try_frame_save(desc, colour, y0, y1, out, bytes_per_row, wait)
        self._chk(st, "frame_save")
        return out

    def try_stage_save(self, desc, planes, colour=None, origin=(0, 0), y0=0, y1=None, out=None, bytes_per_row=None,
                       size=None, stride=None):
        """jxlh_stage_save on 3 + num_ec planes: float32 arrays [h, w], or device pointers with size=(w, h) and stride"""
        if size is None:
            pl = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
            h, w = pl[0].shape
            stride = w
        else:
            pl = list(planes)
            w, h = size
            stride = w if stride is None else stride
        if out is None:
            out = np.zeros(self.save_shape(desc, w, h), dtype=self._save_dtype(desc))
        if bytes_per_row is None:
            bytes_per_row = out.strides[0]
        pp = (C.c_void_p * len(pl))(*[_addr(a).value for a in pl])
        st = self.L.jxlh_stage_save(self._ctx, None if colour is None else C.byref(colour), C.byref(desc), pp, len(pl), w, h,
                                    stride, int(origin[0]), int(origin[1]), int(y0), int(h if y1 is None else y1),
                                    _addr(out), int(bytes_per_row))
        return st, out

    def stage_save(self, desc, planes, colour=None, origin=(0, 0), y0=0, y1=None, out=None, bytes_per_row=None,
                   size=None, stride=None):
        st, out = self.try_stage_save(desc, planes, colour, origin, y0, y1, out, bytes_per_row, size, stride)
        self._chk(st, "stage_save")
        return out

    # ---- save rectangles ----
    def changed_rects(self, group_ids):
        """jxlh_changed_rects for the current frame's parameters"""
        return changed_rects(self.params, group_ids)

    def repaint_changed_rects(self, group_ids):
        """jxlh_repaint_changed_rects for the current frame's parameters"""
        return repaint_changed_rects(self.params, group_ids)

    def try_frame_save_rects(self, desc, rects, colour=None, out=None, bytes_per_row=None, wait=True):
        """jxlh_frame_save_rects (_async when not `wait`), returning (status, out).  rects: rows (x0, y0, w, h) of the
        result; out as in try_frame_save (the WHOLE oriented image; a zeroed one is made when None)"""
        w, h = self.out_size
        if out is None:
            out = np.zeros(self.save_shape(desc, w, h), dtype=self._save_dtype(desc))
        if bytes_per_row is None:
            bytes_per_row = out.strides[0]
        r, n = _rect_array(rects)
        fn = self.L.jxlh_frame_save_rects if wait else self.L.jxlh_frame_save_rects_async
        st = fn(self._ctx, None if colour is None else C.byref(colour), C.byref(desc), _addr(r) if n else None, n,
                _addr(out), int(bytes_per_row))
        return st, out

    def frame_save_rects(self, desc, rects, colour=None, out=None, bytes_per_row=None):
        """jxlh_frame_save_rects: only the pixels of `rects` of the frame's result, each at its display position in `out`"""
        st, out = self.try_frame_save_rects(desc, rects, colour, out, bytes_per_row, True)
        self._chk(st, "frame_save_rects")
        return out

    def frame_save_rects_async(self, desc, rects, colour=None, out=None, bytes_per_row=None):
        """... without the final wait (sync() or a mark before `out` is read)"""
        st, out = self.try_frame_save_rects(desc, rects, colour, out, bytes_per_row, False)
        self._chk(st, "frame_save_rects_async")
        return out

    def try_stage_save_rects(self, desc, planes, rects, colour=None, origin=(0, 0), out=None, bytes_per_row=None,
                             size=None, stride=None):
        """jxlh_stage_save_rects on 3 + num_ec planes, as try_stage_save with the row band replaced by `rects`"""
        if size is None:
            pl = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
            h, w = pl[0].shape
            stride = w
        else:
            pl = list(planes)
            w, h = size
            stride = w if stride is None else stride
        if out is None:
            out = np.zeros(self.save_shape(desc, w, h), dtype=self._save_dtype(desc))
        if bytes_per_row is None:
            bytes_per_row = out.strides[0]
        r, n = _rect_array(rects)
        pp = (C.c_void_p * len(pl))(*[_addr(a).value for a in pl])
        st = self.L.jxlh_stage_save_rects(self._ctx, None if colour is None else C.byref(colour), C.byref(desc), pp, len(pl),
                                          w, h, stride, int(origin[0]), int(origin[1]), _addr(r) if n else None, n,
                                          _addr(out), int(bytes_per_row))
        return st, out

    def stage_save_rects(self, desc, planes, rects, colour=None, origin=(0, 0), out=None, bytes_per_row=None, size=None,
                         stride=None):
        st, out = self.try_stage_save_rects(desc, planes, rects, colour, origin, out, bytes_per_row, size, stride)
        self._chk(st, "stage_save_rects")
        return out

    # ---- LF frames ----
    def try_set_lf_frame(self, slot, x, y, b, w=None, h=None, stride=None):
        """jxlh_ctx_set_lf_frame, returning the status.  x, y, b: host arrays (2-D, rows contiguous, any row pitch), or
        DeviceArrays / raw device pointers with w, h and stride (floats)"""
        (x, y, b), w, h, stride = _rect_planes((x, y, b), np.float32, w, h, stride)
        return self.L.jxlh_ctx_set_lf_frame(self._ctx, int(slot), w, h, _addr(x), _addr(y), _addr(b), stride)

    def set_lf_frame(self, slot, x, y, b, w=None, h=None, stride=None):
        """LF slot `slot` <- the X, Y, B planes of an LF frame decoded elsewhere"""
        self._chk(self.try_set_lf_frame(slot, x, y, b, w, h, stride), "ctx_set_lf_frame")

    def try_save_lf(self, slot):
        return self.L.jxlh_frame_save_lf(self._ctx, int(slot))

    def save_lf(self, slot):
        """jxlh_frame_save_lf: LF slot `slot` (= the frame's lf_level - 1) <- the rendered frame's colour planes"""
        self._chk(self.try_save_lf(slot), "frame_save_lf")

    def clear_lf_frame(self, slot):
        self._chk(self.L.jxlh_ctx_clear_lf_frame(self._ctx, int(slot)), "ctx_clear_lf_frame")

    def try_set_lf_from_slot(self, slot):
        return self.L.jxlh_frame_set_lf_from_slot(self._ctx, int(slot))

    def set_lf_from_slot(self, slot):
        """jxlh_frame_set_lf_from_slot: the current VarDCT frame's LF image <- a copy of LF slot `slot` (= the frame's
        lf_level); the frame then runs no adaptive LF smoothing"""
        self._chk(self.try_set_lf_from_slot(slot), "frame_set_lf_from_slot")

    def try_lf_preview(self, slot, image_w, image_h, desc, colour, rect=None, out=None, bytes_per_row=None, wait=True):
        """jxlh_lf_preview (_async when not `wait`), returning (status, out).  rect: (x0, y0, w, h) in LF pixels, the
        whole slot by default; out: None (a zeroed array of the oriented image's samples is made), a numpy array, or a
        device pointer / DeviceArray with bytes_per_row given"""
        if rect is None:
            rect = (0, 0, (image_w + 7) // 8, (image_h + 7) // 8)
        if out is None:
            out = np.zeros(self.save_shape(desc, image_w, image_h), dtype=self._save_dtype(desc))
        if bytes_per_row is None:
            bytes_per_row = out.strides[0]
        fn = self.L.jxlh_lf_preview if wait else self.L.jxlh_lf_preview_async
        st = fn(self._ctx, int(slot), int(image_w), int(image_h), *[int(v) for v in rect],
                None if colour is None else C.byref(colour), None if desc is None else C.byref(desc), _addr(out),
                int(bytes_per_row))
        return st, out

    def lf_preview(self, slot, image_w, image_h, desc, colour, rect=None, out=None, bytes_per_row=None, wait=True):
        """the full-size preview of LF slot `slot`: Upsample8x, colour stage, conversion and oriented interleaved save
        of one rect in one pass"""
        st, out = self.try_lf_preview(slot, image_w, image_h, desc, colour, rect, out, bytes_per_row, wait)
        self._chk(st, "lf_preview")
        return out

    def tune_placement(self, trials=0):
        """jxlh_ctx_tune_placement: trials > 0 sets the number of candidate sets the next first allocation of the large
        buffers is picked from; returns (ratings [(k1-like ms, filter-like ms), ...] of the last pick, index taken)"""
        rep = np.zeros(128, np.float32)
        n, pick = C.c_int32(0), C.c_int32(-1)
        self._chk(self.L.jxlh_ctx_tune_placement(self._ctx, int(trials), _addr(rep), rep.size, C.byref(n), C.byref(pick)),
                  "ctx_tune_placement")
        return [(float(rep[2 * i]), float(rep[2 * i + 1])) for i in range(min(n.value, rep.size) // 2)], pick.value

    def probe_placement(self):
        """jxlh_probe_placement: (k1-like ms, filter-like ms) of two byte movers on the context's own buffers"""
        a, b = C.c_float(), C.c_float()
        self._chk(self.L.jxlh_probe_placement(self._ctx, C.byref(a), C.byref(b)), "probe_placement")
        return a.value, b.value

    def k1_counters(self):
        """jxlh_frame_k1_counters: dict of the last transform launch's work-list counters"""
        out = np.zeros(29, np.int32)
        self._chk(self.L.jxlh_frame_k1_counters(self._ctx, _addr(out), 29), "frame_k1_counters")
        names = ["dct8", "dct16x8", "dct8x16", "dct16x16", "dct32x8", "dct8x32", "dct32x16", "dct16x32", "dct32x32"]
        # varblocks per batch (Shape::NB) of the entries form, which the fallback counters belong to; dense slabs run the
        # classes with a 32-point side at half of it
        nb = [8, 8, 8, 4, 4, 8, 4, 4, 2]
        return {"varblocks": {k: int(v) for k, v in zip(names + ["special", "large"], out[:11])},
                "fallback_batches": {k: int(v) for k, v in zip(names, out[11:20])},
                "batches": {k: int(-(-int(v) // b)) for k, v, b in zip(names, out[:9], nb)},
                "dense_route_varblocks": {k: int(v) for k, v in zip(names, out[20:29])}}

    def frame_path(self):
        """(strip kernel ran, 64x64 tiles of the frame, tiles left to the transform class kernels) of the last frame_run"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self.L.jxlh_frame_path(self._ctx, C.byref(a), C.byref(b), C.byref(c)), "frame_path")
        return bool(a.value), int(b.value), int(c.value)

    # ---- multi-GPU (one process per GPU: RCCL communicator owned by the library)
    def comm_init(self, unique_id, rank, nranks):
        """unique_id: the 128 bytes rank 0 obtained from comm_unique_id() and the launcher distributed"""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._chk(self.L.jxlh_comm_init(self._ctx, buf, rank, nranks), "comm_init")

    def comm_destroy(self):
        self._chk(self.L.jxlh_comm_destroy(self._ctx), "comm_destroy")

    def comm_band(self):
        """(rank, nranks, group_row0, group_row1) of this context inside the current frame"""
        r, n, a, b = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.jxlh_comm_band(self._ctx, C.byref(r), C.byref(n), C.byref(a), C.byref(b)), "comm_band")
        return r.value, n.value, a.value, b.value

    def frame_run_sharded(self):
        self._chk(self.L.jxlh_frame_run_sharded(self._ctx), "frame_run_sharded")

    def frame_allgather(self):
        self._chk(self.L.jxlh_frame_allgather(self._ctx), "frame_allgather")

    def comm_allgather(self, dev_ptr, bytes_per_rank):
        self._chk(self.L.jxlh_comm_allgather(self._ctx, _addr(dev_ptr), bytes_per_rank), "comm_allgather")

    @property
    def out_size(self):
        """(width, height) of what the jxlh_frame_read_* calls return: the frame, or its upsampled image, or the image
        the frame was blended onto"""
        if getattr(self, "_blend_size", None):
            return self._blend_size
        p = self.params
        n = max(1, p.upsampling)
        return (p.xsize_upsampled or p.xsize * n, p.ysize_upsampled or p.ysize * n)

    def read_planes(self):
        w, h = self.out_size
        out = [np.zeros((h, w), dtype=np.float32) for _ in range(3)]
        planes = (Plane * 3)(*[Plane(o.ctypes.data, w * 4, h, w * 4) for o in out])
        self._chk(self.L.jxlh_frame_read_planes(self._ctx, planes), "frame_read_planes")
        return out

    def read_planes_rect(self, x0, y0, w, h, out=None):
        """jxlh_frame_read_planes_rect: the rect [x0, x0 + w) x [y0, y0 + h) of the three finished planes (cut at the
        result's edge) into `out` (three float32 arrays of at least the cut size; allocated h x w, zeroed, when None)"""
        if out is None:
            out = [np.zeros((h, w), dtype=np.float32) for _ in range(3)]
        planes = (Plane * 3)(*[Plane(o.ctypes.data, o.shape[1] * 4, o.shape[0], o.strides[0]) for o in out])
        self._chk(self.L.jxlh_frame_read_planes_rect(self._ctx, x0, y0, w, h, planes), "frame_read_planes_rect")
        return out

    def read_group_planes(self, group_id):
        """the reference's unit of hand-over (RenderPipeline::set_buffer_for_group, render/mod.rs:128-137): group
        `group_id` of the result on the 256 x 256 grid, in buffers rounded up to 16 pixels
        (group_size_for_channel, render/internal.rs:144-167); returns (planes, (w, h) of the group's part of the frame)"""
        W, H = self.out_size
        xg = (W + 255) // 256
        x0, y0 = (group_id % xg) * 256, (group_id // xg) * 256
        gw, gh = min(256, W - x0), min(256, H - y0)
        bw, bh = (min(256, W) + 15) // 16 * 16, (min(256, H) + 15) // 16 * 16
        out = [np.zeros((bh, bw), dtype=np.float32) for _ in range(3)]
        self.read_planes_rect(x0, y0, bw, bh, out)
        return out, (gw, gh)

    def read_rgb8(self, xyb_params, channels=3, y0=0, y1=None, out=None):
        """8-bit interleaved sRGB of rows [y0, y1) (jxlh_frame_read_rgb8).  xyb_params: 16 floats in
        jxlh_xyb_params order.  out: optional device pointer (int) with tight rows; else a numpy array is returned."""
        pr = np.ascontiguousarray(xyb_params, dtype=np.float32)
        assert pr.size == 16
        y1 = self.out_size[1] if y1 is None else y1
        if out is not None:
            self._chk(self.L.jxlh_frame_read_rgb8(self._ctx, _addr(pr), channels, y0, y1, C.c_void_p(int(out)),
                                                  self.out_size[0] * channels), "frame_read_rgb8")
            return None
        arr = np.zeros((y1 - y0, self.out_size[0], channels), dtype=np.uint8)
        self._chk(self.L.jxlh_frame_read_rgb8(self._ctx, _addr(pr), channels, y0, y1, _addr(arr),
                                              self.out_size[0] * channels), "frame_read_rgb8")
        return arr

    def read_rgb16(self, xyb_params, channels=3, y0=0, y1=None):
        """16-bit interleaved sRGB of rows [y0, y1) (jxlh_frame_read_rgb16) as a uint16 array."""
        pr = np.ascontiguousarray(xyb_params, dtype=np.float32)
        assert pr.size == 16
        y1 = self.out_size[1] if y1 is None else y1
        arr = np.zeros((y1 - y0, self.out_size[0], channels), dtype=np.uint16)
        self._chk(self.L.jxlh_frame_read_rgb16(self._ctx, _addr(pr), channels, y0, y1, _addr(arr),
                                               self.out_size[0] * channels * 2), "frame_read_rgb16")
        return arr

    @staticmethod
    def output_desc(color=COLOR_XYB, transfer="srgb", xyb_params=None, tf_param=0.0, lum=(0.2627, 0.678, 0.0593), bits=8,
                    channels=3):
        d = OutputDesc()
        d.color, d.transfer, d.bits, d.channels, d.tf_param = color, TF[transfer], bits, channels, tf_param
        if xyb_params is not None:
            d.xyb = XybParams.from_buffer_copy(np.ascontiguousarray(xyb_params, dtype=np.float32))
        for i in range(3):
            d.hlg_luminance_rgb[i] = lum[i]
        return d

    def frame_allgather_output(self, desc, out_ptr, bytes_per_row):
        """jxlh_frame_allgather_output: this rank's band converted into the device image at out_ptr, bands all-gathered"""
        self._chk(self.L.jxlh_frame_allgather_output(self._ctx, C.byref(desc), out_ptr, bytes_per_row), "frame_allgather_output")

    def read_output(self, color=COLOR_XYB, transfer="srgb", xyb_params=None, tf_param=0.0, lum=(0.2627, 0.678, 0.0593),
                    bits=8, channels=3, y0=0, y1=None):
        """jxlh_frame_read_output: interleaved 8- or 16-bit samples after the frame's colour stage"""
        d = self.output_desc(color, transfer, xyb_params, tf_param, lum, bits, channels)
        w, h = self.out_size
        y1 = h if y1 is None else y1
        arr = np.zeros((y1 - y0, w, channels), dtype=np.uint8 if bits == 8 else np.uint16)
        self._chk(self.L.jxlh_frame_read_output(self._ctx, C.byref(d), y0, y1, _addr(arr), w * channels * (bits // 8)),
                  "frame_read_output")
        return arr

    def read_ycbcr_rgb8(self, channels=3, y0=0, y1=None):
        """8-bit interleaved RGB of a YCbCr frame (planes Cb, Y, Cr; jxlh_frame_read_ycbcr_rgb8)."""
        y1 = self.out_size[1] if y1 is None else y1
        arr = np.zeros((y1 - y0, self.out_size[0], channels), dtype=np.uint8)
        self._chk(self.L.jxlh_frame_read_ycbcr_rgb8(self._ctx, channels, y0, y1, _addr(arr),
                                                    self.out_size[0] * channels), "frame_read_ycbcr_rgb8")
        return arr

    def read_ycbcr_rgb16(self, channels=3, y0=0, y1=None):
        y1 = self.out_size[1] if y1 is None else y1
        arr = np.zeros((y1 - y0, self.out_size[0], channels), dtype=np.uint16)
        self._chk(self.L.jxlh_frame_read_ycbcr_rgb16(self._ctx, channels, y0, y1, _addr(arr),
                                                     self.out_size[0] * channels * 2), "frame_read_ycbcr_rgb16")
        return arr

    def device_planes(self):
        ptrs = (C.c_void_p * 3)()
        stride = C.c_size_t()
        self._chk(self.L.jxlh_frame_device_planes(self._ctx, ptrs, C.byref(stride)), "frame_device_planes")
        return [ptrs[i] for i in range(3)], stride.value

    def read_lf(self):
        out = [np.zeros((self.yblocks, self.xblocks), dtype=np.float32) for _ in range(3)]
        self._chk(self.L.jxlh_frame_read_lf(self._ctx, _addr(out[0]), _addr(out[1]), _addr(out[2]), self.xblocks),
                  "frame_read_lf")
        return out

    # ---- timing ----
    def timer_start(self):
        self._chk(self.L.jxlh_timer_start(self._ctx), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.jxlh_timer_stop(self._ctx, C.byref(ms)), "timer_stop")
        return ms.value

    def kernel_timing(self, enable):
        self._chk(self.L.jxlh_kernel_timing_enable(self._ctx, 1 if enable else 0), "kernel_timing_enable")

    def kernel_timing_reset(self):
        self._chk(self.L.jxlh_kernel_timing_reset(self._ctx), "kernel_timing_reset")

    def kernel_times(self):
        out = {}
        i = 0
        while True:
            name, ms, n = C.c_char_p(), C.c_float(), C.c_int32()
            st = self.L.jxlh_kernel_timing_get(self._ctx, i, C.byref(name), C.byref(ms), C.byref(n))
            if st != OK:
                break
            out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out

    # ---- stage hooks ----
    def selftest_recip(self, lo=1.0, hi=16.0):
        """Number of floats in [lo, hi) whose fast EPF reciprocal differs from IEEE 1/w."""
        lo_b = int(np.float32(lo).view(np.uint32))
        hi_b = int(np.float32(hi).view(np.uint32))
        bad = C.c_uint64(0)
        self._chk(self.L.jxlh_selftest_recip(self._ctx, C.c_uint32(lo_b), C.c_uint32(hi_b), C.byref(bad)),
                  "selftest_recip")
        return int(bad.value)

    def flow_profile(self, enable=True):
        """timeline of the last dataflow squeeze launch (if profiling was on): a list of per-level dicts, times in us
        from the first level's start; then switches the profile on / off for the launches that follow"""
        n = C.c_int32(0)
        rows = (C.c_uint64 * (11 * 16))()
        self._chk(self.L.jxlh_flow_profile(self._ctx, 1 if enable else 0, C.byref(n), rows, 16), "flow_profile")
        if n.value == 0:
            return []
        t0 = min(rows[11 * i] for i in range(n.value))
        return [{"start_us": (rows[11 * i] - t0) / 100.0, "end_us": (rows[11 * i + 1] - t0) / 100.0,
                 "poll_wait_us_sum": rows[11 * i + 2] / 100.0, "polls": int(rows[11 * i + 3]),
                 "lifetime_us_sum": rows[11 * i + 4] / 100.0,
                 "mover_phases_us_sum": [rows[11 * i + 5 + k] / 100.0 for k in range(6)]} for i in range(n.value)]

    def stage_gaborish(self, plane, w1, w2, w=None, h=None):
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        H, S = plane.shape
        w = S if w is None else w
        h = H if h is None else h
        out = np.zeros_like(plane)
        self._chk(self.L.jxlh_stage_gaborish(self._ctx, _addr(plane), _addr(out), w, h, S, w1, w2), "stage_gaborish")
        return out

    def stage_epf(self, stage, params, planes, inv_sigma, w=None, h=None):
        planes = [np.ascontiguousarray(a, dtype=np.float32) for a in planes]
        H, S = planes[0].shape
        w = S if w is None else w
        h = H if h is None else h
        sig = np.ascontiguousarray(inv_sigma, dtype=np.float32)
        out = [np.zeros_like(planes[0]) for _ in range(3)]
        pin = (C.c_void_p * 3)(*[a.ctypes.data for a in planes])
        pout = (C.c_void_p * 3)(*[a.ctypes.data for a in out])
        self._chk(self.L.jxlh_stage_epf(self._ctx, stage, C.byref(params), pin, pout, w, h, S, _addr(sig),
                                        sig.shape[1]), "stage_epf")
        return out

    def stage_lf_smooth(self, params, lf):
        lf = [np.ascontiguousarray(a, dtype=np.float32) for a in lf]
        h, w = lf[0].shape
        out = [np.zeros_like(lf[0]) for _ in range(3)]
        pin = (C.c_void_p * 3)(*[a.ctypes.data for a in lf])
        pout = (C.c_void_p * 3)(*[a.ctypes.data for a in out])
        self._chk(self.L.jxlh_stage_lf_smooth(self._ctx, C.byref(params), pin, pout, w, h), "stage_lf_smooth")
        return out

    def set_upsampling_weights(self, w2=None, w4=None, w8=None):
        arrs = [None if w is None else np.ascontiguousarray(w, dtype=np.float32) for w in (w2, w4, w8)]
        for a, n in zip(arrs, (15, 55, 210)):
            assert a is None or a.size == n
        self._chk(self.L.jxlh_set_upsampling_weights(self._ctx, *[None if a is None else _addr(a) for a in arrs]),
                  "set_upsampling_weights")

    def stage_upsample(self, n, plane):
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        h, w = plane.shape
        out = np.zeros((h * n, w * n), dtype=np.float32)
        self._chk(self.L.jxlh_stage_upsample(self._ctx, n, _addr(plane), _addr(out), w, h), "stage_upsample")
        return out

    def stage_noise_generate(self, visible, nonvisible, w, h):
        out = [np.zeros((h, w), dtype=np.float32) for _ in range(3)]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in out])
        self._chk(self.L.jxlh_stage_noise_generate(self._ctx, visible, nonvisible, w, h, ptrs), "stage_noise_generate")
        return out

    def stage_noise_convolve(self, plane):
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        h, w = plane.shape
        out = np.zeros_like(plane)
        self._chk(self.L.jxlh_stage_noise_convolve(self._ctx, _addr(plane), _addr(out), w, h), "stage_noise_convolve")
        return out

    def stage_noise_add(self, params, planes, rnd):
        pl = [np.ascontiguousarray(a, dtype=np.float32).copy() for a in planes]
        rn = [np.ascontiguousarray(a, dtype=np.float32) for a in rnd]
        pp = (C.c_void_p * 3)(*[a.ctypes.data for a in pl])
        pr = (C.c_void_p * 3)(*[a.ctypes.data for a in rn])
        self._chk(self.L.jxlh_stage_noise_add(self._ctx, C.byref(params), pp, pr, pl[0].size), "stage_noise_add")
        return pl

    def stage_chroma_upsample(self, plane, horizontal):
        plane = np.ascontiguousarray(plane, dtype=np.float32)
        h, w = plane.shape
        out = np.zeros((h, 2 * w) if horizontal else (2 * h, w), dtype=np.float32)
        self._chk(self.L.jxlh_stage_chroma_upsample(self._ctx, _addr(plane), _addr(out), w, h, 1 if horizontal else 0),
                  "stage_chroma_upsample")
        return out

    def stage_transform_to_pixels(self, ttype, coeffs, lf):
        """coeffs [n, cx*cy*64], lf [n, cx*cy] -> pixels [n, cy*8, cx*8]."""
        cx, cy = self.L.jxlh_covered_blocks_x(ttype), self.L.jxlh_covered_blocks_y(ttype)
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float32).reshape(-1, cx * cy * 64)
        lf = np.ascontiguousarray(lf, dtype=np.float32).reshape(-1, cx * cy)
        n = coeffs.shape[0]
        assert lf.shape[0] == n
        out = np.zeros((n, cy * 8, cx * 8), dtype=np.float32)
        self._chk(self.L.jxlh_stage_transform_to_pixels(self._ctx, ttype, n, _addr(coeffs), _addr(lf), _addr(out)),
                  "stage_transform_to_pixels")
        return out

    # ---- modular ----
    def rct(self, planes, op, perm):
        ps = [np.ascontiguousarray(a, dtype=np.int32).copy() for a in planes]
        self._chk(self.L.jxlh_rct(self._ctx, _addr(ps[0]), _addr(ps[1]), _addr(ps[2]), ps[0].size, op, perm), "rct")
        return ps

    def palette(self, index, palette, num_colors, nb_channels, bit_depth):
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pal = np.ascontiguousarray(palette, dtype=np.int32)
        out = np.zeros((nb_channels,) + idx.shape, dtype=np.int32)
        self._chk(self.L.jxlh_palette(self._ctx, _addr(idx), idx.size, _addr(pal), num_colors, pal.shape[1],
                                      nb_channels, bit_depth, _addr(out)), "palette")
        return out

    def modular_to_rgb8(self, planes, multiplier, maxv, channels=3):
        pl = [np.ascontiguousarray(a, dtype=np.int32) for a in planes]
        h, w = pl[0].shape
        out = np.zeros((h, w, channels), dtype=np.uint8)
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data for a in pl])
        self._chk(self.L.jxlh_modular_to_rgb8(self._ctx, ptrs, w, w, h, multiplier, maxv, channels, _addr(out), w * channels),
                  "modular_to_rgb8")
        return out

    def modular_to_f32(self, plane, bits, exp_bits=0):
        a = np.ascontiguousarray(plane, dtype=np.int32)
        out = np.zeros(a.shape, dtype=np.float32)
        self._chk(self.L.jxlh_modular_to_f32(self._ctx, _addr(a), a.size, bits | exp_bits << 8, _addr(out)), "modular_to_f32")
        return out

    def modular_xyb_to_f32(self, y, x, b, quant_factors):
        y, x, b = [np.ascontiguousarray(v, dtype=np.int32) for v in (y, x, b)]
        q = np.ascontiguousarray(quant_factors, dtype=np.float32)
        out = [np.zeros(y.shape, dtype=np.float32) for _ in range(3)]
        self._chk(self.L.jxlh_modular_xyb_to_f32(self._ctx, _addr(y), _addr(x), _addr(b), y.size, _addr(q),
                                                 *[_addr(o) for o in out]), "modular_xyb_to_f32")
        return out

    def palette_delta(self, index, palette, num_colors, num_deltas, bit_depth, predictor):
        """index [h, w]; palette [nb_channels, >= num_colors + num_deltas] -> [nb_channels, h, w] (jxlh_palette_delta)"""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pal = np.ascontiguousarray(palette, dtype=np.int32)
        h, w = idx.shape
        out = np.zeros((pal.shape[0], h, w), dtype=np.int32)
        self._chk(self.L.jxlh_palette_delta(self._ctx, _addr(idx), w, h, _addr(pal), num_colors, num_deltas, pal.shape[1],
                                            pal.shape[0], bit_depth, predictor, _addr(out)), "palette_delta")
        return out

    def palette_delta_wp(self, index, palette, num_colors, num_deltas, bit_depth, wp_header):
        """The Weighted-predictor branch of the palette step; wp_header = (p1c, p2c, p3ca..p3ce, w0..w3)."""
        idx = np.ascontiguousarray(index, dtype=np.int32)
        pal = np.ascontiguousarray(palette, dtype=np.int32)
        hdr = np.ascontiguousarray(wp_header, dtype=np.uint32)
        assert hdr.size == 11
        h, w = idx.shape
        out = np.zeros((pal.shape[0], h, w), dtype=np.int32)
        self._chk(self.L.jxlh_palette_delta_wp(self._ctx, _addr(idx), w, h, _addr(pal), num_colors, num_deltas,
                                               pal.shape[1], pal.shape[0], bit_depth, _addr(hdr), _addr(out)),
                  "palette_delta_wp")
        return out

    def unsqueeze_planes(self, horizontal, avg, res, out, out_w, out_h, avg_stride, res_stride, out_stride):
        """Device-resident batched step: avg/res/out are lists (<= 3) of device pointers / tensors."""
        n = len(avg)
        av = (C.c_void_p * n)(*[_addr(a).value for a in avg])
        rv = (C.c_void_p * n)(*[_addr(a).value for a in res])
        ov = (C.c_void_p * n)(*[_addr(a).value for a in out])
        self._chk(self.L.jxlh_unsqueeze_planes(self._ctx, 1 if horizontal else 0, n, av, avg_stride, rv, res_stride,
                                               out_w, out_h, ov, out_stride), "unsqueeze_planes")

    def unsqueeze_levels(self, levels, base, base_stride, base_w, base_h, out, out_stride):
        """Several squeeze steps in one call (device-resident): levels = [(horizontal, out_w, out_h, [res planes],
        res_stride)], base / out = lists of n_planes device pointers."""
        n_planes = len(base)
        arr = (SqueezeLevel * len(levels))()
        for i, (hz, ow, oh, res, rstride) in enumerate(levels):
            arr[i].horizontal = 1 if hz else 0
            arr[i].out_w, arr[i].out_h = ow, oh
            for p in range(3):
                arr[i].res[p] = _addr(res[p]).value if p < n_planes and res[p] is not None else None
            arr[i].res_stride = rstride
        bv = (C.c_void_p * n_planes)(*[_addr(a).value for a in base])
        ov = (C.c_void_p * n_planes)(*[_addr(a).value for a in out])
        self._chk(self.L.jxlh_unsqueeze_levels(self._ctx, n_planes, len(levels), C.cast(arr, C.c_void_p), bv, base_stride,
                                               base_w, base_h, ov, out_stride), "unsqueeze_levels")

    def unsqueeze_chain(self, levels, base, base_stride, base_w, base_h, out, out_stride, rct=None):
        """The inverse of a whole squeeze transform (+ the RCT after it, rct = (op, perm)) in one call; arguments as
        unsqueeze_levels."""
        n_planes = len(base)
        arr = (SqueezeLevel * len(levels))()
        for i, (hz, ow, oh, res, rstride) in enumerate(levels):
            arr[i].horizontal = 1 if hz else 0
            arr[i].out_w, arr[i].out_h = ow, oh
            for p in range(3):
                arr[i].res[p] = _addr(res[p]).value if p < n_planes and res[p] is not None else None
            arr[i].res_stride = rstride
        bv = (C.c_void_p * n_planes)(*[_addr(a).value for a in base])
        ov = (C.c_void_p * n_planes)(*[_addr(a).value for a in out])
        op, perm = rct if rct is not None else (-1, 0)
        self._chk(self.L.jxlh_unsqueeze_chain(self._ctx, n_planes, len(levels), C.cast(arr, C.c_void_p), bv, base_stride,
                                              base_w, base_h, ov, out_stride, op, perm), "unsqueeze_chain")

    def unsqueeze_chain_preview(self, levels, base, base_stride, base_w, base_h, out, out_stride, rct=None, cvt_rne=False,
                                flags=None):
        """A progressive preview of a whole squeeze transform in one call (jxlh_unsqueeze_chain_preview): arguments as
        unsqueeze_chain; a level whose residual planes are all None has not arrived and runs the reference's smooth
        step (squeeze_preview_kinds says which).  cvt_rne: the x86 reference builds' float-to-int conversion."""
        n_planes = len(base)
        arr = _squeeze_levels(levels, n_planes)
        bv = (C.c_void_p * n_planes)(*[_addr(a).value for a in base])
        ov = (C.c_void_p * n_planes)(*[_addr(a).value for a in out])
        op, perm = rct if rct is not None else (-1, 0)
        if flags is None:
            flags = self.SMOOTH_CVT_NEAREST_EVEN if cvt_rne else 0
        self._chk(self.L.jxlh_unsqueeze_chain_preview(self._ctx, n_planes, len(levels), C.cast(arr, C.c_void_p), bv,
                                                      base_stride, base_w, base_h, ov, out_stride, op, perm, flags),
                  "unsqueeze_chain_preview")

    def unsqueeze_chain_preview_tiles(self, levels, tiles, base, base_stride, base_w, base_h, out, out_stride, rct=None,
                                      cvt_rne=False, flags=None):
        """A progressive preview per grid cell in one call (jxlh_unsqueeze_chain_preview_tiles): arguments as
        unsqueeze_chain_preview plus tiles = [(tile_w, tile_h, present)] per level -- present None, or a [tiles_y,
        tiles_x] array that is non-zero where the cell's residual samples have arrived (squeeze_tile_kinds says what
        each cell runs).  The residual planes of a partly arrived level are whole planes; samples of missing cells are
        not read."""
        n_planes = len(base)
        arr = _squeeze_levels(levels, n_planes)
        tarr, keep = _squeeze_tiles(levels, tiles)
        bv = (C.c_void_p * n_planes)(*[_addr(a).value for a in base])
        ov = (C.c_void_p * n_planes)(*[_addr(a).value for a in out])
        op, perm = rct if rct is not None else (-1, 0)
        if flags is None:
            flags = self.SMOOTH_CVT_NEAREST_EVEN if cvt_rne else 0
        self._chk(self.L.jxlh_unsqueeze_chain_preview_tiles(self._ctx, n_planes, len(levels), C.cast(arr, C.c_void_p),
                                                            C.cast(tarr, C.c_void_p), bv, base_stride, base_w, base_h, ov,
                                                            out_stride, op, perm, flags), "unsqueeze_chain_preview_tiles")

    def unsqueeze_rct(self, horizontal, avg, res, out, out_w, out_h, avg_stride, res_stride, out_stride, op, perm):
        """Unsqueeze of three device-resident planes fused with the inverse RCT on them."""
        av = (C.c_void_p * 3)(*[_addr(a).value for a in avg])
        rv = (C.c_void_p * 3)(*[_addr(a).value for a in res])
        ov = (C.c_void_p * 3)(*[_addr(a).value for a in out])
        self._chk(self.L.jxlh_unsqueeze_rct(self._ctx, 1 if horizontal else 0, av, avg_stride, rv, res_stride, out_w,
                                            out_h, ov, out_stride, op, perm), "unsqueeze_rct")

    SMOOTH_H, SMOOTH_V, SMOOTH_2D = 0, 1, 2
    SMOOTH_CVT_NEAREST_EVEN = 0x100  # the x86 back-ends' as_i32 (cvtps2dq) instead of truncation

    def smooth_unsqueeze(self, kind, avg, out_w, out_h, x0=0, y0=0, out=None, cvt_rne=False):
        """smooth_{h,v,2d}_unsqueeze (squeeze.rs:908-1225): `avg` the whole average channel, host array."""
        kind |= self.SMOOTH_CVT_NEAREST_EVEN if cvt_rne else 0
        avg = np.ascontiguousarray(avg, dtype=np.int32)
        if out is None:
            out = np.zeros((out_h, out_w), dtype=np.int32)
        self._chk(self.L.jxlh_smooth_unsqueeze(self._ctx, kind, _addr(avg), avg.shape[1], avg.shape[1], avg.shape[0],
                                               x0, y0, _addr(out), out.shape[1], out_w, out_h), "smooth_unsqueeze")
        return out

    def smooth_unsqueeze_dev(self, kind, avg, avg_stride, avg_w, avg_h, out, out_stride, out_w, out_h, x0=0, y0=0):
        """Device-resident form (pointers / DeviceArray / tensors)."""
        self._chk(self.L.jxlh_smooth_unsqueeze(self._ctx, kind, _addr(avg), avg_stride, avg_w, avg_h, x0, y0,
                                               _addr(out), out_stride, out_w, out_h), "smooth_unsqueeze")

    def unsqueeze(self, horizontal, avg, res, out_w, out_h):
        avg = np.ascontiguousarray(avg, dtype=np.int32)
        res = np.ascontiguousarray(res, dtype=np.int32)
        out = np.zeros((out_h, out_w), dtype=np.int32)
        self._chk(self.L.jxlh_unsqueeze(self._ctx, 1 if horizontal else 0, _addr(avg), avg.shape[1],
                                        _addr(res) if res.size else None, max(res.shape[1], 1) if res.ndim == 2 else 1,
                                        out_w, out_h, _addr(out), out_w), "unsqueeze")
        return out
