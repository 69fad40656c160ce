"""Shared helpers for the parity tests: run the same workload through the CPU oracle and
through the HIP path (via the C ABI), and forward-squeeze for round-trip properties."""
import os
import subprocess

import numpy as np


def c_struct_layouts(tmp_path, structs):
    """What the C compiler lays out for structs of include/jxl_hip.h.  structs: {C name: [field names]}; returns
    {(C name, "size"): sizeof, (C name, field): offsetof, (C name, field + ".size"): the field's sizeof}.  The yardstick of the generated bindings' layout tests."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "jxl_hip.h"', "int main(void) {"]
    for n, fields in structs.items():
        lines.append(f'  printf("{n} size %zu\\n", sizeof({n}));')
        for f in fields:
            lines.append(f'  printf("{n} {f} %zu\\n", offsetof({n}, {f}));')
            lines.append(f'  printf("{n} {f}.size %zu\\n", sizeof((({n}*)0)->{f}));')
    lines +=["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-std=c99", "-I", include, str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        n, f, v = ln.split()
        got[(n, f)] = int(v)
    return got


def _set_shifts(p, wl):
    for c in range(3):
        p.hshift[c] = wl.opts.get("hshift", (0, 0, 0))[c]
        p.vshift[c] = wl.opts.get("vshift", (0, 0, 0))[c]


def is_subsampled(wl):
    return any(wl.opts.get("hshift", (0, 0, 0))) or any(wl.opts.get("vshift", (0, 0, 0)))


def oracle_params_from(o, wl, **over):
    p = o.default_params(wl.xsize, wl.ysize)
    p.epf_iters = wl.opts.get("epf_iters", 2)
    p.gab = 1 if wl.opts.get("gab", True) else 0
    p.do_lf_smoothing = 1 if wl.opts.get("lf_smoothing", True) else 0
    _set_shifts(p, wl)
    p.xsize_blocks, p.ysize_blocks = wl.xblocks, wl.yblocks
    for k, v in over.items():
        setattr(p, k, v)
    return p


def gpu_params_from(ctx, wl, **over):
    p = ctx.default_params(wl.xsize, wl.ysize)
    p.epf_iters = wl.opts.get("epf_iters", 2)
    p.gab = 1 if wl.opts.get("gab", True) else 0
    p.do_lf_smoothing = 1 if wl.opts.get("lf_smoothing", True) else 0
    _set_shifts(p, wl)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def run_oracle_frame(o, wl, num_threads=8, tables=None, lf=None, **over):
    """Whole chain on the CPU oracle.  Returns (planes cropped to the frame, smoothed LF).  lf: the dequantised LF
    (X, Y, B) to use instead of dequantising wl.lf_q whole (a test that dequantises rect by rect stitches it)."""
    p = oracle_params_from(o, wl, **over)
    if lf is not None:
        lf = [np.ascontiguousarray(a, dtype=np.float32) for a in lf]
    elif is_subsampled(wl):  # no chroma-from-luma; channel c <- its own coded plane (Y, X, B order in lf_q)
        lf = [o.dequant_lf_channel(p, 0, wl.lf_q[1]), o.dequant_lf_channel(p, 1, wl.lf_q[0]),
              o.dequant_lf_channel(p, 2, wl.lf_q[2])]
    else:
        lf = o.dequant_lf(p, *wl.lf_q)
    tables = wl.tables if tables is None else tables
    planes, lf_sm = o.vardct_frame(p, wl.coeffs, wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob, lf,
                                   tables, num_threads=num_threads)
    return [pl[:wl.ysize, :wl.xsize].copy() for pl in planes], lf_sm


def upload_frame(ctx, wl, **over):
    p = gpu_params_from(ctx, wl, **over)
    ctx.frame_begin(p)
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    return p


def run_gpu_frame(ctx, wl, **over):
    upload_frame(ctx, wl, **over)
    ctx.frame_run()
    ctx.sync()
    return ctx.read_planes(), ctx.read_lf()


# ---- frames assembled rect by rect (tests/test_gpu_frame_assembly.py) ----
LF_GROUP_BLOCKS = 256  # an LF group is 256 x 256 blocks (2048 x 2048 pixels)
POISON = {np.dtype(np.int32): 0x7fffffff, np.dtype(np.float32): np.nan, np.dtype(np.uint8): 0xff, np.dtype(np.int8): 0x7f}


def lf_group_rects(xblocks, yblocks):
    """the rects (x0, y0, w, h) in blocks a decoder delivers: the LF-group grid, cut at the frame's edge"""
    n = LF_GROUP_BLOCKS
    return [(x, y, min(n, xblocks - x), min(n, yblocks - y)) for y in range(0, yblocks, n) for x in range(0, xblocks, n)]


def _cuts(rng, n, lo, hi, step=1):
    """cut points 0 = c0 < c1 < ... = n, multiples of `step` (except n), pieces between lo and hi long; always holds a
    piece of the smallest length `step` when n allows one"""
    cuts, first = [0], True
    while cuts[-1] < n:
        d = step if (first and n > step) else int(rng.integers(lo, hi + 1))
        first = False
        cuts.append(min(n, cuts[-1] + max(step, d // step * step)))
    return cuts


def ragged_lf_rects(xblocks, yblocks, seed):
    """a seeded tiling of the frame into LF rects of any origin and size: bands of random height (one is a single
    block row), each cut into pieces of random width (one per band a single block column)"""
    rng = np.random.default_rng([0x4C46, seed, xblocks, yblocks])
    rects = []
    ys = _cuts(rng, yblocks, 1, max(2, yblocks // 3))
    for y0, y1 in zip(ys[:-1], ys[1:]):
        xs = _cuts(rng, xblocks, 1, max(2, xblocks // 2))
        rects += [(x0, y0, x1 - x0, y1 - y0) for x0, x1 in zip(xs[:-1], xs[1:])]
    return rects


def ragged_map_rects(xblocks, yblocks, seed):
    """a seeded tiling for jxlh_frame_set_hf_meta: origins are multiples of 8, and every rect reaches 1..7 blocks into
    its right and lower neighbours (cut at the frame's edge), so sizes are not multiples of 8 and neighbouring rects
    share a colour tile -- which carries the same value from either side, as both cut it from the whole-frame map"""
    rng = np.random.default_rng([0x4D41, seed, xblocks, yblocks])
    rects = []
    ys = _cuts(rng, yblocks, 8, max(16, yblocks // 2), step=8)
    for y0, y1 in zip(ys[:-1], ys[1:]):
        xs = _cuts(rng, xblocks, 8, max(16, xblocks // 2), step=8)
        for x0, x1 in zip(xs[:-1], xs[1:]):
            ex, ey = int(rng.integers(1, 8)), int(rng.integers(1, 8))
            rects.append((x0, y0, min(xblocks, x1 + ex) - x0, min(yblocks, y1 + ey) - y0))
    return rects


def rects_cover(rects, xblocks, yblocks):
    """how often each block of the frame is covered; raises if a rect leaves the frame"""
    n = np.zeros((yblocks, xblocks), dtype=np.int32)
    for x0, y0, w, h in rects:
        if x0 < 0 or y0 < 0 or w < 0 or h < 0 or x0 + w > xblocks or y0 + h > yblocks:
            raise ValueError(f"rect {(x0, y0, w, h)} leaves the {xblocks} x {yblocks} frame")
        n[y0:y0 + h, x0:x0 + w] += 1
    return n


def subsampled_corner_mask(wl, c):
    """bool [yblocks, xblocks]: the LF samples channel c (X, Y, B) of a sub-sampled frame holds -- the top-left
    (w >> hshift) x (h >> vshift) corner of each LF group's rect.  From the geometry alone."""
    hs, vs = wl.opts.get("hshift", (0, 0, 0))[c], wl.opts.get("vshift", (0, 0, 0))[c]
    m = np.zeros((wl.yblocks, wl.xblocks), dtype=bool)
    for x0, y0, w, h in lf_group_rects(wl.xblocks, wl.yblocks):
        m[y0:y0 + (h >> vs), x0:x0 + (w >> hs)] = True
    return m


def _padded(a, pad):
    """the rect `a` as a view into a wider array whose other columns hold a value that would show if read"""
    a = np.asarray(a)
    if pad <= 0:
        return np.ascontiguousarray(a)
    big = np.full((a.shape[0], a.shape[1] + pad), POISON[a.dtype], dtype=a.dtype)
    off = pad // 2
    big[:, off:off + a.shape[1]] = a
    return big[:, off:off + a.shape[1]]


def _as_device(views, keep):
    """the padded views' backing arrays on the device: (pointers to each rect's first sample, pitch in elements)"""
    from jxl_rs_amd.lib import DeviceArray
    ptrs = []
    for v in views:
        base = v.base if v.base is not None else v
        d = DeviceArray(base)
        keep.append(d)
        ptrs.append(d.ptr + (v.ctypes.data - base.ctypes.data))
    v = views[0]
    return ptrs, (v.strides[0] // v.itemsize if v.shape[0] > 1 else max(v.shape[1], 1))


def lf_piece(wl, rect, ep=0, low_bits=None):
    """the quantised LF of one rect (coded order Y, X, B) scaled by 1 << ep, so that dequantising it with
    mul = 1 / (1 << ep) gives the whole-frame values; low_bits (a Generator) adds a random value below 1 << ep to
    every sample: values only that rect's own mul dequantises right"""
    x0, y0, w, h = rect
    out = []
    for q in wl.lf_q:
        v = q[y0:y0 + h, x0:x0 + w].astype(np.int64) * (1 << ep)
        if low_bits is not None and ep:
            v = v + low_bits.integers(0, 1 << ep, size=v.shape)
        out.append(v.astype(np.int32))  # (wraps for the huge values a test puts where nobody may look)
    return out


def oracle_lf_piece(o, wl, pieces, ep=0, **over):
    """what the oracle dequantises one rect's quantised pieces (Y, X, B) to: X, Y, B"""
    p = oracle_params_from(o, wl, **over)
    mul = 1.0 / (1 << ep)
    if is_subsampled(wl):
        return [o.dequant_lf_channel(p, 0, pieces[1], mul), o.dequant_lf_channel(p, 1, pieces[0], mul),
                o.dequant_lf_channel(p, 2, pieces[2], mul)]
    return o.dequant_lf(p, *pieces, mul=mul)


def upload_frame_piecewise(ctx, wl, lf_rects, map_rects, *, order=None, pitch_pad=0, extra_precision=0,
                           lf_as_float=False, on_device=False, oracle=None, low_bits=None, begin=True, submit=True,
                           **over):
    """The workload through one setter call per rect.
      order ........... None: LF rects, then map rects, as listed; an int: a permutation of all calls seeded with it; a
                        list: indices into [LF rects..., map rects...]
      pitch_pad ....... every piece sits in an array that many columns wider, the other columns poisoned
      extra_precision . int or f(index, rect) -> 0..3 for the quantised LF rects (lf_piece)
      lf_as_float ..... bool or f(index, rect) -> bool: that rect's LF is dequantised by `oracle` and goes through
                        jxlh_frame_set_lf
      on_device ....... every piece is handed over as a device pointer
      low_bits ........ seed: see lf_piece; the LF truth is then the returned stitched image only
      begin, submit ... frame_begin + tables first / the groups (dense) after the rects
    Returns (params, lf): lf is the oracle's dequantised LF (X, Y, B) stitched from the delivered pieces in delivery
    order when `oracle` is given, else None."""
    calls = [("lf", i, r) for i, r in enumerate(lf_rects)] + [("map", i, r) for i, r in enumerate(map_rects)]
    if isinstance(order, (int, np.integer)):
        calls = [calls[i] for i in np.random.default_rng([0x4F52, int(order)]).permutation(len(calls))]
    elif order is not None:
        calls = [calls[i] for i in order]
    p = gpu_params_from(ctx, wl, **over)
    if begin:
        ctx.frame_begin(p)
        ctx.set_dequant_tables(wl.tables)
    pick = lambda v, i, r: v(i, r) if callable(v) else v
    lb = None if low_bits is None else np.random.default_rng([0x4C42, low_bits])
    stitched = [np.zeros((wl.yblocks, wl.xblocks), dtype=np.float32) for _ in range(3)] if oracle is not None else None
    for kind, i, rect in calls:
        x0, y0, w, h = rect
        keep = []
        if kind == "lf":
            ep = pick(extra_precision, i, rect)
            pieces = lf_piece(wl, rect, ep, lb)
            as_float = pick(lf_as_float, i, rect)
            if oracle is not None or as_float:  # (lf_as_float needs the oracle)
                deq = oracle_lf_piece(oracle, wl, pieces, ep, **over)
            if oracle is not None:
                for c in range(3):
                    stitched[c][y0:y0 + h, x0:x0 + w] = deq[c]
            if as_float:
                views, call, kw = [_padded(a, pitch_pad) for a in deq], ctx.set_lf, {}
            else:
                views, call, kw = [_padded(a, pitch_pad) for a in pieces], ctx.set_lf_quantized, dict(extra_precision=ep)
            if on_device:
                ptrs, stride = _as_device(views, keep)
                call(*ptrs, x0=x0, y0=y0, w=w, h=h, stride=stride, **kw)
            else:
                call(*views, x0=x0, y0=y0, **kw)
        else:
            cw, ch = (w + 7) // 8, (h + 7) // 8
            maps = [_padded(a[y0:y0 + h, x0:x0 + w], pitch_pad) for a in (wl.transform_map, wl.raw_quant, wl.epf_map)]
            cmaps = [_padded(a[y0 // 8:y0 // 8 + ch, x0 // 8:x0 // 8 + cw], pitch_pad) for a in (wl.ytox, wl.ytob)]
            if on_device:
                mp, ms = _as_device(maps, keep)
                cp, cs = _as_device(cmaps, keep)
                ctx.set_hf_meta(*mp, *cp, x0=x0, y0=y0, w=w, h=h, map_stride=ms, cmap_stride=cs)
            else:
                ctx.set_hf_meta(*maps, *cmaps, x0=x0, y0=y0)
        for d in keep:  # the setters return after their copies have landed
            d.free()
    if submit:
        for g in range(wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
    return p, stitched


def bit_equal(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff_report(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    bad = np.argwhere(np.asarray(a, dtype=np.float32).view(np.uint32) != np.asarray(b, dtype=np.float32).view(np.uint32))
    first = bad[:5].tolist()
    return f"max abs {d.max():.3e}, rmse {np.sqrt((d * d).mean()):.3e}, mismatches {len(bad)}/{a.size}, first {first}"


# ---- forward squeeze (encoder side; only used to build round-trip properties) ----
def _tendency(b, a, n):
    """smooth_tendency_scalar (squeeze.rs:143-168), vectorised over int64 arrays."""
    b = b.astype(np.int64)
    a = a.astype(np.int64)
    n = n.astype(np.int64)
    diff = np.zeros_like(a)
    up = (b >= a) & (a >= n)
    dn = (b <= a) & (a <= n) & ~up
    d1 = (4 * b - 3 * n - a + 6)
    d1 = np.where(d1 >= 0, d1 // 12, -((-d1) // 12))
    d1 = np.where(d1 - (d1 & 1) > 2 * (b - a), 2 * (b - a) + 1, d1)
    d1 = np.where(d1 + (d1 & 1) > 2 * (a - n), 2 * (a - n), d1)
    d2 = (4 * b - 3 * n - a - 6)
    d2 = np.where(d2 >= 0, d2 // 12, -((-d2) // 12))
    d2 = np.where(d2 + (d2 & 1) < 2 * (b - a), 2 * (b - a) - 1, d2)
    d2 = np.where(d2 - (d2 & 1) < 2 * (a - n), 2 * (a - n), d2)
    diff = np.where(up, d1, diff)
    diff = np.where(dn, d2, diff)
    return diff


def forward_squeeze_h(img):
    """img [h, w] int32 -> (avg [h, ceil(w/2)], res [h, floor(w/2)]) such that the decoder's
    horizontal unsqueeze reproduces img exactly."""
    img = img.astype(np.int64)
    h, w = img.shape
    nr = w // 2
    na = w - nr
    avg = np.zeros((h, na), dtype=np.int64)
    a = img[:, 0:2 * nr:2]
    b = img[:, 1:2 * nr:2]
    avg[:, :nr] = (a + b + (a > b)) >> 1
    if w & 1:
        avg[:, nr] = img[:, w - 1]
    res = np.zeros((h, nr), dtype=np.int64)
    for x in range(nr):
        prev = avg[:, 0] if x == 0 else img[:, 2 * x - 1]
        nxt = avg[:, x + 1] if x + 1 < na else avg[:, x]
        res[:, x] = (a[:, x] - b[:, x]) - _tendency(prev, avg[:, x], nxt)
    return avg.astype(np.int32), res.astype(np.int32)


def forward_squeeze_v(img):
    a, r = forward_squeeze_h(np.ascontiguousarray(img.T))
    return np.ascontiguousarray(a.T), np.ascontiguousarray(r.T)


from jxl_rs_amd.lib import DeviceArray  # noqa: E402,F401  (device buffers for tests that hand DEVICE pointers to the C ABI)


# ---- Modular chain (jxl_rs_amd.modular.ModularChain): what the oracle makes of the same planes ----
def modular_chain_oracle(chain, oracle):
    """the chain's levels one by one on the CPU oracle, then the RCT"""
    cur = [b.copy() for b in chain.base]
    for (hz, ow, oh), res in zip(chain.steps, chain.residuals):
        cur = [oracle.unsqueeze_h(cur[c], res[c], ow) if hz else oracle.unsqueeze_v(cur[c], res[c], oh) for c in range(3)]
    return oracle.rct(cur, *chain.rct) if chain.rct is not None else cur


def modular_pipeline_oracle(chain, oracle):
    """chain + RCT and the palette expansion of BASELINE configs[3]"""
    idx, pal = chain.palette
    return modular_chain_oracle(chain, oracle), list(oracle.palette(idx, pal, pal.shape[1], 3, 8))
