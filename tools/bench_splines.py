"""Cost of the splines draw (k_splines.hip) on a 7680 x 4320 frame (a measurement tool, not a test).

Two workloads, one JSON line each:
  thin   64 splines of about 6000 segments each, one pixel apart along smooth curves across the frame, sigma 1..3
         (maximum_distance from add_segment's rule at low precision)
  wide   the 1940 segments the reference's init_draw_cache test builds (tests/golden/splines_kat.json) through
         jxlh_splines_build_segments, their centres spread over the frame: maximum_distance up to about 3000
Columns:
  draw_ms        k_splines alone, from the library's event timers on three device planes through jxlh_stage_splines:
                 median over `reps` repetitions of the mean of `steps` draws (all batches of a draw), smallest and largest
  set_ms         jxlh_frame_set_splines on the host clock: bounds, batch plan, the bin list of a one-batch set, uploads
  call_ms        one jxlh_stage_splines call on the host clock (staging copies and, for a set of several batches, the
                 binning and upload of every batch included)
  batches, bin_entries
  pairs, Gpairs_per_s   pixel-segment pairs of the per-pixel rule, and pairs / draw_ms
  floor_ms, bound       the least time the hardware could take: max of
                   compute  pairs x 83 issue cycles / (256 CUs x 64 lanes x 2.4 GHz) -- the loop body's 64 VALU
                            instructions in the gfx950 code, its 10 packed ones counted twice and its 3 quarter-rate ones
                            (sqrt, two rcp) four times
                   memory   24 B per touched pixel (3 loads, 3 stores) / 6.29 TB/s (the measured copy rate)
                 and which of the two it is

  python tools/bench_splines.py [--width 7680] [--height 4320] [--steps 10] [--reps 5] [--only thin|wide]
bin_entries are counted for the library's own bin geometry (jxlh_splines_bin_layout)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ISSUE_CYCLES_PER_PAIR = 83
LANES_PER_S = 256 * 64 * 2.4e9
COPY_BPS = 6.29e12


def thin_segments(np, w, h, n_splines=64, n_seg=6000):
    rng = np.random.default_rng(7)
    out = []
    for s in range(n_splines):
        t = np.arange(n_seg, dtype=np.float64)
        ang = rng.uniform(0, 2 * np.pi) + 0.0004 * t * rng.uniform(-1, 1) + 0.3 * np.sin(t / rng.uniform(300, 900))
        x = rng.uniform(0.1, 0.9) * w + np.cumsum(np.cos(ang))
        y = rng.uniform(0.1, 0.9) * h + np.cumsum(np.sin(ang))
        x, y = w - np.abs(x % (2 * w) - w), h - np.abs(y % (2 * h) - h)  # a curve that reaches an edge turns back
        sigma = (2.0 + np.sin(t / 500.0 + s)).astype(np.float32)  # 1..3
        color = np.stack([0.3 + 0.2 * np.sin(t / 700.0 + c + s) for c in range(3)], 1).astype(np.float32)
        max_color = np.maximum(0.01, np.abs(color).max(1)).astype(np.float32)
        md = np.sqrt(-2.0 * sigma * sigma * (np.log(np.float32(0.1)) * np.float32(3.0) - np.log(max_color)))
        seg = np.zeros((n_seg, 8), np.float32)
        seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3], seg[:, 4] = x, y, md, 1.0 / sigma, 0.25 * sigma
        seg[:, 5:8] = color
        out.append(seg)
    return np.concatenate(out)


def wide_segments(np, lib, w, h):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "splines_kat.json")))["init_draw_cache"]
    splines = [(q["control_points"], q["color_dct"], q["sigma_dct"], tuple(s)) for q, s in zip(k["splines"], k["starting_points"])]
    st, seg = lib.try_build_spline_segments(splines, k["quantization_adjustment"], k["y_to_x_lf"], k["y_to_b_lf"],
                                            k["image_xsize"], k["image_ysize"], k["high_precision"])
    assert st == lib.OK and seg.shape[0] == k["n_segments"]
    cx, cy = seg[:, 0], seg[:, 1]
    seg[:, 0] = (cx - cx.min()) / (cx.max() - cx.min()) * (w - 1)
    seg[:, 1] = (cy - cy.min()) / (cy.max() - cy.min()) * (h - 1)
    return seg


def boxes(np, seg, w, h):
    """the per-pixel rule's ranges, clipped to the plane (the workloads hold no NaN and nothing beyond 2^31)"""
    def rnd(v):
        return (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int64)
    x0 = np.clip(rnd(seg[:, 0] - seg[:, 2]), 0, None)
    x1 = np.minimum(np.clip(rnd(seg[:, 0] + seg[:, 2]), 0, None) + 1, w)
    y0 = np.clip(rnd(seg[:, 1] - seg[:, 2]), 0, None)
    y1 = np.minimum(rnd(seg[:, 1] + seg[:, 2]) + 1, h)
    return x0, np.maximum(x1, x0), y0, np.maximum(y1, y0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=7680)
    ap.add_argument("--height", type=int, default=4320)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only")
    ap.add_argument("--bin")
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    w, h = a.width, a.height
    a.bin = a.bin or "%dx%d" % lib.splines_bin_layout()  # (a library built before the hook existed: say it)
    BIN_W, BIN_H = (int(v) for v in a.bin.split("x"))
    ctx = jxl_rs_amd.Context(0, 1)
    ctx.frame_begin(ctx.default_params(w, h))
    rng = np.random.default_rng(1)
    planes = [lib.DeviceArray(rng.random((h, w), dtype=np.float32)) for _ in range(3)]
    pp = (C.c_void_p * 3)(*[p.ptr for p in planes])

    def draw():
        st = ctx.L.jxlh_stage_splines(ctx._ctx, pp, w, h, w)
        assert st == 0, st

    for name in ("thin", "wide"):
        if a.only and a.only != name:
            continue
        seg = thin_segments(np, w, h) if name == "thin" else wide_segments(np, lib, w, h)
        x0, x1, y0, y1 = boxes(np, seg, w, h)
        pairs = int(((x1 - x0) * (y1 - y0)).sum())
        live = (x1 > x0) & (y1 > y0)
        entries = int((((x1 - 1) // BIN_W - x0 // BIN_W + 1) * ((y1 - 1) // BIN_H - y0 // BIN_H + 1))[live].sum())
        # touched pixels: the union of the boxes, by rows
        cover = np.zeros((h, w), np.bool_)
        for i in np.flatnonzero(live):
            cover[y0[i]:y1[i], x0[i]:x1[i]] = True
        touched = int(cover.sum())
        set_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            ctx.set_splines(seg)
            set_ms.append((time.perf_counter() - t0) * 1e3)
        draw()  # warm
        ctx.sync()
        k_ms, call_ms = [], []
        launches = 0
        for _ in range(a.reps):
            ctx.kernel_timing_reset()
            ctx.kernel_timing(True)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                draw()
            ctx.sync()
            call_ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            kt = ctx.kernel_times()
            ctx.kernel_timing(False)
            k_ms.append(kt["k_splines"][0] / a.steps)
            launches = kt["k_splines"][1] // a.steps
        km = statistics.median(k_ms)
        compute_ms = pairs * ISSUE_CYCLES_PER_PAIR / LANES_PER_S * 1e3
        memory_ms = touched * 24 / COPY_BPS * 1e3
        print(json.dumps({
            "case": name, "frame": f"{w}x{h}", "bin": a.bin, "segments": int(seg.shape[0]), "batches": launches, "bin_entries": entries,
            "pairs": pairs, "touched_pixels": touched, "draw_ms": km, "draw_ms_min_max": [min(k_ms), max(k_ms)],
            "Gpairs_per_s": pairs / km * 1e-6, "set_ms": statistics.median(set_ms), "call_ms": statistics.median(call_ms),
            "floor_compute_ms": compute_ms, "floor_memory_ms": memory_ms, "floor_ms": max(compute_ms, memory_ms),
            "bound": "compute" if compute_ms >= memory_ms else "memory", "of_floor": max(compute_ms, memory_ms) / km,
        }), flush=True)
    for p in planes:
        p.free()
    ctx.close()


if __name__ == "__main__":
    main()
