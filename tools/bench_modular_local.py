"""Cost of the group-local Modular transforms on the device (k_modular_local.hip, abi_modular_local.hip) on an 8192 x 8192
8-bit RGB frame in 1024 rects of 256 x 256 (a measurement tool, not a test).

Cases of the new call (jxlh_frame_set_modular_groups*, device-resident arena, the descriptors lowered and uploaded inside
the timed call): rct = every rect an RCT, types cycling; palette = every rect a 256-colour three-channel palette; mixed =
half and half.  One JSON line per case:
  kernel_ms       k_modular_local alone, from the library's event timers: median over `reps` of the mean of `steps`
  bytes / TBps    the kernel's own traffic (12 B/px read for an RCT rect, 4 B/px for a palette rect, 12 B/px written)
  call_ms         the _async call by the host clock, `steps` calls and one synchronise: lowering, upload, launch
  blocking_ms     the blocking call, one at a time
  host_arena_ms   (rct only) the blocking call with the arena in host memory: the one-copy upload included
What the interface offered before, on the same data, same session:
  whole_plane     one whole-plane jxlh_rct (k4_rct, in place) + one whole-frame jxlh_frame_set_modular_channels from device
                  memory: only possible when all groups share an op
  per_group       1024 x (jxlh_rct on the group's contiguous buffer + one rect call)
Two contexts alternate between repetitions.

  python tools/bench_modular_local.py [--size 8192] [--steps 10] [--reps 5] [--kernel-only] [--general | --squeeze | --rgba | --host-side]
--kernel-only: a few launches of the rct case and nothing else, for a profiler run of its own.

--general: the group-local palettes with delta entries (jxlh_frame_set_modular_groups_general, k_modular_local_palette.hip)
on the same frame and rects, device-resident arena, kernels alone from the library's event timers (median, min and max
over `reps` of the mean of `steps`; --steps 20 --reps 5 for the recorded table):
  delta_p5   every rect a three-channel delta palette (11 colours, 5 delta entries, the tests' index recipe), predictor 5
  delta_p6   the same under the weighted predictor (default header)
  mix16      1 rect in 16 a predictor-5 delta palette, the others RCTs -- the batch the old refusal made expensive
against
  whole_p5 / whole_p6   jxlh_palette_delta / jxlh_palette_delta_wp on ONE 8192 x 8192 plane set with the same palette and
                        index statistics (k5_palette + k5_palette_delta / k5_palette_wp): the only device path for
                        this arithmetic before
  mix16_lookup          k_modular_local on the mix16 batch with the delta rects replaced by look-up palettes: the
                        difference to mix16 is what the general groups cost
With --kernel-only: a few launches of delta_p5 and nothing else.

--squeeze: group-local squeezes (jxlh_frame_set_modular_groups_squeeze_async, k_modular_local_squeeze.hip) on the same
frame: 3 channels, every 256 x 256 rect a default squeeze (the 4:2:0-preview steps included) of its own coded channels,
device-resident arena; median, min and max over `reps` of the mean of `steps`:
  squeeze     kernel times per label with the launches per call (the LDS launch, the streamed level launches), the _async
              call on the host clock, and the bytes moved: arena read, planes written, scratch written and read back
  per_group   what the interface offered before for such a frame: per group one jxlh_unsqueeze_chain (three planes of one
              geometry: the default squeeze without the preview steps) plus one rect intake
              (jxlh_frame_set_modular_channels from device memory); kernels summed over all labels, and the host clock
With --kernel-only: a few calls of the squeeze case and nothing else.

--rgba: groups with an extra channel (jxlh_frame_set_modular_groups_extra_async, jxl_hip_local_extra.h) on an 8-bit RGBA
frame of the same size and rects, device-resident arena, extra channel 0 begun at the frame's size.  Cases: rct = every
rect an RCT on channels 0..2, types cycling, the alpha as coded; palette = every rect a 256-colour palette over all four
channels.  Per case and route one JSON line, median, min and max over `reps` of the mean of `steps`:
  direct       the one _async call: kernels_ms from the library's event timers (all labels, listed), call_ms by the host
               clock (`steps` calls and one synchronise); absent when the library predates the call (JXLH_LIBRARY: A/B runs)
  three_calls  what the interface offered before: jxlh_modular_local_transforms_squeeze into four caller planes (it
               waits), jxlh_frame_set_modular_channels of three of them, jxlh_frame_set_extra_channel_rects_async of the
               fourth; the same two clocks
  bytes / TBps the route's own traffic over kernels_ms: the coded channels read and four channels written, plus -- three
               calls -- three channels copied and one scattered, read and written again
With --kernel-only: a few direct calls of the rct case and nothing else.

--host-side [--only plain|mix16|squeeze]: what a 1024-rect batch costs on the host, one context, event timers off: rct of
the first table (plain), mix16 of --general, squeeze of --squeeze.  Per case one JSON line, median, min and max over
`reps` of the mean of `steps` calls (--steps 20 --reps 7 for the recorded table):
  enqueue_ms              the _async call until it returns: lowering, planning, the block, one copy, the launches enqueued
  call_plus_sync_ms       the call and one synchronise
  kernels_ms              the k_modular_local* event timers, in a pass of their own
  wall_minus_kernels_ms   median call_plus_sync_ms - median kernels_ms
  minor_faults_per_call   page faults of the process inside the timed calls (getrusage): memory the allocator hands
                          back and takes again on every call shows here"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--squeeze", action="store_true")
    ap.add_argument("--rgba", action="store_true")
    ap.add_argument("--host-side", action="store_true")
    ap.add_argument("--only", choices=["plain", "mix16", "squeeze"])
    a = ap.parse_args()
    if a.host_side:
        return host_side(a)
    if a.general:
        return general(a)
    if a.squeeze:
        return squeeze(a)
    if a.rgba:
        return rgba(a)
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n, g = a.size, 256
    rng = np.random.default_rng(1)
    chan = [rng.integers(0, 64, size=(g, g)).astype(np.int32) for _ in range(3)]
    index = rng.integers(0, 256, size=(g, g)).astype(np.int32)
    table = rng.integers(0, 256, size=(3, 256)).astype(np.int32)

    def specs(kind):
        out = []
        for k, (gy, gx) in enumerate((y, x) for y in range(0, n, g) for x in range(0, n, g)):
            pal = kind == "palette" or (kind == "mixed" and k % 2)
            steps = [lib.local_palette(0, 3, table)] if pal else [lib.local_rct(0, k % 42)]
            out.append({"x0": gx, "y0": gy, "n_channels": 3, "steps": steps, "coded": [index] if pal else chan})
        return out

    ctxs = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    p = ctxs[0].default_params(n, n)
    p.gab, p.epf_iters = 0, 0
    for c in ctxs:
        c.modular_frame_begin(p)

    def timed(c, call, steps, kernel):
        c.kernel_timing_reset()
        c.kernel_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            call(c)
        c.sync()
        host = (time.perf_counter() - t0) * 1e3 / steps
        kt = c.kernel_times()
        c.kernel_timing(False)
        return host, sum(ms for k, (ms, _) in kt.items() if k == kernel) / steps

    def measure(call, steps, kernel):
        """median over reps of (host ms per call, kernel ms per call), the two contexts alternating"""
        for c in ctxs:
            call(c)
            c.sync()
        h, k = zip(*[timed(ctxs[r % 2], call, steps, kernel) for r in range(a.reps)])
        return statistics.median(h), [min(h), max(h)], statistics.median(k), [min(k), max(k)]

    for kind in ("rct", "palette", "mixed"):
        sp = specs(kind)
        arena, groups = lib.pack_local_groups(sp)
        dev = lib.DeviceArray(arena)
        launch = lambda c, wait=False: c.set_modular_groups(dev, groups, 8, n=len(sp), arena_samples=arena.size, wait=wait)
        if a.kernel_only:
            for _ in range(5):
                launch(ctxs[0])
            ctxs[0].sync()
            dev.free()
            break
        n_pal = sum(1 for s in sp if len(s["coded"]) == 1)
        nbytes = g * g * 4 * (3 * len(sp) + n_pal * 1 + (len(sp) - n_pal) * 3)
        call_ms, call_mm, k_ms, k_mm = measure(launch, a.steps, "k_modular_local")
        block_ms = measure(lambda c: launch(c, True), a.steps, "k_modular_local")[0]
        row = {"case": kind, "frame": f"{n}x{n}", "rects": len(sp), "bytes": nbytes, "kernel_ms": k_ms, "kernel_ms_min_max": k_mm,
               "TBps": nbytes / k_ms * 1e-9, "call_ms": call_ms, "call_ms_min_max": call_mm, "blocking_ms": block_ms}
        if kind == "rct":
            row["host_arena_ms"] = measure(lambda c: c.set_modular_groups(arena, groups, 8, n=len(sp)), 2, "k_modular_local")[0]
        print(json.dumps(row), flush=True)
        dev.free()
    if not a.kernel_only:
        # the old interface on the same amount of data: three device planes, transformed in place
        planes = [lib.DeviceArray(rng.integers(0, 64, size=(n, n)).astype(np.int32)) for _ in range(3)]

        def whole(c):
            c._chk(c.L.jxlh_rct(c._ctx, planes[0].ptr, planes[1].ptr, planes[2].ptr, n * n, 6, 0), "rct")
            c.set_modular_channels(*[d.ptr for d in planes], 8, w=n, h=n, stride=n)

        h_ms, h_mm, k_ms, k_mm = measure(whole, a.steps, "k4_rct")
        print(json.dumps({"case": "whole_plane", "call_ms": h_ms, "call_ms_min_max": h_mm, "k4_rct_ms": k_ms, "k4_rct_ms_min_max": k_mm,
                          "k4_rct_TBps": 24 * n * n / k_ms * 1e-9}), flush=True)
        bufs = [lib.DeviceArray(c) for c in chan]

        def per_group(c):
            for k, (gy, gx) in enumerate((y, x) for y in range(0, n, g) for x in range(0, n, g)):
                c._chk(c.L.jxlh_rct(c._ctx, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, g * g, k % 7, k // 7 % 6), "rct")
                c.set_modular_channels(*[d.ptr for d in bufs], 8, x0=gx, y0=gy, w=g, h=g, stride=g)

        h_ms, h_mm, _, _ = measure(per_group, 2, "k4_rct")
        print(json.dumps({"case": "per_group", "call_ms": h_ms, "call_ms_min_max": h_mm}), flush=True)
        for d in planes + bufs:
            d.free()
    for c in ctxs:
        c.close()


def rgba(a):
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n, g = a.size, 256
    rng = np.random.default_rng(4)
    chan = [rng.integers(0, 64, size=(g, g)).astype(np.int32) for _ in range(4)]
    index = rng.integers(0, 256, size=(g, g)).astype(np.int32)
    table = rng.integers(0, 256, size=(4, 256)).astype(np.int32)
    cells = [(x, y) for y in range(0, n, g) for x in range(0, n, g)]
    have_direct = hasattr(lib.load(), "jxlh_frame_set_modular_groups_extra_async")
    ctxs = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    p = ctxs[0].default_params(n, n)
    p.gab, p.epf_iters = 0, 0
    for c in ctxs:
        c.modular_frame_begin(p)
        c.begin_extra_channel(0, n, n, 8, 1)
    outs = [lib.DeviceArray(nbytes=n * n * 4) for _ in range(4)]
    descs = np.zeros(len(cells), dtype=lib.EC_RECT_DTYPE)
    for d, (x, y) in zip(descs, cells):
        d["ec"], d["x0"], d["y0"], d["w"], d["h"], d["offset"], d["stride"] = 0, x, y, g, g, y * n + x, n

    def timed(c, call, steps):
        c.kernel_timing_reset()
        c.kernel_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            call(c)
        c.sync()
        host = (time.perf_counter() - t0) * 1e3 / steps
        kt = {k: (ms / steps, cnt // steps) for k, (ms, cnt) in c.kernel_times().items() if cnt}
        c.kernel_timing(False)
        return host, sum(ms for ms, _ in kt.values()), kt

    def measure(call):
        for c in ctxs:
            call(c)
            c.sync()
        rows = [timed(ctxs[r % 2], call, a.steps) for r in range(a.reps)]
        h, k = [r[0] for r in rows], [r[1] for r in rows]
        labels = {name: [round(statistics.median(r[2][name][0] for r in rows), 4), rows[0][2][name][1]] for name in rows[0][2]}
        return statistics.median(h), [min(h), max(h)], statistics.median(k), [min(k), max(k)], labels

    for kind in ("rct", "palette"):
        pal = kind == "palette"
        sp = [{"x0": x, "y0": y, "w": g, "h": g, "n_channels": 4, "squeeze": None,
               "steps": [lib.local_palette(0, 4, table)] if pal else [lib.local_rct(0, k % 42)],
               "coded": [index] if pal else chan} for k, (x, y) in enumerate(cells)]
        arena, batch = lib.pack_local_squeeze_groups(sp)
        dev = lib.DeviceArray(arena)
        dest = lib.local_dest(3, [0]) if have_direct else None
        direct = lambda c: c.set_modular_groups_extra(dev, batch, 8, dest, n=len(sp), arena_samples=arena.size, wait=False)

        def three(c):
            c.modular_local_transforms_squeeze(dev, batch, 8, outs, n, n, n, n=len(sp), arena_samples=arena.size)
            c.set_modular_channels(outs[0].ptr, outs[1].ptr, outs[2].ptr, 8, w=n, h=n, stride=n)
            c.set_extra_channel_rects(descs, block=outs[3], n_samples=n * n, wait=False)

        if a.kernel_only:
            for _ in range(5):
                (direct if have_direct else three)(ctxs[0])
            ctxs[0].sync()
            dev.free()
            break
        samples = (1 if pal else 4) + 4  # per pixel: coded channels read, four written
        for route, call, per_px in (("direct", direct, samples), ("three_calls", three, samples + 8)):
            if route == "direct" and not have_direct:
                continue
            call_ms, call_mm, k_ms, k_mm, labels = measure(call)
            nbytes = per_px * 4 * n * n
            print(json.dumps({"case": kind, "route": route, "library": os.environ.get("JXLH_LIBRARY", "tree"), "frame": f"{n}x{n}",
                              "rects": len(sp), "bytes": nbytes, "kernels_ms": k_ms, "kernels_ms_min_max": k_mm,
                              "TBps": nbytes / k_ms * 1e-9, "call_ms": call_ms, "call_ms_min_max": call_mm, "kernels": labels}),
                  flush=True)
        dev.free()
    for o in outs:
        o.free()
    for c in ctxs:
        c.close()


def general(a):
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n, g = a.size, 256
    rng = np.random.default_rng(2)
    num_colors, num_deltas = 11, 5
    table = rng.integers(0, 256, size=(3, num_deltas + num_colors)).astype(np.int32)
    table[:, :num_deltas] = rng.integers(-12, 13, size=(3, num_deltas))

    def recipe_index(shape):
        idx = rng.integers(-8, num_colors + num_deltas + 200, size=shape).astype(np.int32)
        redraw = rng.random(shape) < 0.5
        idx[redraw] = rng.integers(0, num_deltas, size=int(redraw.sum()))
        return idx

    index = recipe_index((g, g))
    chan = [rng.integers(0, 64, size=(g, g)).astype(np.int32) for _ in range(3)]
    WP_DEFAULT = (16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12)

    def specs(kind):
        out = []
        for k, (gy, gx) in enumerate((y, x) for y in range(0, n, g) for x in range(0, n, g)):
            if kind == "delta_p5" or (kind.startswith("mix16") and k % 16 == 0):
                steps = [lib.local_palette(0, 3, table, *((0, 0) if kind == "mix16_lookup" else (num_deltas, 5)))]
            elif kind == "delta_p6":
                steps = [lib.local_palette(0, 3, table, num_deltas, 6)]
            else:
                steps = [lib.local_rct(0, k % 42)]
            out.append({"x0": gx, "y0": gy, "n_channels": 3, "steps": steps, "coded": [index] if steps[0]["kind"] == lib.LOCAL_PALETTE else chan})
        return out

    ctxs = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    p = ctxs[0].default_params(n, n)
    p.gab, p.epf_iters = 0, 0
    for c in ctxs:
        c.modular_frame_begin(p)

    def timed(c, call, steps):
        c.kernel_timing_reset()
        c.kernel_timing(True)
        for _ in range(steps):
            call(c)
        c.sync()
        kt = c.kernel_times()
        c.kernel_timing(False)
        return {k: ms / steps for k, (ms, _) in kt.items()}, {k: cnt // steps for k, (_, cnt) in kt.items()}

    def measure(call):
        for c in ctxs:
            call(c)
            c.sync()
        runs = [timed(ctxs[r % 2], call, a.steps) for r in range(a.reps)]
        labels = sorted(runs[0][0])
        row = {"launches_per_call": runs[0][1]}
        for k in labels + ["total"]:
            v = [sum(r[0].values()) if k == "total" else r[0][k] for r in runs]
            row[k + "_ms"] = [statistics.median(v), min(v), max(v)]
        return row

    for kind in ("delta_p5", "delta_p6", "mix16", "mix16_lookup"):
        sp = specs(kind)
        arena, groups = lib.pack_local_groups(sp)
        dev = lib.DeviceArray(arena)
        wp = lib.wp_headers([WP_DEFAULT] * len(sp))
        if kind == "mix16_lookup":
            launch = lambda c: c.set_modular_groups(dev, groups, 8, n=len(sp), arena_samples=arena.size, wait=False)
        else:
            launch = lambda c: c.set_modular_groups_general(dev, groups, 8, wp=wp, n=len(sp), arena_samples=arena.size, wait=False)
        if a.kernel_only:
            for _ in range(3):
                launch(ctxs[0])
            ctxs[0].sync()
            dev.free()
            break
        row = {"case": kind, "frame": f"{n}x{n}", "rects": len(sp), "median_min_max": True}
        row.update(measure(launch))
        print(json.dumps(row), flush=True)
        dev.free()
    if not a.kernel_only:
        # the whole-plane kernels on one plane set of the frame's size
        idx = lib.DeviceArray(recipe_index((n, n)))
        pal = lib.DeviceArray(table)
        out = lib.DeviceArray(nbytes=3 * n * n * 4)
        hdr = lib.wp_headers([WP_DEFAULT])

        def whole_p5(c):
            c._chk(c.L.jxlh_palette_delta(c._ctx, idx.ptr, n, n, pal.ptr, num_colors, num_deltas, num_colors + num_deltas, 3, 8, 5,
                                          out.ptr), "palette_delta")

        def whole_p6(c):
            c._chk(c.L.jxlh_palette_delta_wp(c._ctx, idx.ptr, n, n, pal.ptr, num_colors, num_deltas, num_colors + num_deltas, 3, 8,
                                             hdr, out.ptr), "palette_delta_wp")

        for name, call in (("whole_p5", whole_p5), ("whole_p6", whole_p6)):
            row = {"case": name, "plane_set": f"3 x {n}x{n}", "median_min_max": True}
            row.update(measure(call))
            print(json.dumps(row), flush=True)
        for d in (idx, pal, out):
            d.free()
    for c in ctxs:
        c.close()


def _squeeze_batch(lib, rng, n, g):
    """every g x g rect of an n x n frame a default squeeze of three channels -> (arena, batch, rects, coded sizes)"""
    import ctypes as C
    import numpy as np
    # one group's coded channels under the default squeeze, as the lowering derives them; every group gets a copy of its own
    one = {"x0": 0, "y0": 0, "w": g, "h": g, "n_channels": 3, "steps": [], "squeeze": lib.local_squeeze(), "coded": []}
    sizes = [(g, g)] * 3
    for horizontal, in_place, begin_c, num_c in lib.default_squeeze(sizes):
        at0 = begin_c + num_c if in_place else len(sizes)
        for ic in range(num_c):
            w, h = sizes[begin_c + ic]
            sizes[begin_c + ic] = ((w + 1) // 2, h) if horizontal else (w, (h + 1) // 2)
            sizes.insert(at0 + ic, (w // 2, h) if horizontal else (w, h // 2))
    one["coded"] = [rng.integers(-40, 40, size=(h, w)).astype(np.int32) for w, h in sizes]
    arena_one, (g1, c1, _) = lib.pack_local_squeeze_groups([one])
    m, per = len(sizes), -(-arena_one.size // 64) * 64
    rects = [(x, y) for y in range(0, n, g) for x in range(0, n, g)]
    arena = np.zeros(per * len(rects), dtype=np.int32)
    groups = (lib.LocalSqueezeGroup * len(rects))()
    coded = (lib.LocalCodedChannel * (m * len(rects)))()
    params = (lib.SqueezeParams * 1)()
    for k, (x, y) in enumerate(rects):
        arena[k * per:k * per + arena_one.size] = arena_one
        C.memmove(C.byref(groups[k]), C.byref(g1[0]), C.sizeof(lib.LocalSqueezeGroup))
        groups[k].x0, groups[k].y0, groups[k].coded_first = x, y, k * m
        for j in range(m):
            C.memmove(C.byref(coded[k * m + j]), C.byref(c1[j]), C.sizeof(lib.LocalCodedChannel))
            coded[k * m + j].offset += k * per
    batch = (groups, coded, params)
    return arena, batch, rects, sizes


def squeeze(a):
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    from jxl_rs_amd.modular import ModularChain
    n, g = a.size, 256
    rng = np.random.default_rng(3)
    arena, batch, rects, sizes = _squeeze_batch(lib, rng, n, g)
    st, progs, bad = lib.modular_local_lower_squeeze(batch, 8, arena.size)
    assert st == lib.OK, (st, bad)
    scratch = 0  # samples written to scratch and read back: every level's output from the LDS launch's last on, but the chain's last
    for ch in list(progs[0].chains)[:3]:
        lv = list(ch.levels)[:ch.n_levels]
        n_lds = sum(1 for q in lv if q.out_w <= 128 and q.out_h <= 128)
        scratch += sum(q.out_w * q.out_h for q in lv[max(n_lds - 1, 0):-1])
    ctxs = [jxl_rs_amd.Context(0, 1) for _ in range(2)]
    p = ctxs[0].default_params(n, n)
    p.gab, p.epf_iters = 0, 0
    for c in ctxs:
        c.modular_frame_begin(p)
    dev = lib.DeviceArray(arena)

    def timed(c, call, steps):
        c.kernel_timing_reset()
        c.kernel_timing(True)
        t0 = time.perf_counter()
        for _ in range(steps):
            call(c)
        c.sync()
        host = (time.perf_counter() - t0) * 1e3 / steps
        kt = c.kernel_times()
        c.kernel_timing(False)
        return host, {k: ms / steps for k, (ms, _) in kt.items()}, {k: cnt // steps for k, (_, cnt) in kt.items()}

    def measure(call, steps):
        for c in ctxs:
            call(c)
            c.sync()
        runs = [timed(ctxs[r % 2], call, steps) for r in range(a.reps)]
        row = {"launches_per_call": runs[0][2], "call_ms": [statistics.median([r[0] for r in runs]), min(r[0] for r in runs), max(r[0] for r in runs)]}
        for k in sorted(runs[0][1]) + ["total"]:
            v = [sum(r[1].values()) if k == "total" else r[1][k] for r in runs]
            row[k + "_ms"] = [statistics.median(v), min(v), max(v)]
        return row

    launch = lambda c: c.set_modular_groups_squeeze(dev, batch, 8, n=len(rects), arena_samples=arena.size, wait=False)
    if a.kernel_only:
        for _ in range(3):
            launch(ctxs[0])
        ctxs[0].sync()
    else:
        row = {"case": "squeeze", "frame": f"{n}x{n}", "rects": len(rects), "median_min_max": True,
               "bytes": {"arena_read": 4 * sum(w * h for w, h in sizes) * len(rects), "planes_written": 12 * g * g * len(rects),
                         "scratch_written_and_read": 8 * scratch * len(rects)}}
        row.update(measure(launch, a.steps))
        print(json.dumps(row), flush=True)
        chains = [ModularChain(c, g, g, seed=5, rct=None) for c in ctxs]

        def per_group(c):
            ch = chains[ctxs.index(c)]
            for x, y in rects:
                ch.run_chain()
                c.set_modular_channels(*[d.ptr for d in ch.d_out], 8, x0=x, y0=y, w=g, h=g, stride=g)

        row = {"case": "per_group", "frame": f"{n}x{n}", "rects": len(rects), "median_min_max": True}
        row.update(measure(per_group, max(1, a.steps // 5)))
        print(json.dumps(row), flush=True)
        for ch in chains:
            ch.free()
    dev.free()
    for c in ctxs:
        c.close()


def host_side(a):
    import resource
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n, g = a.size, 256
    rng = np.random.default_rng(1)
    rects = [(x, y) for y in range(0, n, g) for x in range(0, n, g)]
    chan = [rng.integers(0, 64, size=(g, g)).astype(np.int32) for _ in range(3)]
    table = rng.integers(0, 256, size=(3, 16)).astype(np.int32)
    table[:, :5] = rng.integers(-12, 13, size=(3, 5))
    index = rng.integers(0, 16, size=(g, g)).astype(np.int32)
    ctx = jxl_rs_amd.Context(0, 1)
    p = ctx.default_params(n, n)
    p.gab, p.epf_iters = 0, 0
    ctx.modular_frame_begin(p)

    def groups_case(kind):
        sp = []
        for k, (x, y) in enumerate(rects):
            pal = kind == "mix16" and k % 16 == 0
            steps = [lib.local_palette(0, 3, table, 5, 5)] if pal else [lib.local_rct(0, k % 42)]
            sp.append({"x0": x, "y0": y, "n_channels": 3, "steps": steps, "coded": [index] if pal else chan})
        arena, groups = lib.pack_local_groups(sp)
        dev = lib.DeviceArray(arena)
        if kind == "plain":
            return dev, lambda: ctx.set_modular_groups(dev, groups, 8, n=len(sp), arena_samples=arena.size, wait=False)
        wp = lib.wp_headers([(16, 10, 7, 7, 7, 0, 0, 13, 12, 12, 12)] * len(sp))
        return dev, lambda: ctx.set_modular_groups_general(dev, groups, 8, wp=wp, n=len(sp), arena_samples=arena.size, wait=False)

    def squeeze_case(kind):
        arena, batch, _, _ = _squeeze_batch(lib, rng, n, g)
        dev = lib.DeviceArray(arena)
        return dev, lambda: ctx.set_modular_groups_squeeze(dev, batch, 8, n=len(rects), arena_samples=arena.size, wait=False)

    def mmm(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    for kind, make in (("plain", groups_case), ("mix16", groups_case), ("squeeze", squeeze_case)):
        if a.only and a.only != kind:
            continue
        dev, call = make(kind)
        for _ in range(5):
            call()
            ctx.sync()
        enq, wall, kern, faults = [], [], [], []
        for _ in range(a.reps):
            e = w = 0.0
            f0 = resource.getrusage(resource.RUSAGE_SELF).ru_minflt
            for _ in range(a.steps):
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                ctx.sync()
                e += t1 - t0
                w += time.perf_counter() - t0
            faults.append((resource.getrusage(resource.RUSAGE_SELF).ru_minflt - f0) / a.steps)
            enq.append(e * 1e3 / a.steps)
            wall.append(w * 1e3 / a.steps)
        for _ in range(a.reps):
            ctx.kernel_timing_reset()
            ctx.kernel_timing(True)
            for _ in range(a.steps):
                call()
            ctx.sync()
            kt = ctx.kernel_times()
            ctx.kernel_timing(False)
            kern.append(sum(ms for k, (ms, _) in kt.items() if k.startswith("k_modular_local")) / a.steps)
        print(json.dumps({"case": kind, "frame": f"{n}x{n}", "rects": len(rects), "median_min_max": True, "enqueue_ms": mmm(enq),
                          "call_plus_sync_ms": mmm(wall), "kernels_ms": mmm(kern),
                          "wall_minus_kernels_ms": round(statistics.median(wall) - statistics.median(kern), 4),
                          "minor_faults_per_call": mmm(faults)}), flush=True)
        dev.free()
    ctx.close()


if __name__ == "__main__":
    main()
