#!/usr/bin/env python3
"""Squeeze previews per grid cell, timed: the default squeeze chain of an n x n image on three channels with the RCT
behind it, planes device resident, cells of 256 samples at the finest level (halved with each level's shift), and the
two finest levels with the first half of their cells present in download (raster) order.

  (a) jxlh_unsqueeze_chain_preview_tiles: the mixed case, one call;
  (b) jxlh_unsqueeze_chain_preview with those two levels wholly missing;
  (c) jxlh_unsqueeze_chain with everything present.
(b) and (c) are the two existing calls that bracket (a): without (a) there is no route for the mixed case itself.  All
three from HIP events on the context's stream, alternated in one process, median of 5 x 20 calls with min and max, the
host-clock time of issuing them, and the library's kernel timers for one call of each.

  python tools/bench_squeeze_tiles.py [n]          # prints one JSON line"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    cell = 256
    ctx = jxl_rs_amd.Context(0, 1)
    rng = np.random.default_rng(11)
    steps, (bw, bh) = synth.default_squeeze_steps(n, n)
    nl = len(steps)
    base = [lib.DeviceArray(rng.integers(0, 256, size=(bh, bw), dtype=np.int32)) for _ in range(3)]
    out = [lib.DeviceArray(nbytes=n * n * 4) for _ in range(3)]
    res = []
    for hz, ow, oh in steps:
        rw, rh = (ow // 2, oh) if hz else (ow, oh // 2)
        res.append([lib.DeviceArray(rng.integers(-8, 9, size=(rh, rw), dtype=np.int32)) for _ in range(3)])
    full = [(hz, ow, oh, [d.ptr for d in r], max(ow // 2 if hz else ow, 1)) for (hz, ow, oh), r in zip(steps, res)]
    missing2 = [lv if i < nl - 2 else lv[:3] + ([None] * 3, lv[4]) for i, lv in enumerate(full)]
    # the grids of the two finest levels, half of each in raster order
    tiles, tw, th, cells = [(0, 0, None)] * nl, cell, cell, []
    for k in range(2):
        level = nl - 1 - k
        nx, ny = lib.squeeze_tile_grid(full[level], (tw, th))
        present = np.zeros(nx * ny, np.uint8)
        present[:nx * ny // 2] = 1
        tiles[level] = (tw, th, present.reshape(ny, nx))
        cells.append(nx * ny)
        tw, th = (tw // 2, th) if steps[level][0] else (tw, th // 2)
    bp, op = [d.ptr for d in base], [d.ptr for d in out]
    calls = {
        "tiles_half_present": lambda: ctx.unsqueeze_chain_preview_tiles(full, tiles, bp, bw, bw, bh, op, n, rct=(6, 0)),
        "preview_two_missing": lambda: ctx.unsqueeze_chain_preview(missing2, bp, bw, bw, bh, op, n, rct=(6, 0)),
        "chain_all_present": lambda: ctx.unsqueeze_chain(full, bp, bw, bw, bh, op, n, rct=(6, 0)),
    }

    def timed(fn, reps):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        for _ in range(reps):
            fn()
        host = (time.perf_counter() - t0) / reps
        return ctx.timer_stop() / reps, host * 1e3

    for fn in calls.values():
        fn()
    samples = {name: [] for name in calls}
    for _ in range(5):
        for name, fn in calls.items():
            samples[name].append(timed(fn, 20))
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    result = {"size": n, "levels": nl, "cell": cell, "cells_of_the_two_finest_levels": cells, "runs": {}}
    def issue_ms(fn):
        """host-clock time of issuing ONE call on an idle stream: in the loops above the host runs into the queue"""
        v = []
        for _ in range(9):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            v.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(v), 4)

    for name, fn in calls.items():
        ctx.kernel_timing(True)
        ctx.kernel_timing_reset()
        fn()
        ctx.sync()
        timers = {k: {"ms": round(ms, 4), "n": cnt} for k, (ms, cnt) in ctx.kernel_times().items()}
        ctx.kernel_timing(False)
        result["runs"][name] = {"ms": stat([x[0] for x in samples[name]]), "host_ms": stat([x[1] for x in samples[name]]),
                                "issue_one_call_host_ms": issue_ms(fn), "kernel_timers": timers}
    kinds = [lib.squeeze_tile_kinds(full, tiles, bw, bh, nl - 1 - k, n_planes=3) for k in range(2)]
    result["kinds_of_the_two_finest_levels"] = [{str(v): int((kd == v).sum()) for v in (0, 1, 2)} for kd in kinds]
    # behind the regular prefix (one jxlh_unsqueeze_chain of its levels): the list copy, then per mixed level the smooth
    # cells and the regular runs, then the RCT
    result["launches_behind_the_prefix"] = {"copies": 1, "kernels": 2 * 2 + 1}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
