#!/usr/bin/env python3
"""The in-process sharded run on one GPU: three ranks, the 520 x 1000 frame of tests/test_gpu_sharding.py (four group
rows: bands of 2, 2 and 0), `--iters` times jxlh_frames_run_sharded_local + jxlh_frames_allgather_local between two
syncs, `--reps` times; reports the median per iteration of the whole loop (ms_per_iter) and of the host's share, the
time until the last call has returned (host_ms_per_iter).  The calls are host routing around small kernels, so this
is where a change to comm.hip's issue path would show.  For an A/B of two builds run it once per build
(JXLH_LIBRARY=... selects another build of the library), the baseline twice for the noise.
usage: [JXLH_LIBRARY=<so>] python tools/bench_sharded_local.py [--iters 300] [--reps 9]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import jxl_rs_amd
from jxl_rs_amd import lib, synth
from jxl_rs_amd.shard import band_for_rank

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

N = 3
wl = synth.make_vardct(520, 1000, mix=synth.MIX_ALL, seed=31 + N, epf_iters=2)
ctxs = [jxl_rs_amd.Context(0, 1) for _ in range(N)]
lib.comm_init_local(ctxs)
for r, c in enumerate(ctxs):
    c.frame_begin(synth.apply_opts(c.default_params(wl.xsize, wl.ysize), wl))
    c.set_dequant_tables(wl.tables)
    c.set_lf_quantized(*wl.lf_q)
    c.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    r0, r1, _ = band_for_rank(wl.ygroups, r, N)
    for g in range(r0 * wl.xgroups, r1 * wl.xgroups):
        c.submit_group(g, wl.coeffs[g])
    c.slot_wait(0)


def loop(iters):
    for c in ctxs:
        c.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        lib.frames_run_sharded_local(ctxs)
        lib.frames_allgather_local(ctxs)
    t1 = time.perf_counter()
    for c in ctxs:
        c.sync()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3 / iters, (t1 - t0) * 1e3 / iters


loop(50)  # warm-up
runs = [loop(args.iters) for _ in range(args.reps)]
for c in ctxs:
    c.close()
print(json.dumps({"lib": os.environ.get("JXLH_LIBRARY", "tree"), "ranks": N, "frame": [wl.xsize, wl.ysize],
                  "iters": args.iters, "reps": args.reps,
                  "ms_per_iter": round(statistics.median(t for t, _ in runs), 4),
                  "host_ms_per_iter": round(statistics.median(h for _, h in runs), 4),
                  "ms_per_iter_all": [round(t, 4) for t, _ in runs]}))
