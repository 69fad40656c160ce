"""Cost of the patches stage on the bench's 8K d1 frame (a measurement tool, not a test).

Workload: the 8192 x 8192 d1 frame of bench.py with one alpha extra channel, plus a screen-like dictionary -- glyph
patches of 8-16 x 12-24 px cut from a 1024 x 256 reference slot, half Replace, half BlendAbove over the alpha channel.
Reports, as one JSON line: the frame ms without and with the dictionary (two contexts, the two variants alternated on
each, median of 5 x `steps` steps), the host binning time of jxlh_frame_set_patches, the k_patches time from the
library's event timers, the covered pixels and the bytes the kernel moves per covered pixel (3 + ec reference floats
read, 3 + ec frame floats read and written) over that time, as a fraction of 8 TB/s.

  python tools/bench_patches.py [--patches 36000] [--steps 20] [--reps 5] [--kernel-only] [--rocprof-db DB]
--kernel-only: one context, a few patched frames, nothing else (for a rocprofv3 --kernel-trace --stats run);
--rocprof-db: print the k_patches dispatch times (ms) that run recorded in its rocpd database, and the bandwidth."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dictionary(np, rng, size, n, ref_w=1024, ref_h=256):
    patches, blendings = [], []
    for i in range(n):
        xs, ys = int(rng.integers(8, 17)), int(rng.integers(12, 25))
        patches.append((int(rng.integers(0, size - xs + 1)), int(rng.integers(0, size - ys + 1)), 0,
                        int(rng.integers(0, ref_w - xs + 1)), int(rng.integers(0, ref_h - ys + 1)), xs, ys))
        mode = 1 if i % 2 == 0 else 4  # Replace / BlendAbove
        blendings += [(mode, 0, 0), (mode, 0, 0)]
    return patches, blendings


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--patches", type=int, default=36000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--rocprof-db")
    ap.add_argument("--covered-px", type=int, default=0, help="with --rocprof-db: covered pixels of the workload")
    a = ap.parse_args()
    if a.rocprof_db:
        import sqlite3
        db = sqlite3.connect(a.rocprof_db)
        ms = [r[0] * 1e-6 for r in db.execute("select end - start from kernels where name like '%k_patches%'")]
        covered = a.covered_px
        print(json.dumps({"k_patches_ms_rocprofv3": ms, "median_ms": statistics.median(ms) if ms else None,
                          "GBps_at_48B_per_covered_px": covered * 48 / (statistics.median(ms) * 1e-3) / 1e9 if ms and covered else None}))
        return
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import synth
    size = a.size
    rng = np.random.default_rng(1)
    wl = synth.make_vardct(size, size, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True,
                           lf_smoothing=True)
    ref = [rng.uniform(0.0, 1.0, (256, 1024)).astype(np.float32) for _ in range(4)]
    alpha = rng.integers(0, 256, size=(size, size)).astype(np.int32)
    patches, blendings = dictionary(np, rng, size, a.patches)
    cover = np.zeros((size, size), bool)
    for x, y, _, _, _, xs, ys in patches:
        cover[y:y + ys, x:x + xs] = True
    covered = int(cover.sum())
    del cover

    def prepare(ctx):
        ctx.frame_begin(synth.apply_opts(ctx.default_params(size, size), wl))
        ctx.set_dequant_tables(wl.tables)
        ctx.set_lf_quantized(*wl.lf_q)
        ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
        for g in range(wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        ctx.set_reference(0, ref)
        ctx.set_extra_channel(0, alpha, 8)

    def set_dict(ctx, on):
        t0 = time.perf_counter()
        ctx.set_patches(patches if on else [], blendings if on else [], [1])
        return (time.perf_counter() - t0) * 1e3

    def steps_ms(ctx, n):
        ctx.frame_run()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(n):
            ctx.frame_run()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / n

    if a.kernel_only:
        ctx = jxl_rs_amd.Context(0, 1)
        prepare(ctx)
        set_dict(ctx, True)
        steps_ms(ctx, 5)
        ctx.close()
        return
    ctxs = [jxl_rs_amd.Context(0, 1), jxl_rs_amd.Context(0, 1)]
    for c in ctxs:
        prepare(c)
    plain, patched, bin_ms = [], [], []
    for r in range(a.reps):
        for i, c in enumerate(ctxs):
            for on in ((False, True) if (r + i) % 2 == 0 else (True, False)):
                t = set_dict(c, on)
                if on:
                    bin_ms.append(t)
                (patched if on else plain).append(steps_ms(c, a.steps))
    c = ctxs[0]
    set_dict(c, True)
    c.frame_run()
    c.sync()
    c.kernel_timing_reset()
    c.kernel_timing(True)
    for _ in range(a.steps):
        c.frame_run()
    c.sync()
    kt = c.kernel_times()
    c.kernel_timing(False)
    k_ms = kt["k_patches"][0] / max(1, kt["k_patches"][1]) if "k_patches" in kt else float("nan")
    nch = 3 + 1
    bytes_moved = covered * nch * 4 * 3
    out = {
        "workload": f"{size}x{size} d1 + 1 alpha EC, {len(patches)} glyph patches (half Replace, half BlendAbove)",
        "covered_px": covered, "covered_fraction": covered / float(size * size),
        "frame_ms_plain": statistics.median(plain), "frame_ms_patched": statistics.median(patched),
        "frame_ms_delta": statistics.median(patched) - statistics.median(plain),
        "plain_ms_all": plain, "patched_ms_all": patched,
        "set_patches_host_ms": statistics.median(bin_ms),
        "k_patches_ms_event": k_ms, "bytes_per_covered_px": nch * 4 * 3,
        "k_patches_GBps": bytes_moved / (k_ms * 1e-3) / 1e9 if k_ms == k_ms else None,
    }
    if out["k_patches_GBps"]:
        out["fraction_of_8TBps"] = out["k_patches_GBps"] / 8000.0
    for c in ctxs:
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
