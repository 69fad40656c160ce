"""Cost of the fill of groups whose HF has not arrived (k_lf_fill.hip, jxlh_frame_set_groups_lf_only) on the bench's
8K d1 frame (a measurement tool, not a test).  One JSON line per case:
  none         (i)   no group marked: the frame as bench.py runs it
  lower_half   (ii)  the lower half of the group rows marked, as for a file arriving top to bottom
  all          (iii) every group marked: the first paint
  zero_coeffs  (iv)  no group marked, every group submitted with all-zero coefficients: the only first paint a library
                     without the call offers (blocky LLF-only pixels) -- its K1 time is what (iii)'s K1 + fill is held to
With JXLH_LIBRARY pointing at a build without the call, (ii) and (iii) are skipped: (i) and (iv) are the parent's
figures, taken by the same tool.
All cases run on one context (one placement of its buffers).  `reps` repetitions alternate over the cases; entering a
case resubmits the coefficients or marks the groups and runs `warmup` frames; a repetition is `steps` jxlh_frame_run calls between
jxlh_timer_start / _stop (the stop synchronises inside the timed window), then `steps` more with the library's event
timers on for the per-kernel times.  Reported: median, min and max over the repetitions of ms per run, of K1, the fill
and the filters; the fill's bytes from the shapes (per marked block 3 x 256 B written and 3 x 4 B read) and its share of
8 TB/s.

  python tools/bench_lf_fill.py [--size 8192] [--steps 20] [--warmup 3] [--reps 5] [--seed 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import synth
    n = a.size
    wl = synth.make_vardct(n, n, mix=synth.MIX_D1, seed=a.seed, unique_groups=24, epf_iters=2, gab=True, lf_smoothing=True)
    ngroups = wl.xgroups * wl.ygroups
    has_call = hasattr(jxl_rs_amd.lib.load(), "jxlh_frame_set_groups_lf_only")
    zero = np.zeros((3, 65536), np.int32)

    def blocks_of(groups):
        t = 0
        for g in groups:
            gx, gy = g % wl.xgroups, g // wl.xgroups
            t += min(32, wl.xblocks - gx * 32) * min(32, wl.yblocks - gy * 32)
        return t

    cases = [("none", [], False), ("zero_coeffs", [], True)]
    if has_call:
        cases[1:1] = [("lower_half", list(range((wl.ygroups // 2) * wl.xgroups, ngroups)), False),
                      ("all", list(range(ngroups)), False)]
    # ONE context: where the driver places a context's buffers moves K1 by up to 10 % (jxlh_ctx_tune_placement), so every
    # case runs on the same planes and coefficient store.  Switching the case resubmits (which clears the marks) or marks.
    c = jxl_rs_amd.Context(0, 1)
    c.frame_begin(synth.apply_opts(c.default_params(n, n), wl))
    c.set_dequant_tables(wl.tables)
    c.set_lf_quantized(*wl.lf_q)
    c.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)

    def enter(name, marked, zeros):
        if not marked:
            for g in range(ngroups):
                c.submit_group(g, zero if zeros else wl.coeffs[g])
            c.slot_wait(0)
        else:
            c.set_groups_lf_only(marked)  # (behind the submissions: a later mark wins)
        for _ in range(a.warmup):
            c.frame_run()
        c.sync()

    wall = {k[0]: [] for k in cases}
    kern = {k[0]: {} for k in cases}
    for _ in range(a.reps):
        for name, marked, zeros in cases:
            enter(name, marked, zeros)
            c.timer_start()
            for _ in range(a.steps):
                c.frame_run()
            wall[name].append(c.timer_stop() / a.steps)
            c.sync()
            c.kernel_timing_reset()
            c.kernel_timing(True)
            for _ in range(a.steps):
                c.frame_run()
            c.sync()
            kt = c.kernel_times()
            c.kernel_timing(False)
            for k in ("k1_vardct", "k_lf_fill", "k23_fused_filters"):
                ms, launches = kt.get(k, (0.0, 0))
                kern[name].setdefault(k, []).append(ms / a.steps if launches else 0.0)

    def mmm(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}

    for name, marked, zeros in cases:
        row = {"case": name, "image": f"{n}x{n}", "groups": ngroups, "marked": len(marked), "steps": a.steps, "reps": a.reps,
               "library": os.path.basename(os.environ.get("JXLH_LIBRARY", "libjxl_hip.so")), "ms_per_run": mmm(wall[name]),
               "k1_ms": mmm(kern[name]["k1_vardct"]), "fill_ms": mmm(kern[name]["k_lf_fill"]),
               "filters_ms": mmm(kern[name]["k23_fused_filters"])}
        row["k1_plus_fill_ms"] = row["k1_ms"]["median"] + row["fill_ms"]["median"]
        if marked:
            nb = blocks_of(marked)
            row["fill_bytes_written"] = nb * 64 * 4 * 3
            row["fill_bytes_read"] = nb * 4 * 3
            t = row["fill_ms"]["median"] * 1e-3
            row["fill_share_of_8TBps"] = (row["fill_bytes_written"] + row["fill_bytes_read"]) / t / HBM_BYTES_PER_S if t > 0 else None
        print(json.dumps(row), flush=True)
    c.close()


if __name__ == "__main__":
    main()
