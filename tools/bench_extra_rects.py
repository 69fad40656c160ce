"""Cost of one arriving group of an RGBA frame, two ways (a measurement tool, not a test; it fails without a GPU).

An 8192 x 8192 d1 frame (32 x 32 groups, Gaborish + EPF 2) with one 8-bit alpha extra channel, at factor 1 (8192 x 8192
samples) and at factor 2 (4096 x 4096), is rendered on two contexts.  Then one group per step arrives with its alpha
samples -- the 256 x 256 rect of the channel that covers the group, (256 / factor)^2 samples, in pinned host memory:
  whole   the route without the rect form: jxlh_frame_set_extra_channel of the WHOLE plane (pinned, updated in place)
          + jxlh_frame_rerender_groups([g]);
  rects   jxlh_frame_set_extra_channel_rects of the one rect + jxlh_frame_rerender_groups([g]).
The two routes alternate, repetition by repetition, in one process.  One JSON line per factor:
  host    a host clock around the step, which ends in a jxlh_ctx_sync: median over `reps` repetitions of the mean of
          `steps` steps, with min and max, per route;
  kernels the new launches (k_ec_scatter, k_ec_finish) and the whole route's (k_modular_to_f32, k_upsample) from the
          library's event timers, ms per step;
  ok      whether the rects' median is below the whole route's MINIMUM.

  python tools/bench_extra_rects.py [--size 8192] [--steps 20] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    n = a.size
    wl = synth.make_vardct(n, n, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True, lf_smoothing=True)
    xg = (n + 255) // 256
    rng = np.random.default_rng(1)
    ctxs = {"whole": jxl_rs_amd.Context(0, 1), "rects": jxl_rs_amd.Context(0, 1)}  # (raises when no GPU is present)
    for up in (1, 2):
        cw = n // up
        gw = 256 // up  # a group's alpha rect, in the channel's samples
        pin, _ = ctxs["whole"].alloc_pinned(cw * cw * 4)
        plane = pin.view(np.int32).reshape(cw, cw)
        plane[:] = rng.integers(0, 256, size=(cw, cw), dtype=np.int32)
        pin_r, _ = ctxs["rects"].alloc_pinned(gw * gw * 4)
        rect = pin_r.view(np.int32)
        desc = np.zeros(1, dtype=lib.EC_RECT_DTYPE)
        for name, ctx in ctxs.items():
            ctx.frame_begin(synth.apply_opts(ctx.default_params(n, n), wl))
            ctx.set_dequant_tables(wl.tables)
            ctx.set_lf_quantized(*wl.lf_q)
            ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
            for g in range(wl.coeffs.shape[0]):
                ctx.submit_group(g, wl.coeffs[g])
            ctx.slot_wait(0)
            if name == "whole":
                ctx._chk(ctx.L.jxlh_frame_set_extra_channel(ctx._ctx, 0, plane.ctypes.data, cw, cw, cw, 8, up), "set_extra_channel")
            else:
                ctx.begin_extra_channel(0, cw, cw, 8, up)
                d = np.zeros(1, dtype=lib.EC_RECT_DTYPE)
                d[0] = (0, 0, 0, cw, cw, 0, cw)
                ctx.set_extra_channel_rects(d, block=plane)
            ctx.frame_run()
            ctx.sync()
        step_no = [0]

        def arrive(name):
            """one group arrives: new alpha samples in its rect, the hand-over, the re-render, the sync"""
            ctx = ctxs[name]
            step_no[0] += 1
            g = (step_no[0] * 37) % (xg * xg)
            x0, y0 = (g % xg) * gw, (g // xg) * gw
            if name == "whole":
                plane[y0:y0 + gw, x0:x0 + gw] ^= 1
                ctx._chk(ctx.L.jxlh_frame_set_extra_channel(ctx._ctx, 0, plane.ctypes.data, cw, cw, cw, 8, up), "set_extra_channel")
            else:
                rect[:] = (step_no[0] * 7) & 0xff
                desc[0] = (0, x0, y0, gw, gw, 0, gw)
                st, _ = ctx.try_set_extra_channel_rects(rect, desc, wait=False)  # (contiguous i32: passed where it lies)
                assert st == lib.OK, st
            ctx.rerender_groups([g])
            ctx.sync()

        def wall_ms(name):
            ctxs[name].sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                arrive(name)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        def kernel_ms(name, labels):
            ctx = ctxs[name]
            ctx.kernel_timing_reset()
            ctx.kernel_timing(True)
            for _ in range(a.steps):
                arrive(name)
            kt = ctx.kernel_times()
            ctx.kernel_timing(False)
            return {l: kt[l][0] / a.steps for l in labels if l in kt}
        for name in ctxs:
            arrive(name)  # warm-up: allocations, first launches
        ms = {"whole": [], "rects": []}
        for _ in range(a.reps):  # the two routes alternate
            for name in ("whole", "rects"):
                ms[name].append(wall_ms(name))
        row = {"case": f"alpha_x{up}", "image": f"{n}x{n}", "channel": f"{cw}x{cw}", "rect": f"{gw}x{gw}", "steps": a.steps,
               "reps": a.reps, "host": {k: stats(v) for k, v in ms.items()},
               "kernels": {"whole": kernel_ms("whole", ["k_modular_to_f32", "k_upsample"]),
                           "rects": kernel_ms("rects", ["k_ec_scatter", "k_ec_finish"])}}
        row["ok"] = row["host"]["rects"]["median"] < row["host"]["whole"]["min"]
        print(json.dumps(row), flush=True)
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
