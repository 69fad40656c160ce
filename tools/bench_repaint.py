"""Cost of repainting one group of an upsampled frame against the whole run it replaces (a measurement tool, not a test).

Two workloads: an 8192 x 8192 result from a 4096 x 4096 coded d1 frame (Gaborish + EPF 2) at upsampling 2, with and
without noise, and a 1024 x 1024 coded frame at upsampling 8.  After a whole jxlh_frame_run one group in the middle of the
frame is submitted again and
  repaint   jxlh_frame_repaint_groups of that group, against
  whole     the whole jxlh_frame_run, the only thing there was for an upsampled frame before;
  upsample  the k_upsample_rows launches of the repaint, against the three whole-frame k_upsample launches scaled by the
            share of coded rows the repaint upsamples (what a perfect row-range kernel of the same speed would take);
  save      jxlh_frame_save_rects of jxlh_repaint_changed_rects' rects into device memory (opaque RGBA8), against the whole
            jxlh_frame_save.
One JSON line per workload: for each pair the median over `reps` alternated repetitions of the mean of `steps` calls,
with min and max -- `device` from the library's event timers (all labels summed, or the one named), `host` from a host
clock around the calls and one jxlh_ctx_sync.

  python tools/bench_repaint.py [--steps 20] [--reps 5] [--small]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
XYB = [11.03, -9.87, -0.16, -3.25, 4.42, -0.16, -3.66, 2.71, 1.95, -0.156, -0.156, -0.156, -0.0038, -0.0038, -0.0038, 1.0]


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="512 x 512 coded frames: a dry run of the tool")
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    cases = [("x2", 4096, 2, False), ("x2_noise", 4096, 2, True), ("x8", 1024, 8, False)]
    ctx = jxl_rs_amd.Context(0, 1)
    for name, size, n, noise in cases:
        if a.small:
            size = 512
        wl = synth.make_vardct(size, size, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True, lf_smoothing=True)
        p = synth.apply_opts(ctx.default_params(size, size), wl)
        p.upsampling = n
        if noise:
            p.noise, p.visible_frame_index = 1, 3
            for i in range(8):
                p.noise_lut[i] = 0.05 + 0.01 * i
        ctx.frame_begin(p)
        ctx.set_dequant_tables(wl.tables)
        ctx.set_lf_quantized(*wl.lf_q)
        ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
        for g in range(wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        ctx.frame_run()
        ctx.sync()
        xg = (size + 255) // 256
        group = [(xg // 2) * xg + xg // 2]
        rects = ctx.repaint_changed_rects(group)
        colour = ctx.output_desc(lib.COLOR_XYB, "srgb", np.float32(XYB))
        d = lib.save_desc(channels=[0, 1, 2], format=lib.SAVE_U8, fill_opaque_alpha=True)
        out_w = size * n
        dev = lib.DeviceArray(nbytes=out_w * out_w * 4)
        bpr = out_w * 4

        def repaint():
            ctx.submit_group(group[0], wl.coeffs[group[0]])  # the later pass: the cost does not depend on the values
            ctx.slot_wait(0)
            ctx.repaint_groups(group)

        def whole():
            ctx.frame_run()

        def save_rects():
            st, _ = ctx.try_frame_save_rects(d, rects, colour, out=dev.ptr, bytes_per_row=bpr, wait=False)
            assert st == lib.OK, st

        def save_whole():
            ctx.frame_save(d, colour, out=dev.ptr, bytes_per_row=bpr, wait=False)

        def device_ms(fn, labels=None):
            ctx.kernel_timing_reset()
            ctx.kernel_timing(True)
            for _ in range(a.steps):
                fn()
            ctx.sync()
            kt = ctx.kernel_times()
            ctx.kernel_timing(False)
            return sum(v[0] for k, v in kt.items() if labels is None or k in labels) / a.steps

        def host_ms(fn):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
                ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / a.steps

        for fn in (repaint, whole, save_rects, save_whole):
            fn()
        ctx.sync()
        m = {k: [] for k in ("repaint_dev", "whole_dev", "repaint_host", "whole_host", "rows_dev", "ups_dev", "save_rects_dev",
                             "save_whole_dev", "save_rects_host", "save_whole_host")}
        for _ in range(a.reps):  # the ways alternate
            m["repaint_dev"].append(device_ms(repaint))
            m["whole_dev"].append(device_ms(whole))
            m["repaint_host"].append(host_ms(repaint))
            m["whole_host"].append(host_ms(whole))
            m["rows_dev"].append(device_ms(repaint, ["k_upsample_rows"]))
            m["ups_dev"].append(device_ms(whole, ["k_upsample"]))
            m["save_rects_dev"].append(device_ms(save_rects, ["k_save_rects"]))
            m["save_whole_dev"].append(device_ms(save_whole, ["k_save"]))
            m["save_rects_host"].append(host_ms(save_rects))
            m["save_whole_host"].append(host_ms(save_whole))
        # the coded rows a repaint of one group upsamples: its 256 rows, the stage list's reach (4) and the window (2)
        gy = group[0] // xg
        rows = min(size, gy * 256 + 256 + 6) - max(0, gy * 256 - 6)
        row = {"case": name, "coded": f"{size}x{size}", "result": f"{out_w}x{out_w}", "upsampling": n, "noise": noise,
               "steps": a.steps, "reps": a.reps, "upsampled_rows": rows, "row_share": rows / size,
               "rect_pixels": int(sum(int(r[2]) * int(r[3]) for r in rects))}
        row.update({k: stats(v) for k, v in m.items()})
        row["ups_dev_scaled_by_row_share"] = statistics.median(m["ups_dev"]) * rows / size
        print(json.dumps(row), flush=True)
        dev.free()
    ctx.close()


if __name__ == "__main__":
    main()
