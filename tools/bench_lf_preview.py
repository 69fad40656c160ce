"""Cost of the LF-frame preview (k_lf_preview.hip) on an 8192 x 8192 image, slot 1024 x 1024, RGBA8 sRGB into device
memory (a measurement tool, not a test).  One JSON line per orientation (1 and 6):
  preview_ms     the kernel alone, from the library's event timers: median over `reps` repetitions of the mean of `steps`
                 launches, with the smallest and largest repetition
  preview_call_ms  the same launches between jxlh_timer_start / _stop (what the composed route is timed with)
  composed_ms    orientation 1 only: the route a caller had before -- jxlh_stage_upsample(8) on the three slot planes
                 (device to device), then jxlh_stage_save of the three upsampled planes -- between jxlh_timer_start / _stop,
                 alternated with the preview.  It cannot reproduce the preview's dither phase; the bytes moved are the
                 point.
  copy_ms        a device-to-device copy kernel of the output's bytes (jxlh_probe_copy_bandwidth: on the context's
                 stream, timed with device events like the preview), alternated with the preview
  vs_copy        copy_ms / preview_ms: the preview's fraction of the copy's rate at the same output size
  vs_composed    composed_ms / preview_call_ms
  vs_identity    orientation 6: preview_ms of orientation 1 over this one's

  python tools/bench_lf_preview.py [--size 8192] [--steps 20] [--reps 5] [--kernel-only ORIENTATION]
--kernel-only: that preview a few times and nothing else, for a profiler run of its own."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# jxlh_xyb_params: plausible magnitudes; the values do not matter to the time
XYB = [11.03, -9.87, -0.16, -3.25, 4.42, -0.16, -3.66, 2.71, 1.95, -0.156, -0.156, -0.156, -0.0038, -0.0038, -0.0038, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int)
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n = a.size
    s = (n + 7) // 8
    rng = np.random.default_rng(1)
    ctx = jxl_rs_amd.Context(0, 1)
    planes = [rng.uniform(-0.02, 0.02, (s, s)).astype(np.float32), rng.uniform(0.0, 0.9, (s, s)).astype(np.float32),
              rng.uniform(0.0, 0.9, (s, s)).astype(np.float32)]
    ctx.set_lf_frame(0, *planes)
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", np.float32(XYB))
    out_bytes = n * n * 4
    out = lib.DeviceArray(nbytes=out_bytes)

    def preview(d):
        ctx.lf_preview(0, n, n, d, colour, out=out.ptr, bytes_per_row=n * 4, wait=False)

    def kernel_ms(fn):
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        for _ in range(a.steps):
            fn()
        ctx.sync()
        kt = ctx.kernel_times()
        ctx.kernel_timing(False)
        return kt["k_lf_preview"][0] / kt["k_lf_preview"][1]

    def call_ms(fn):
        ctx.timer_start()
        for _ in range(a.steps):
            fn()
        return ctx.timer_stop() / a.steps

    def copy_ms(nbytes):
        # jxlh_probe_copy_bandwidth: a float4 copy kernel on the context's stream, timed with device events like the
        # preview (the better of plain and non-temporal accesses); GB/s counts bytes read + written
        return 2 * nbytes / (ctx.probe_copy_bandwidth(nbytes, a.steps) * 1e9) * 1e3

    if a.kernel_only:
        d = lib.save_desc([0, 1, 2], lib.SAVE_U8, fill_opaque_alpha=True, orientation=a.kernel_only)
        for _ in range(6):
            preview(d)
        ctx.sync()
        return

    # the composed route's buffers: the slot planes and the upsampled planes on the device
    slot_dev = [lib.DeviceArray(p) for p in planes]
    up_dev = [lib.DeviceArray(nbytes=n * n * 4) for _ in range(3)]
    d1 = lib.save_desc([0, 1, 2], lib.SAVE_U8, fill_opaque_alpha=True)

    def composed():
        for c in range(3):
            ctx._chk(ctx.L.jxlh_stage_upsample(ctx._ctx, 8, slot_dev[c].ptr, up_dev[c].ptr, s, s), "stage_upsample")
        ctx.stage_save(d1, [u.ptr for u in up_dev], colour, out=out.ptr, bytes_per_row=n * 4, size=(n, n))

    identity = None
    for o in (1, 6):
        d = lib.save_desc([0, 1, 2], lib.SAVE_U8, fill_opaque_alpha=True, orientation=o)
        preview(d)
        ctx.sync()
        if o == 1:
            composed()
        k, pc, cp, co = [], [], [], []
        for _ in range(a.reps):  # the preview and its yardsticks alternate
            k.append(kernel_ms(lambda: preview(d)))
            pc.append(call_ms(lambda: preview(d)))
            cp.append(copy_ms(out_bytes))
            if o == 1:
                co.append(call_ms(composed))
        km, pm, cm = statistics.median(k), statistics.median(pc), statistics.median(cp)
        row = {"case": f"rgba8_srgb_o{o}", "image": f"{n}x{n}", "slot": f"{s}x{s}", "out_bytes": out_bytes,
               "preview_ms": km, "preview_ms_min_max": [min(k), max(k)], "preview_call_ms": pm,
               "preview_call_ms_min_max": [min(pc), max(pc)], "copy_ms": cm, "copy_ms_min_max": [min(cp), max(cp)],
               "vs_copy": cm / km}
        if o == 1:
            com = statistics.median(co)
            row.update({"composed_ms": com, "composed_ms_min_max": [min(co), max(co)], "vs_composed": com / pm})
            identity = km
        else:
            row["vs_identity"] = identity / km
        print(json.dumps(row), flush=True)
    for b in slot_dev + up_dev + [out]:
        b.free()
    ctx.close()


if __name__ == "__main__":
    main()
