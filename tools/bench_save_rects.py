"""Cost of a repaint after a group re-render, two ways (a measurement tool, not a test).

An 8192 x 8192 d1 frame (32 x 32 groups, Gaborish + EPF 2) is rendered; k = 1, 4 and 32 groups are re-rendered
(jxlh_frame_rerender_groups; k = 4 and 32 lie on the diagonal: no two share a group row or column), and the picture is
repainted as opaque RGBA8 and as RGB f16 under orientations 1 and 6, into (a) device memory and (b) pinned host memory:
  rects   jxlh_frame_save_rects[_async] on jxlh_changed_rects' output: ONE call;
  bands   the only way without it: jxlh_frame_save[_async] over the full-width row bands that cover the same rects
          (overlapping bands merged), one call per band.
One JSON line per case:
  device  the kernels alone, from the library's event timers (labels k_save_rects / k_save, summed over a repaint's
          launches): median over `reps` alternated repetitions of the mean of `steps` repaints, with min and max;
  host    a host clock around the repaint -- the _async calls and ONE jxlh_ctx_sync, so the staging copies over the bus
          are inside (the event timers span the kernels only) --, the same statistics;
  bytes   the pixel bytes each way writes, counted from the rects.
  host_ok whether the rects' median is not slower than the bands' median by more than the bands' own min-max spread.
--full-only: jxlh_frame_save of the whole frame into device memory alone (k_save's event timer), one line per format and
  orientation: run once per build (JXLH_LIBRARY=... selects another build of the library) and alternation for an A/B
  against the parent, which has this call and not the others.

  python tools/bench_save_rects.py [--size 8192] [--steps 10] [--reps 7] [--full-only]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIBRARY = os.path.basename(os.path.dirname(os.environ.get("JXLH_LIBRARY", ""))) or "tree"
# jxlh_xyb_params: plausible magnitudes; the values do not matter to the time
XYB = [11.03, -9.87, -0.16, -3.25, 4.42, -0.16, -3.66, 2.71, 1.95, -0.156, -0.156, -0.156, -0.0038, -0.0038, -0.0038, 1.0]


def cover_bands(rects, height):
    """the full-width row bands [y0, y1) that cover the rects, overlapping or touching ones merged"""
    bands = []
    for y0, y1 in sorted((int(r[1]), min(height, int(r[1]) + int(r[3]))) for r in rects):
        if bands and y0 <= bands[-1][1]:
            bands[-1][1] = max(bands[-1][1], y1)
        else:
            bands.append([y0, y1])
    return bands


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--full-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    n = a.size
    wl = synth.make_vardct(n, n, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True, lf_smoothing=True)
    ctx = jxl_rs_amd.Context(0, 1)
    ctx.frame_begin(synth.apply_opts(ctx.default_params(n, n), wl))
    ctx.set_dequant_tables(wl.tables)
    ctx.set_lf_quantized(*wl.lf_q)
    ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
    for g in range(wl.coeffs.shape[0]):
        ctx.submit_group(g, wl.coeffs[g])
    ctx.slot_wait(0)
    ctx.frame_run()
    ctx.sync()
    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", np.float32(XYB))
    formats = [("rgba8", dict(channels=[0, 1, 2], format=lib.SAVE_U8, fill_opaque_alpha=True)),
               ("rgb_f16", dict(channels=[0, 1, 2], format=lib.SAVE_F16))]
    dev = lib.DeviceArray(nbytes=n * n * 8)
    host, _ = ctx.alloc_pinned(n * n * 8)

    def kernel_ms(fn, labels):
        """mean per repaint of the listed timer labels over `steps` repaints"""
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        for _ in range(a.steps):
            fn()
        ctx.sync()
        kt = ctx.kernel_times()
        ctx.kernel_timing(False)
        return sum(kt[l][0] for l in labels if l in kt) / a.steps

    def wall_ms(fn):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
            ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    if a.full_only:
        for fname, kw in formats:
            for o in (1, 6):
                d = lib.save_desc(orientation=o, **kw)
                bpr = n * d.pixel_bytes

                def full():
                    ctx.frame_save(d, colour, out=dev.ptr, bytes_per_row=bpr, wait=False)
                full()
                ctx.sync()
                print(json.dumps({"case": f"full_{fname}_o{o}", "library": LIBRARY, "image": f"{n}x{n}",
                                  "k_save_ms": [kernel_ms(full, ["k_save"]) for _ in range(a.reps)]}), flush=True)
        dev.free()
        ctx.close()
        return

    xg = (n + 255) // 256
    for k in (1, 4, 32):
        step = max(1, min(xg, 32) // k)
        diagonal = sorted({(i * step) % xg for i in range(k)})  # (fewer than k on a frame of fewer groups)
        groups = [i * xg + i for i in diagonal] if k > 1 else [(xg // 2) * xg + xg // 2]
        for g in groups:  # the later pass: the same coefficients again -- the repaint's cost does not depend on them
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        ctx.rerender_groups(groups)
        ctx.sync()
        rects = ctx.changed_rects(groups)
        bands = cover_bands(rects, n)
        for fname, kw in formats:
            for o in (1, 6):
                d = lib.save_desc(orientation=o, **kw)
                bpr = n * d.pixel_bytes
                row = {"case": f"k{k}_{fname}_o{o}", "library": LIBRARY, "image": f"{n}x{n}", "groups": k, "rects": len(rects),
                       "bands": len(bands), "rect_bytes": int(sum(int(r[2]) * int(r[3]) for r in rects)) * d.pixel_bytes,
                       "band_bytes": sum(y1 - y0 for y0, y1 in bands) * n * d.pixel_bytes}
                for where, out in (("device", dev.ptr), ("host", host)):
                    def by_rects():
                        st, _ = ctx.try_frame_save_rects(d, rects, colour, out=out, bytes_per_row=bpr, wait=False)
                        assert st == lib.OK, st

                    def by_bands():
                        for y0, y1 in bands:
                            st, _ = ctx.try_frame_save(d, colour, y0=y0, y1=y1, out=out, bytes_per_row=bpr, wait=False)
                            assert st == lib.OK, st
                    by_rects()
                    by_bands()
                    ctx.sync()
                    r_ms, b_ms = [], []
                    for _ in range(a.reps):  # the two ways alternate
                        if where == "device":
                            r_ms.append(kernel_ms(by_rects, ["k_save_rects"]))
                            b_ms.append(kernel_ms(by_bands, ["k_save"]))
                        else:
                            r_ms.append(wall_ms(by_rects))
                            b_ms.append(wall_ms(by_bands))
                    row[where] = {"rects_ms": stats(r_ms), "bands_ms": stats(b_ms)}
                b = row["host"]["bands_ms"]
                row["host_ok"] = row["host"]["rects_ms"]["median"] <= b["median"] + (b["max"] - b["min"])
                print(json.dumps(row), flush=True)
    dev.free()
    ctx.close()


if __name__ == "__main__":
    main()
