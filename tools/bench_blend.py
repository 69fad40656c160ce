"""Cost of frame blending (k_blend.hip) on an 8192 x 8192 image (a measurement tool, not a test).

For 0 and 1 extra channels, three compositions of a rendered VarDCT frame onto the image from reference slot 0:
  full      a full-size frame, mode Blend            every pixel blended
  crop25    a 4096 x 4096 frame (25 % of the area) at (2049, 2051), mode Blend
  extend    the same cropped frame, mode Replace     the frame's pixels replace, the rest is the extend stage's copy
Each row of the table, one JSON line each:
  k_blend_ms   the kernel alone, from the library's event timers: median over `reps` repetitions of the mean of `steps`
               launches, with the smallest and largest repetition
  bytes        by the kernel's own model: (3 + ec) x 4 B x (2 reads + 1 write) per pixel of frame and image,
               (3 + ec) x 4 B x 2 per pixel outside the frame
  TBps         bytes / k_blend_ms
  copy_ms / copy_TBps   a hipMemcpyAsync device-to-device copy of bytes / 2 (so that read + written = bytes), in the same
               process, timed the same number of times: the yardstick
  frame_ms / frame_blend_ms   jxlh_frame_run alone and followed by jxlh_frame_blend, host clock around `steps` calls

  python tools/bench_blend.py [--size 8192] [--steps 20] [--reps 5] [--kernel-only CASE] [--rects]
--kernel-only CASE (e.g. crop25_ec1): that composition a few times and nothing else, for a profiler run of its own.
--rects: blend rectangles (k_blend_rects.hip, jxlh_frame_blend_rects) instead.  For the full frame and the crop, 0 and 1
extra channels, three lists recomposed in the canvas a whole blend left:
  group     the changed rects of one re-rendered group in the middle of the frame (jxlh_changed_rects, mapped by
            jxlh_blend_image_rects)
  row       ... of one whole group row
  image     one image-sized rect: the whole blend's work through the rect kernel
One JSON line each: k_blend_rects_ms (as k_blend_ms above), the bytes of the rects by the same model, and the two
yardsticks timed alternately in the same process: k_blend_ms, the whole jxlh_frame_blend that was the only route, and
k_save_rects_ms, jxlh_frame_save_rects of the same list as RGB8 into device memory."""
import argparse
import ctypes as C
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-only")
    ap.add_argument("--rects", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    size, half = a.size, a.size // 2
    rng = np.random.default_rng(1)
    hip = lib.DeviceArray.hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    frames = {}

    def frame(n):
        if n not in frames:
            frames[n] = synth.make_vardct(n, n, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True,
                                          lf_smoothing=True)
        return frames[n]

    def prepare(ctx, n, num_ec):
        wl = frame(n)
        ctx.frame_begin(synth.apply_opts(ctx.default_params(n, n), wl))
        ctx.set_dequant_tables(wl.tables)
        ctx.set_lf_quantized(*wl.lf_q)
        ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
        for g in range(wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        for i in range(num_ec):
            ctx.set_extra_channel(i, rng.integers(0, 256, size=(n, n)).astype(np.int32), 8)

    def copy_ms(nbytes, n):
        src, dst = lib.DeviceArray(nbytes=nbytes), lib.DeviceArray(nbytes=nbytes)
        for _ in range(3):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        t0 = time.perf_counter()
        for _ in range(n):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        ms = (time.perf_counter() - t0) * 1e3 / n
        src.free()
        dst.free()
        return ms

    def timed(ctx, label, call):
        """mean kernel ms of `steps` calls, from the library's event timers"""
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        for _ in range(a.steps):
            call()
        ctx.sync()
        kt = ctx.kernel_times()
        ctx.kernel_timing(False)
        return kt[label][0] / kt[label][1]

    def bench_rects(ctx, tag, n, x0, y0, d, nch):
        wl = frame(n)
        xg, yg = wl.xgroups, wl.ygroups
        mid = (yg // 2) * xg + xg // 2
        whole = np.array([[0, 0, size, size]], dtype=np.uint32)
        lists = [("group", lib.blend_image_rects(d, n, n, ctx.changed_rects([mid]))),
                 ("row", lib.blend_image_rects(d, n, n, ctx.changed_rects(list(range((yg // 2) * xg, (yg // 2 + 1) * xg))))),
                 ("image", whole)]
        sd = lib.save_desc([0, 1, 2], lib.SAVE_U8)
        paint = lib.DeviceArray(nbytes=size * size * 3)
        for name, rects in lists:
            px = inside = 0
            for rx, ry, rw, rh in rects.tolist():
                px += rw * rh
                inside += max(0, min(rx + rw, x0 + n) - max(rx, x0)) * max(0, min(ry + rh, y0 + n) - max(ry, y0))
            nbytes = nch * 4 * (3 * inside + 2 * (px - inside))
            r_ms, b_ms, s_ms = [], [], []
            ctx.blend_rects(d, rects)
            ctx.sync()
            for _ in range(a.reps):  # the rect kernel and its two yardsticks alternate
                r_ms.append(timed(ctx, "k_blend_rects", lambda: ctx.blend_rects(d, rects)))
                b_ms.append(timed(ctx, "k_blend", lambda: ctx.blend(d)))
                s_ms.append(timed(ctx, "k_save_rects", lambda: ctx.frame_save_rects_async(sd, rects, out=paint, bytes_per_row=size * 3)))
            rm = statistics.median(r_ms)
            print(json.dumps({
                "case": f"{tag}_{name}", "image": f"{size}x{size}", "frame": f"{n}x{n} at ({x0}, {y0})", "channels": nch,
                "rects": len(rects), "pixels": px, "bytes": nbytes, "k_blend_rects_ms": rm,
                "k_blend_rects_ms_min_max": [min(r_ms), max(r_ms)], "TBps": nbytes / rm * 1e-9,
                "k_blend_ms": statistics.median(b_ms), "k_blend_ms_min_max": [min(b_ms), max(b_ms)],
                "k_save_rects_ms": statistics.median(s_ms), "k_save_rects_ms_min_max": [min(s_ms), max(s_ms)],
            }), flush=True)
        paint.free()

    cases = [("full", size, 0, 0, lib.BLEND_BLEND), ("crop25", half, half // 2 + 1, half // 2 + 3, lib.BLEND_BLEND),
             ("extend", half, half // 2 + 1, half // 2 + 3, lib.BLEND_REPLACE)]
    for num_ec in (0, 1):
        nch = 3 + num_ec
        ctx = jxl_rs_amd.Context(0, 1)
        ctx.set_reference(0, [rng.random((size, size), dtype=np.float32) for _ in range(nch)])
        for name, n, x0, y0, mode in cases:
            tag = f"{name}_ec{num_ec}"
            if a.kernel_only and a.kernel_only != tag:
                continue
            prepare(ctx, n, num_ec)
            d = lib.blend_desc(x0, y0, size, size, (mode, 0, 1, 0), [(mode, 0, 1, 0)] * num_ec, [lib.EC_ALPHA] * num_ec)
            ctx.frame_run()
            ctx.blend(d)
            ctx.sync()
            if a.kernel_only:
                for _ in range(5):
                    ctx.blend(d)
                ctx.sync()
                continue
            if a.rects:
                if name != "extend":
                    bench_rects(ctx, tag, n, x0, y0, d, nch)
                continue
            inside = n * n
            nbytes = nch * 4 * (3 * inside + 2 * (size * size - inside))
            k_ms, c_ms = [], []
            for _ in range(a.reps):  # kernel and yardstick alternate
                ctx.kernel_timing_reset()
                ctx.kernel_timing(True)
                for _ in range(a.steps):
                    ctx.blend(d)
                ctx.sync()
                kt = ctx.kernel_times()
                ctx.kernel_timing(False)
                k_ms.append(kt["k_blend"][0] / kt["k_blend"][1])
                c_ms.append(copy_ms(nbytes // 2, a.steps))

            def steps_ms(with_blend):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    ctx.frame_run()
                    if with_blend:
                        ctx.blend(d)
                ctx.sync()
                return (time.perf_counter() - t0) * 1e3 / a.steps
            f_ms, fb_ms = [], []
            for _ in range(a.reps):
                f_ms.append(steps_ms(False))
                fb_ms.append(steps_ms(True))
            km, cm = statistics.median(k_ms), statistics.median(c_ms)
            print(json.dumps({
                "case": tag, "image": f"{size}x{size}", "frame": f"{n}x{n} at ({x0}, {y0})", "channels": nch,
                "bytes": nbytes, "k_blend_ms": km, "k_blend_ms_min_max": [min(k_ms), max(k_ms)], "TBps": nbytes / km * 1e-9,
                "copy_ms": cm, "copy_ms_min_max": [min(c_ms), max(c_ms)], "copy_TBps": nbytes / cm * 1e-9,
                "frame_ms": statistics.median(f_ms), "frame_blend_ms": statistics.median(fb_ms),
            }), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
