"""Cost of the save tail (k_save.hip) on an 8192 x 8192 frame with one extra channel (a measurement tool, not a test).

Cases, each under orientations 1 (identity), 3 (rotate 180) and 6 (rotate 90 cw), into device memory, behind the
XYB + sRGB colour stage:
  rgba8_alpha   RGBA 8 bit, alpha from the extra channel      16 B/px in, 4 B/px out
  rgba8_filled  RGBA 8 bit, opaque fill                       12 B/px in, 4 B/px out
  rgb16         RGB 16 bit                                    12 B/px in, 6 B/px out
  rgba_f16      RGBA half floats, alpha from the extra channel 16 B/px in, 8 B/px out
  gray8         channel 0 alone, 8 bit                        12 B/px in (the colour stage reads three planes), 1 B/px out
One JSON line per case and orientation:
  k_save_ms    the kernel alone, from the library's event timers: median over `reps` repetitions of the mean of `steps`
               launches, with the smallest and largest repetition
  bytes / TBps bytes read and written, counted from the shapes, over k_save_ms
  copy_ms / copy_TBps / vs_copy   a hipMemcpyAsync device-to-device copy of bytes / 2 (read + written = bytes),
               alternated with the kernel: the first yardstick
  shipped_ms / vs_shipped   rgba8_filled, orientation 1 only: jxlh_frame_read_rgb8 (k_xyb_to_rgb8<4, sRGB>, which moves the
               same bytes) on the same frame, alternated with the kernel: the second yardstick
  vs_identity  orientations 3 and 6: k_save_ms of orientation 1 of the same case over this one's

  python tools/bench_save.py [--size 8192] [--steps 20] [--reps 5] [--shipped-only] [--kernel-only CASE]
                             [--readouts] [--merge FILE ...]
--shipped-only: jxlh_frame_read_rgb8 alone (the calls an older build of the library has: JXLH_LIBRARY=... runs the parent's).
--kernel-only CASE (e.g. rgba8_alpha_o6): that save a few times and nothing else, for a profiler run of its own.
--readouts: the integer read-outs into device memory by their timer labels (which name the read-out, whatever kernel
  serves it): jxlh_frame_read_rgb8 / _rgb16 with 3 and 4 channels on the XYB frame, and jxlh_frame_read_ycbcr_rgb8 on a
  4:2:0 frame without filters (the chroma-fused kernel).  One JSON line per case: `ms` = the mean of `steps` launches,
  once per repetition.  For an A/B of two builds run it once per build and alternation (JXLH_LIBRARY, --reps 1) ...
--merge FILE ...: ... and merge the lines of all runs: per case and library the median, min-max and TB/s, and whether
  the second library's median is within the first's own min-max spread of the first's median."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIBRARY = os.path.basename(os.path.dirname(os.environ.get("JXLH_LIBRARY", ""))) or "tree"

# jxlh_xyb_params (inverse matrix, cbrt(bias), scaled bias, intensity scale): plausible magnitudes; the values do not
# matter to the time
XYB = [11.03, -9.87, -0.16, -3.25, 4.42, -0.16, -3.66, 2.71, 1.95, -0.156, -0.156, -0.156, -0.0038, -0.0038, -0.0038, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shipped-only", action="store_true")
    ap.add_argument("--kernel-only")
    ap.add_argument("--readouts", action="store_true")
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge)
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    n = a.size
    px = n * n
    rng = np.random.default_rng(1)
    hip = lib.DeviceArray.hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = jxl_rs_amd.Context(0, 1)

    def render(wl, extra_channel=False):
        ctx.frame_begin(synth.apply_opts(ctx.default_params(n, n), wl))
        ctx.set_dequant_tables(wl.tables)
        ctx.set_lf_quantized(*wl.lf_q)
        ctx.set_hf_meta(wl.transform_map, wl.raw_quant, wl.epf_map, wl.ytox, wl.ytob)
        for g in range(wl.coeffs.shape[0]):
            ctx.submit_group(g, wl.coeffs[g])
        ctx.slot_wait(0)
        if extra_channel:
            ctx.set_extra_channel(0, rng.integers(0, 256, size=(n, n)).astype(np.int32), 8)
        ctx.frame_run()
        ctx.sync()

    render(synth.make_vardct(n, n, mix=synth.MIX_D1, seed=1, unique_groups=24, epf_iters=2, gab=True, lf_smoothing=True),
           extra_channel=not (a.shipped_only or a.readouts))
    out = lib.DeviceArray(nbytes=px * 8)
    xyb = np.float32(XYB)

    def timed(name, fn):
        ctx.kernel_timing_reset()
        ctx.kernel_timing(True)
        for _ in range(a.steps):
            fn()
        ctx.sync()
        kt = ctx.kernel_times()
        ctx.kernel_timing(False)
        return kt[name][0] / kt[name][1]

    def shipped():
        ctx.read_rgb8(xyb, 4, out=out.ptr)

    if a.readouts:
        L, dst, pr = ctx.L, C.c_void_p(out.ptr), xyb.ctypes.data_as(C.c_void_p)

        def case(name, label, in_bytes, out_bytes, fn):
            fn()
            ctx.sync()
            print(json.dumps({"case": name, "library": LIBRARY, "image": f"{n}x{n}", "bytes": px * (in_bytes + out_bytes),
                              "ms": [timed(label, fn) for _ in range(a.reps)]}), flush=True)

        for bits, f, label in ((8, L.jxlh_frame_read_rgb8, "k_xyb_to_rgb8"), (16, L.jxlh_frame_read_rgb16, "k_xyb_to_rgb16")):
            for ch in (3, 4):
                pitch = n * ch * bits // 8
                case(f"read_rgb{bits}_x{ch}", label, 12, ch * bits // 8,
                     lambda: ctx._chk(f(ctx._ctx, pr, ch, 0, n, dst, pitch), "read-out"))
        # 4:2:0 without filters: Y at full size, two chroma channels at a quarter (6 B/px in)
        render(synth.make_vardct(n, n, mix=synth.MIX_8X8, seed=1, unique_groups=24, epf_iters=0, gab=False,
                                 lf_smoothing=False, hshift=(1, 0, 1), vshift=(1, 0, 1)))
        case("read_ycbcr420_rgb8_x3", "k_ycbcr_sub_to_rgb", 6, 3,
             lambda: ctx._chk(L.jxlh_frame_read_ycbcr_rgb8(ctx._ctx, 3, 0, n, dst, n * 3), "read-out"))
        out.free()
        ctx.close()
        return

    if a.shipped_only:
        shipped()
        ctx.sync()
        ms = [timed("k_xyb_to_rgb8", shipped) for _ in range(a.reps)]
        nbytes = px * 16
        print(json.dumps({"case": "shipped_rgba8", "image": f"{n}x{n}", "bytes": nbytes, "shipped_ms": statistics.median(ms),
                          "shipped_ms_min_max": [min(ms), max(ms)], "TBps": nbytes / statistics.median(ms) * 1e-9}), flush=True)
        return

    def copy_ms(nbytes):
        src, dst = lib.DeviceArray(nbytes=nbytes), lib.DeviceArray(nbytes=nbytes)
        for _ in range(3):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        src.free()
        dst.free()
        return ms

    colour = ctx.output_desc(lib.COLOR_XYB, "srgb", xyb)
    cases = [("rgba8_alpha", dict(channels=[0, 1, 2, 3], format=lib.SAVE_U8), 16),
             ("rgba8_filled", dict(channels=[0, 1, 2], format=lib.SAVE_U8, fill_opaque_alpha=True), 12),
             ("rgb16", dict(channels=[0, 1, 2], format=lib.SAVE_U16), 12),
             ("rgba_f16", dict(channels=[0, 1, 2, 3], format=lib.SAVE_F16), 16),
             ("gray8", dict(channels=[0], format=lib.SAVE_U8), 12)]
    for name, kw, in_bytes in cases:
        identity_ms = None
        for o in (1, 3, 6):
            tag = f"{name}_o{o}"
            if a.kernel_only and a.kernel_only != tag:
                continue
            d = lib.save_desc(orientation=o, **kw)
            bpr = n * d.pixel_bytes

            def save():
                ctx.frame_save(d, colour, out=out.ptr, bytes_per_row=bpr)
            save()
            ctx.sync()
            if a.kernel_only:
                for _ in range(5):
                    save()
                ctx.sync()
                continue
            nbytes = px * (in_bytes + d.pixel_bytes)
            with_shipped = name == "rgba8_filled" and o == 1
            k_ms, c_ms, s_ms = [], [], []
            for _ in range(a.reps):  # kernel and yardsticks alternate
                k_ms.append(timed("k_save", save))
                c_ms.append(copy_ms(nbytes // 2))
                if with_shipped:
                    s_ms.append(timed("k_xyb_to_rgb8", shipped))
            km, cm = statistics.median(k_ms), statistics.median(c_ms)
            row = {"case": tag, "image": f"{n}x{n}", "pixel_bytes": d.pixel_bytes, "bytes": nbytes, "k_save_ms": km,
                   "k_save_ms_min_max": [min(k_ms), max(k_ms)], "TBps": nbytes / km * 1e-9, "copy_ms": cm,
                   "copy_ms_min_max": [min(c_ms), max(c_ms)], "copy_TBps": nbytes / cm * 1e-9, "vs_copy": cm / km}
            if with_shipped:
                sm = statistics.median(s_ms)
                row.update({"shipped_ms": sm, "shipped_ms_min_max": [min(s_ms), max(s_ms)], "vs_shipped": sm / km})
            if o == 1:
                identity_ms = km
            elif identity_ms:
                row["vs_identity"] = identity_ms / km
            print(json.dumps(row), flush=True)
    out.free()
    ctx.close()


def merge(files):
    """the --readouts lines of several runs -> per case and library: median, min-max, TB/s; libraries in order of appearance"""
    rows, libs = {}, []
    for name in files:
        with open(name) as f:
            for line in f:
                if not line.startswith("{"):
                    continue
                r = json.loads(line)
                if r["library"] not in libs:
                    libs.append(r["library"])
                rows.setdefault(r["case"], {"bytes": r["bytes"]}).setdefault(r["library"], []).extend(r["ms"])
    for case, per in rows.items():
        row = {"case": case, "bytes": per["bytes"]}
        for lib in libs:
            ms = per.get(lib, [])
            if ms:
                med = statistics.median(ms)
                row[lib] = {"n": len(ms), "median_ms": med, "min_max_ms": [min(ms), max(ms)], "TBps": per["bytes"] / med * 1e-9}
        if len(libs) == 2 and all(lib in row for lib in libs):
            a, b = row[libs[0]], row[libs[1]]
            row["margin_ms"] = a["min_max_ms"][1] - a["min_max_ms"][0]  # the first library's own spread
            row["ok"] = b["median_ms"] <= a["median_ms"] + row["margin_ms"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
