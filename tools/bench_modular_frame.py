"""Cost of a Modular frame on the device (k_modular_frame.hip, abi_modular_frame.hip) at 8192 x 8192 (a measurement
tool, not a test).

Workload: an 8-bit RGB frame plus an 8-bit alpha channel, the samples device-resident (set once, device to device),
without filters and again with Gaborish + epf_iters = 2.  One JSON line per stage list:
  k_intake_ms     k_modular_intake alone, from the library's event timers: median over `reps` repetitions of the mean of
                  `steps` launches, with the smallest and largest repetition
  bytes           the intake's own traffic: 8 B per sample and channel (4 read, 4 written)
  TBps            bytes / k_intake_ms
  copy_ms / copy_TBps   a hipMemcpyAsync device-to-device copy of bytes / 2 (read + written = bytes), in the same process,
                  alternated with the kernel: the yardstick
  run_ms          the whole jxlh_frame_run from the same event timers: the sum over every kernel of the run (intake,
                  filters, the alpha channel's conversion) per call, median over `reps` with min / max; run_kernels_ms
                  lists the parts
  save_ms         jxlh_frame_save of the result as RGBA8 into a device buffer, from the event timers (k_save)
  run_host_ms / save_host_ms   the same calls by the host clock around `steps` calls that end in a synchronise: these
                  include launch overhead and the gaps between the kernels
  set_host_ms     jxlh_frame_set_modular_channels of the whole frame, device to device, by the host clock (the call waits
                  for its copies)

  python tools/bench_modular_frame.py [--size 8192] [--steps 20] [--reps 5] [--kernel-only]
--kernel-only: a few runs of the unfiltered frame and nothing else, for a profiler run of its own."""
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
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import jxl_rs_amd
    from jxl_rs_amd import lib
    n = a.size
    rng = np.random.default_rng(1)
    hip = lib.DeviceArray.hip()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    ctx = jxl_rs_amd.Context(0, 1)
    chans = [lib.DeviceArray(rng.integers(0, 256, size=(n, n)).astype(np.int32)) for _ in range(3)]
    alpha = rng.integers(0, 256, size=(n, n)).astype(np.int32)
    out = lib.DeviceArray(nbytes=n * n * 4)
    desc = lib.save_desc([0, 1, 2, 3], lib.SAVE_U8)

    def copy_ms(nbytes, steps):
        src, dst = lib.DeviceArray(nbytes=nbytes), lib.DeviceArray(nbytes=nbytes)
        for _ in range(3):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        t0 = time.perf_counter()
        for _ in range(steps):
            hip.hipMemcpyAsync(dst.ptr, src.ptr, nbytes, 3, None)
        lib.DeviceArray._settle()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        src.free()
        dst.free()
        return ms

    def host_ms(call):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def set_channels():
        ctx.set_modular_channels(*[d.ptr for d in chans], 8, w=n, h=n, stride=n)

    for name, gab, epf in (("no_filters", 0, 0), ("gab_epf2", 1, 2)):
        p = ctx.default_params(n, n)
        p.gab, p.epf_iters = gab, epf
        ctx.modular_frame_begin(p)
        set_channels()
        ctx.set_extra_channel(0, alpha, 8)
        ctx.frame_run()
        ctx.frame_save(desc, out=out.ptr, bytes_per_row=n * 4)
        ctx.sync()
        if a.kernel_only:
            for _ in range(5):
                ctx.frame_run()
            ctx.sync()
            break
        nbytes = 3 * 8 * n * n
        def timed(call):
            """{kernel: ms per call} from the library's event timers over `steps` calls"""
            ctx.kernel_timing_reset()
            ctx.kernel_timing(True)
            for _ in range(a.steps):
                call()
            ctx.sync()
            kt = ctx.kernel_times()
            ctx.kernel_timing(False)
            return {k: ms / a.steps for k, (ms, _) in kt.items()}

        save = lambda: ctx.frame_save(desc, out=out.ptr, bytes_per_row=n * 4, wait=False)
        k_ms, c_ms, r_ms, s_ms, rh_ms, sh_ms, set_ms, parts = [], [], [], [], [], [], [], {}
        for _ in range(a.reps):  # kernel and yardstick alternate
            run = timed(ctx.frame_run)
            k_ms.append(run["k_modular_intake"])
            c_ms.append(copy_ms(nbytes // 2, a.steps))
            r_ms.append(sum(run.values()))
            for k, v in run.items():
                parts.setdefault(k, []).append(v)
            s_ms.append(sum(timed(save).values()))
            rh_ms.append(host_ms(ctx.frame_run))
            sh_ms.append(host_ms(save))
            set_ms.append(host_ms(set_channels))
        km, cm = statistics.median(k_ms), statistics.median(c_ms)
        print(json.dumps({
            "case": name, "frame": f"{n}x{n}", "bytes": nbytes, "k_intake_ms": km, "k_intake_ms_min_max": [min(k_ms), max(k_ms)],
            "TBps": nbytes / km * 1e-9, "copy_ms": cm, "copy_ms_min_max": [min(c_ms), max(c_ms)], "copy_TBps": nbytes / cm * 1e-9,
            "run_ms": statistics.median(r_ms), "run_ms_min_max": [min(r_ms), max(r_ms)],
            "run_kernels_ms": {k: statistics.median(v) for k, v in parts.items()},
            "save_ms": statistics.median(s_ms), "save_ms_min_max": [min(s_ms), max(s_ms)],
            "run_host_ms": statistics.median(rh_ms), "save_host_ms": statistics.median(sh_ms),
            "set_host_ms": statistics.median(set_ms),
        }), flush=True)
    for d in chans + [out]:
        d.free()
    ctx.close()


if __name__ == "__main__":
    main()
