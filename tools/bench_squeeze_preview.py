#!/usr/bin/env python3
"""Progressive previews of a squeezed image, timed: the default squeeze chain of an n x n image on three channels with
the residuals of the last K levels not arrived (K = 2 and 4), planes device resident.

  (a) jxlh_unsqueeze_chain_preview: one call;
  (b) the route without it: jxlh_unsqueeze_chain for the regular prefix, one blocking-free but single-plane
      jxlh_smooth_unsqueeze per missing level and channel (every level, as a caller without the liveness rule runs
      them), then jxlh_rct;
both from HIP events on the context's stream, alternated in one process, median of 5 x 10 with min and max, plus the
host-clock time of issuing them; and the fused last level (smooth 2-D + RCT) as a launch of its own.

  python tools/bench_squeeze_preview.py [n]          # prints one JSON line

manual_route() is also what tests/test_gpu_squeeze_preview.py compares the new call with."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def level_kinds(levels, base_w, base_h, n_planes):
    """per level: (kind, level whose output it reads, -1 = the base)"""
    from jxl_rs_amd import lib
    kinds, _ = lib.squeeze_preview_kinds(levels, base_w, base_h, n_planes=n_planes)
    return [(int(k), i - 2 if k == lib.PREVIEW_SMOOTH_2D else i - 1) for i, k in enumerate(kinds)]


class ManualRoute:
    """(b): the calls available without jxlh_unsqueeze_chain_preview, for a chain whose missing levels are a suffix.
    Intermediate planes are the caller's, allocated once."""

    def __init__(self, ctx, levels, base, base_stride, base_w, base_h, out, out_stride, rct, cvt_rne=False):
        from jxl_rs_amd import lib
        self.ctx, self.levels, self.base, self.out, self.rct = ctx, levels, base, out, rct
        self.base_geom = (base_stride, base_w, base_h)
        self.out_stride = out_stride
        self.n_planes = len(base)
        self.flag = ctx.SMOOTH_CVT_NEAREST_EVEN if cvt_rne else 0
        self.kinds = level_kinds(levels, base_w, base_h, self.n_planes)
        self.n_prefix = next((i for i, (k, _) in enumerate(self.kinds) if k != lib.PREVIEW_REGULAR), len(levels))
        assert all(k != lib.PREVIEW_REGULAR for k, _ in self.kinds[self.n_prefix:]), "missing levels must be a suffix"
        self.mid = {}   # level -> planes of that level's output (the last level's are `out`)
        for i in range(max(self.n_prefix - 1, 0), len(levels) - 1):
            _, ow, oh, _, _ = levels[i]
            self.mid[i] = [lib.DeviceArray(nbytes=ow * oh * 4, device=ctx.device) for _ in range(self.n_planes)]

    def planes_of(self, level):
        """(pointers, stride, w, h) of a level's output"""
        if level < 0:
            return [lib_addr(b) for b in self.base], *self.base_geom
        _, ow, oh, _, _ = self.levels[level]
        if level == len(self.levels) - 1:
            return [lib_addr(o) for o in self.out], self.out_stride, ow, oh
        return [d.ptr for d in self.mid[level]], ow, ow, oh

    def run(self):
        from jxl_rs_amd import lib
        ctx, n = self.ctx, len(self.levels)
        if self.n_prefix:
            dst, dstride, _, _ = self.planes_of(self.n_prefix - 1)
            ctx.unsqueeze_chain(self.levels[:self.n_prefix], self.base, *self.base_geom, dst, dstride,
                                rct=self.rct if self.n_prefix == n else None)
        for i in range(self.n_prefix, n):
            kind, src_level = self.kinds[i]
            hz, ow, oh, _, _ = self.levels[i]
            src, sstride, sw, sh = self.planes_of(src_level)
            dst, dstride, _, _ = self.planes_of(i)
            k = ctx.SMOOTH_2D if kind == lib.PREVIEW_SMOOTH_2D else ctx.SMOOTH_H if hz else ctx.SMOOTH_V
            for p in range(self.n_planes):
                ctx.smooth_unsqueeze_dev(k | self.flag, src[p], sstride, sw, sh, dst[p], dstride, ow, oh)
        if self.rct is not None and self.n_prefix < n:
            dst, dstride, ow, oh = self.planes_of(n - 1)
            assert dstride == ow, "jxlh_rct takes flat planes"
            ctx._chk(ctx.L.jxlh_rct(ctx._ctx, dst[0], dst[1], dst[2], ow * oh, *self.rct), "rct")

    def free(self):
        for planes in self.mid.values():
            for d in planes:
                d.free()


def lib_addr(a):
    from jxl_rs_amd import lib
    return lib._addr(a).value


def main():
    import jxl_rs_amd
    from jxl_rs_amd import lib, synth
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
    ctx = jxl_rs_amd.Context(0, 1)
    rng = np.random.default_rng(11)
    steps, (bw, bh) = synth.default_squeeze_steps(n, n)
    base = [lib.DeviceArray(rng.integers(0, 256, size=(bh, bw), dtype=np.int32)) for _ in range(3)]
    out = [lib.DeviceArray(nbytes=n * n * 4) for _ in range(3)]
    res = []
    for i, (hz, ow, oh) in enumerate(steps):   # the two finest levels are missing in every run: no planes for them
        rw, rh = (ow // 2, oh) if hz else (ow, oh // 2)
        res.append([lib.DeviceArray(rng.integers(-8, 9, size=(rh, rw), dtype=np.int32)) if i < len(steps) - 2 else None
                    for _ in range(3)])
    result = {"size": n, "levels": len(steps), "runs": {}}

    def timed(fn, reps):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.timer_start()
        for _ in range(reps):
            fn()
        host = (time.perf_counter() - t0) / reps
        return ctx.timer_stop() / reps, host * 1e3

    for missing in (2, 4):
        levels = [(hz, ow, oh, [d.ptr for d in r] if i < len(steps) - missing else [None] * 3, max(ow // 2 if hz else ow, 1))
                  for i, ((hz, ow, oh), r) in enumerate(zip(steps, res))]
        bp, op = [d.ptr for d in base], [d.ptr for d in out]
        manual = ManualRoute(ctx, levels, bp, bw, bw, bh, op, n, (6, 0))
        new = lambda: ctx.unsqueeze_chain_preview(levels, bp, bw, bw, bh, op, n, rct=(6, 0))
        new(), manual.run()
        a, b = [], []
        for _ in range(5):
            a.append(timed(new, 10))
            b.append(timed(manual.run, 10))
        stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        result["runs"][f"missing_{missing}"] = {
            "preview_call_ms": stat([x[0] for x in a]), "manual_route_ms": stat([x[0] for x in b]),
            "preview_call_host_ms": stat([x[1] for x in a]), "manual_route_host_ms": stat([x[1] for x in b]),
            "kinds": [int(k) for k in lib.squeeze_preview_kinds(levels, bw, bh, n_planes=3)[0]],
            "live": [int(k) for k in lib.squeeze_preview_kinds(levels, bw, bh, n_planes=3)[1]]}
        manual.free()
    # the fused last level alone: H then V both missing from an n/2 x n/2 base -> one smooth 2-D + RCT launch
    half = (n + 1) // 2
    quarter = [lib.DeviceArray(rng.integers(0, 256, size=(half, half), dtype=np.int32)) for _ in range(3)]
    two = [(True, n, half, [None] * 3, 1), (False, n, n, [None] * 3, 1)]
    qp, op = [d.ptr for d in quarter], [d.ptr for d in out]
    fused = lambda: ctx.unsqueeze_chain_preview(two, qp, half, half, half, op, n, rct=(6, 0))
    fused()
    ms = [timed(fused, 10)[0] for _ in range(5)]
    moved = 3 * 4 * (n * n + half * half)   # bytes written and read
    result["fused_last_level"] = {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                                  "bytes_per_output_sample": round(moved / (n * n), 2),
                                  "TB_per_s": round(moved / statistics.median(ms) / 1e9, 3),
                                  "ms_for_24_B_per_sample_at_8_TB_per_s": round(24.0 * n * n / 8e12 * 1e3, 4)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
