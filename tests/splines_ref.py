"""CPU restatement of the reference's splines (jxl/src/features/spline.rs) for the tests: tests/cpp/splines_ref.c, compiled
here with gcc -ffp-contract=off in two builds like the oracle -- Ref(fused=True) evaluates the reference's mul_add with
fmaf (exact: glibc's, or the hardware instruction), Ref(fused=False) as a * b + c.  float32 all the way; nothing goes
through float64.

Segments are float32 [n, 8] arrays in the field order of jxlh_spline_segment: center_x, center_y, maximum_distance,
inv_sigma, sigma_over_4_times_intensity, color[3].  A quantized spline is (deltas [(dx, dy)], color_dct 3 x 32,
sigma_dct 32, (start_x, start_y))."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "splines_ref.c")
_dir = None
_libs = {}

i64, u64, i32, f32, vp = C.c_int64, C.c_uint64, C.c_int32, C.c_float, C.c_void_p


def _load(fused):
    global _dir
    if fused in _libs:
        return _libs[fused]
    if _dir is None:
        _dir = tempfile.mkdtemp(prefix="splines_ref_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
    so = os.path.join(_dir, "libsplines_ref_%s.so" % ("fused" if fused else "unfused"))
    cmd = ["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Werror",
           "-DSR_FUSED=%d" % (1 if fused else 0), _SRC, "-o", so, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(so)
    L.sr_segment_box.argtypes = [vp, i64, i64] + [C.POINTER(i64)] * 4
    L.sr_segment_box.restype = None
    L.sr_draw.argtypes = [vp, vp, vp, i64, i64, C.c_size_t, vp, i64]
    L.sr_draw.restype = None
    L.sr_idct_fast.argtypes = [vp, f32]
    L.sr_idct_fast.restype = f32
    L.sr_idct_original.argtypes = [vp, f32]
    L.sr_idct_original.restype = f32
    L.sr_dequantize.argtypes = [vp, i64, vp, vp, f32, f32, i32, f32, f32, u64, vp, vp, vp, C.POINTER(u64)]
    L.sr_dequantize.restype = C.c_int
    L.sr_catmull_rom.argtypes = [vp, i64, vp]
    L.sr_catmull_rom.restype = i64
    L.sr_equally_spaced.argtypes = [vp, i64, f32, vp]
    L.sr_equally_spaced.restype = i64
    L.sr_add_segment.argtypes = [f32, f32, f32, vp, f32, C.c_int, vp]
    L.sr_add_segment.restype = C.c_int
    L.sr_segments_from_points.argtypes = [vp, vp, vp, i64, f32, f32, C.c_int, vp]
    L.sr_segments_from_points.restype = i64
    L.sr_build.argtypes = [vp, vp, vp, vp, vp, i64, i32, f32, f32, u64, u64, C.c_int, vp, vp, vp, vp, vp]
    L.sr_build.restype = i64
    _libs[fused] = L
    return L


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return a.ctypes.data if a.size else None


class Ref:
    def __init__(self, fused=True):
        self.fused = fused
        self.L = _load(fused)

    # ---- the draw
    def segment_box(self, seg, w, h):
        """(x_lo, x_hi, y_lo, y_hi), half open, of one segment on a w x h plane"""
        s = _f(seg).reshape(8)
        v = [i64() for _ in range(4)]
        self.L.sr_segment_box(s.ctypes.data, w, h, *[C.byref(x) for x in v])
        return tuple(x.value for x in v)

    def draw(self, planes, segments, w=None):
        """the segments drawn in index order onto copies of three float32 planes [h, row]; w = image width when the
        rows are longer than the image (what lies beyond is left alone)"""
        pl = [_f(a).copy() for a in planes]
        h, row = pl[0].shape
        seg = _f(segments).reshape(-1, 8)
        self.L.sr_draw(pl[0].ctypes.data, pl[1].ctypes.data, pl[2].ctypes.data, row if w is None else w, h, row,
                       _p(seg), seg.shape[0])
        return pl

    # ---- from the bitstream's form to segments
    def idct_fast(self, coeffs, t):
        return np.float32(self.L.sr_idct_fast(_f(coeffs).ctypes.data, float(t)))

    def idct_original(self, coeffs, t):
        return np.float32(self.L.sr_idct_original(_f(coeffs).ctypes.data, float(t)))

    def dequantize(self, spline, adjustment, y_to_x, y_to_b, image_size):
        """-> (points [n + 1, 2], color_dct [3, 32], sigma_dct [32], estimated area) or None for an error"""
        deltas, color, sigma, start = spline
        d = np.ascontiguousarray(np.asarray(deltas, dtype=np.int64).reshape(-1, 2))
        c = np.ascontiguousarray(np.asarray(color, dtype=np.int32).reshape(96))
        s = np.ascontiguousarray(np.asarray(sigma, dtype=np.int32).reshape(32))
        pts = np.zeros((d.shape[0] + 1, 2), np.float32)
        cd, sd, area = np.zeros((3, 32), np.float32), np.zeros(32, np.float32), u64()
        ok = self.L.sr_dequantize(_p(d), d.shape[0], c.ctypes.data, s.ctypes.data, float(start[0]), float(start[1]),
                                  int(adjustment), float(y_to_x), float(y_to_b), int(image_size), pts.ctypes.data,
                                  cd.ctypes.data, sd.ctypes.data, C.byref(area))
        return (pts, cd, sd, area.value) if ok else None

    def catmull_rom(self, points):
        p = _f(points).reshape(-1, 2)
        n = self.L.sr_catmull_rom(_p(p), p.shape[0], None)
        out = np.zeros((n, 2), np.float32)
        self.L.sr_catmull_rom(_p(p), p.shape[0], _p(out))
        return out

    def equally_spaced(self, points, desired):
        """-> [m, 3]: x, y, multiplier"""
        p = _f(points).reshape(-1, 2)
        n = self.L.sr_equally_spaced(_p(p), p.shape[0], float(desired), None)
        out = np.zeros((n, 3), np.float32)
        self.L.sr_equally_spaced(_p(p), p.shape[0], float(desired), _p(out))
        return out

    def add_segment(self, center, intensity, color, sigma, high_precision):
        """-> segment [8] or None when add_segment filters it"""
        out = np.zeros(8, np.float32)
        ok = self.L.sr_add_segment(float(center[0]), float(center[1]), float(np.float32(intensity)), _f(color).ctypes.data,
                                   float(np.float32(sigma)), int(bool(high_precision)), out.ctypes.data)
        return out if ok else None

    def segments_from_points(self, color_dct, sigma_dct, points, length, desired, high_precision):
        cd, sd, p = _f(color_dct).reshape(96), _f(sigma_dct).reshape(32), _f(points).reshape(-1, 3)
        out = np.zeros((p.shape[0], 8), np.float32)
        n = self.L.sr_segments_from_points(cd.ctypes.data, sd.ctypes.data, _p(p), p.shape[0], float(np.float32(length)),
                                           float(desired), int(bool(high_precision)), _p(out))
        return out[:n]

    def build(self, splines, adjustment, y_to_x_lf, y_to_b_lf, xsize, ysize, high_precision=False):
        """Splines::initialize_draw_cache up to the segment list -> [n, 8], or None for one of the reference's errors"""
        area = min(int(xsize) * int(ysize), 2 ** 64 - 1)
        sizes_a = sizes_b = 1
        for sp in splines:  # sizes of the intermediate point lists
            dq = self.dequantize(sp, adjustment, y_to_x_lf, y_to_b_lf, area)
            if dq is None:
                return None
            inter = self.catmull_rom(dq[0])
            sizes_a = max(sizes_a, inter.shape[0])
            if np.all(np.isfinite(inter)):
                sizes_b = max(sizes_b, self.L.sr_equally_spaced(_p(inter), inter.shape[0], 1.0, None))
        n = len(splines)
        d = np.ascontiguousarray(np.concatenate([np.asarray(s[0], dtype=np.int64).reshape(-1, 2) for s in splines]
                                                + [np.zeros((0, 2), np.int64)]))
        npts = np.array([len(s[0]) for s in splines], dtype=np.int64)
        color = np.ascontiguousarray(np.array([np.asarray(s[1]).reshape(96) for s in splines], dtype=np.int32).reshape(-1))
        sigma = np.ascontiguousarray(np.array([np.asarray(s[2]).reshape(32) for s in splines], dtype=np.int32).reshape(-1))
        starts = _f([s[3] for s in splines]).reshape(-1)
        points = np.zeros(2 * (int(npts.sum()) + n) + 2, np.float32)
        dcts = np.zeros(128 * max(n, 1), np.float32)
        sa, sb = np.zeros(2 * sizes_a, np.float32), np.zeros(3 * sizes_b, np.float32)
        args = (_p(d), _p(npts), _p(color), _p(sigma), _p(starts), n, int(adjustment), float(y_to_x_lf), float(y_to_b_lf),
                int(xsize), int(ysize), int(bool(high_precision)), points.ctypes.data, dcts.ctypes.data, sa.ctypes.data,
                sb.ctypes.data)
        m = self.L.sr_build(*args, None)
        if m < 0:
            return None
        out = np.zeros((m, 8), np.float32)
        self.L.sr_build(*args, _p(out))
        return out


def kat_spline(q, start):
    """a QuantizedSpline of tests/golden/splines_kat.json + its starting point -> the tuple form"""
    return (q["control_points"], q["color_dct"], q["sigma_dct"], tuple(start))


# the spline of the reference's consistency test (render/stages/splines.rs:62-92): 500 x 500, default colour correlation
# (y_to_x_lf 0, y_to_b_lf 1), quantization adjustment 0, low precision
CONSISTENCY_SPLINE = (
    [(109, 105), (-130, -261), (-66, 193), (227, -52), (-170, 290)],
    [[168, 119] + [0] * 30, [9, 0, 7] + [0] * 29, [-10, 7] + [0] * 30],
    [4, 0, 0, 0, 0, 0, 0, 2] + [0] * 24,
    (9.0, 54.0),
)
CONSISTENCY_ARGS = dict(adjustment=0, y_to_x_lf=0.0, y_to_b_lf=1.0, xsize=500, ysize=500, high_precision=False)
