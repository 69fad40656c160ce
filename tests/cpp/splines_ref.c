/* CPU restatement of the reference's splines (jxl/src/features/spline.rs, util/fast_math.rs), what the tests hold the
 * library to.  Compiled by tests/splines_ref.py with gcc -ffp-contract=off, twice: -DSR_FUSED=1 evaluates the places
 * where the reference writes mul_add with fmaf (its SIMD back-ends; what the device must equal bit for bit),
 * -DSR_FUSED=0 as a * b + c (its scalar back-end).  Only the draw has such places; the path from the bitstream's form
 * to segments is scalar and unfused in the reference.  All arithmetic is float, in the reference's order. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef SR_FUSED
#define SR_FUSED 1
#endif
#if SR_FUSED
#define MULADD(a, b, c) fmaf((a), (b), (c))
#else
#define MULADD(a, b, c) ((a) * (b) + (c))
#endif

#define SR_PI 3.14159265358979323846f
#define SR_SQRT2 1.41421356237309504880f
#define SR_FRAC_1_SQRT_2 0.70710678118654752440f

/* ------------------------------------------------------------------------------------------------ the draw */

/* `v.round() as i64` of Rust: half away from zero; NaN -> 0; saturating */
static int64_t round_as_i64(float v) {
  float r = roundf(v);
  if (isnan(r)) return 0;
  if (r >= 9223372036854775808.0f) return INT64_MAX;
  if (r <= -9223372036854775808.0f) return INT64_MIN;
  return (int64_t)r;
}
/* `v.round() as usize`: negative -> 0 as well */
static uint64_t round_as_usize(float v) {
  float r = roundf(v);
  if (isnan(r) || r <= 0.0f) return 0;
  if (r >= 18446744073709551616.0f) return UINT64_MAX;
  return (uint64_t)r;
}

/* fast_erff_simd (fast_math.rs:64-77) */
static float erf_simd(float v) {
  float t = fabsf(v);
  float d1 = MULADD(t, 7.77394369e-02f, 2.05260015e-04f);
  float d2 = MULADD(d1, t, 2.32120216e-01f);
  float d3 = MULADD(d2, t, 2.77820801e-01f);
  float d4 = MULADD(d3, t, 1.0f);
  float d5 = d4 * d4;
  float inv = 1.0f / d5;
  float sq = inv * inv;
  return copysignf(1.0f - sq, v);
}

/* row range of add_segment (:690-694) and column range of draw_segment_simd (:612-622) on a w x h plane: half open,
 * empty when hi <= lo.  seg = center_x, center_y, maximum_distance, inv_sigma, sigma_over_4_times_intensity, color[3] */
void sr_segment_box(const float* seg, int64_t w, int64_t h, int64_t* x_lo, int64_t* x_hi, int64_t* y_lo, int64_t* y_hi) {
  float cx = seg[0], cy = seg[1], md = seg[2];
  int64_t y0 = round_as_i64(cy - md);
  int64_t y1 = round_as_i64(cy + md);
  uint64_t x0 = round_as_usize(cx - md);
  uint64_t x1 = round_as_usize(cx + md);
  if (y0 < 0) y0 = 0;
  /* the + 1 of a saturated bound is taken as "to the end" */
  *y_lo = y0;
  *y_hi = y1 >= h ? h : y1 + 1;
  *x_lo = x0 >= (uint64_t)w ? w : (int64_t)x0;
  *x_hi = x1 >= (uint64_t)w ? w : (int64_t)x1 + 1;
}

/* Splines::draw_segments over every row: the segments in index order (the stable sort by row keeps it per row) */
void sr_draw(float* p0, float* p1, float* p2, int64_t w, int64_t h, size_t stride, const float* segs, int64_t n) {
  float* pl[3] = {p0, p1, p2};
  for (int64_t s = 0; s < n; s++) {
    const float* g = segs + 8 * s;
    float cx = g[0], cy = g[1], inv_sigma = g[3], s4i = g[4];
    int64_t xa, xb, ya, yb;
    sr_segment_box(g, w, h, &xa, &xb, &ya, &yb);
    for (int64_t y = ya; y < yb; y++) {
      float dy = (float)y - cy;
      float dy2 = dy * dy;
      for (int64_t x = xa; x < xb; x++) {
        float dx = (float)x - cx;
        float dist = sqrtf(MULADD(dx, dx, dy2));
        float a1 = MULADD(dist, 0.5f, 0.35355338f) * inv_sigma;
        float a2 = MULADD(dist, 0.5f, -0.35355338f) * inv_sigma;
        float f = erf_simd(a1) - erf_simd(a2);
        float li = s4i * f * f;
        for (int c = 0; c < 3; c++) {
          float* q = pl[c] + (size_t)y * stride + (size_t)x;
          *q = MULADD(g[5 + c], li, *q);
        }
      }
    }
  }
}

/* ------------------------------------------------------------------------------------------------ the builder */

/* fast_cos (fast_math.rs:18-44) */
static float fast_cos(float x) {
  float pi2 = SR_PI * 2.0f;
  float pi2_inv = 0.5f / SR_PI;
  float npi2 = floorf(x * pi2_inv) * pi2;
  float xmodpi2 = x - npi2;
  float x_pi = fminf(xmodpi2, pi2 - xmodpi2);
  int above = x_pi >= SR_PI / 2.0f;
  float x_pihalf = above ? SR_PI - x_pi : x_pi;
  float xs = x_pihalf * 0.25f;
  float x2 = xs * xs;
  float x4 = x2 * x2;
  float pre = x4 * 0.06960438f + (x2 * -0.84087373f + 1.68179268f);
  float s1 = pre * pre - SR_SQRT2;
  float s2 = s1 * s1 - 1.0f;
  return above ? -s2 : s2;
}

static float dct_multiplier(int i) { return SR_PI / 32.0f * (float)i; }

/* Dct32::continuous_idct_fast over PrecomputedCosines::new(t) (:491-520): the products summed in index order (the sum
 * of an iterator of floats starts from -0.0, which leaves the first product as it is) */
float sr_idct_fast(const float* coeffs, float t) {
  float th = t + 0.5f, acc = 0.0f;
  for (int i = 0; i < 32; i++) {
    float prod = coeffs[i] * fast_cos(dct_multiplier(i) * th);
    acc = i == 0 ? prod : acc + prod;
  }
  return acc * SR_SQRT2;
}
/* the test-only original (:917-922) */
float sr_idct_original(const float* coeffs, float t) {
  float th = t + 0.5f, acc = 0.0f;
  for (int i = 0; i < 32; i++) {
    float prod = SR_SQRT2 * coeffs[i] * fast_cos(dct_multiplier(i) * th);
    acc = i == 0 ? prod : acc + prod;
  }
  return acc;
}

static uint64_t as_u64(float v) {
  if (isnan(v) || v <= 0.0f) return 0;
  if (v >= 18446744073709551616.0f) return UINT64_MAX;
  return (uint64_t)v;
}

static uint64_t area_limit(uint64_t image_size) {
  uint64_t cap = (uint64_t)1 << 42, v;
  if (image_size > UINT64_MAX / 1024) return cap;
  v = 1024 * image_size;
  if (v > UINT64_MAX - ((uint64_t)1 << 32)) return cap;
  v += (uint64_t)1 << 32;
  return v < cap ? v : cap;
}

static int in_pos_range(int64_t v) { return v >= -((int64_t)1 << 23) && v < ((int64_t)1 << 23); }

static uint64_t ceil_log2_u64(uint64_t v) { /* v > 0 */
  uint64_t fl = 0;
  while ((v >> (fl + 1)) != 0 && fl < 63) fl++;
  return (v & (v - 1)) ? fl + 1 : fl;
}

static uint64_t iabs64(int64_t v) { return v < 0 ? (uint64_t)(-v) : (uint64_t)v; }

/* QuantizedSpline::dequantize (:235-335).  deltas: npts (dx, dy) pairs; color: 96; sigma: 32.  Writes npts + 1 points
 * (x, y), the four dequantized DCTs and the estimated area.  0 = one of the reference's errors. */
int sr_dequantize(const int64_t* deltas, int64_t npts, const int32_t* color, const int32_t* sigma, float start_x,
                  float start_y, int32_t adjustment, float y_to_x, float y_to_b, uint64_t image_size, float* points,
                  float* color_dct, float* sigma_dct, uint64_t* area) {
  static const float weight_of[4] = {0.0042f, 0.075f, 0.07f, 0.3333f};
  uint64_t limit = area_limit(image_size), manhattan = 0, est[3] = {0, 0, 0}, max_color, logcolor, width = 0;
  float px = roundf(start_x), py = roundf(start_y), inv_quant, weight_limit;
  int64_t cx, cy, ddx = 0, ddy = 0;
  if (isnan(px) || isnan(py) || fabsf(px) > 2147483647.0f || fabsf(py) > 2147483647.0f) return 0; /* to_i32().unwrap() */
  cx = (int64_t)px;
  cy = (int64_t)py;
  if (!in_pos_range(cx) || !in_pos_range(cy)) return 0;
  points[0] = (float)cx;
  points[1] = (float)cy;
  for (int64_t i = 0; i < npts; i++) {
    int64_t dx = deltas[2 * i], dy = deltas[2 * i + 1];
    if (iabs64(dx) >= ((uint64_t)1 << 30) || iabs64(dy) >= ((uint64_t)1 << 30)) return 0; /* DELTA_LIMIT at read */
    ddx += dx;
    ddy += dy;
    if (!in_pos_range(ddx) || !in_pos_range(ddy)) return 0;
    manhattan += iabs64(ddx) + iabs64(ddy);
    if (manhattan > limit) return 0;
    cx += ddx;
    cy += ddy;
    if (!in_pos_range(cx) || !in_pos_range(cy)) return 0;
    points[2 * (i + 1)] = (float)cx;
    points[2 * (i + 1) + 1] = (float)cy;
  }
  if (adjustment >= 0) inv_quant = 1.0f / (1.0f + 0.125f * (float)adjustment);
  else inv_quant = 1.0f - 0.125f * (float)adjustment;
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) {
      float factor = i == 0 ? SR_FRAC_1_SQRT_2 : 1.0f;
      color_dct[32 * c + i] = (float)color[32 * c + i] * factor * weight_of[c] * inv_quant;
    }
  for (int i = 0; i < 32; i++) {
    color_dct[i] += y_to_x * color_dct[32 + i];
    color_dct[64 + i] += y_to_b * color_dct[32 + i];
  }
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) est[c] += as_u64(ceilf(inv_quant * (float)iabs64(color[32 * c + i])));
  est[0] += as_u64(ceilf(fabsf(y_to_x))) * est[1];
  est[2] += as_u64(ceilf(fabsf(y_to_b))) * est[1];
  max_color = est[0] > est[1] ? est[0] : est[1];
  if (est[2] > max_color) max_color = est[2];
  logcolor = ceil_log2_u64(1 + max_color);
  if (logcolor < 1) logcolor = 1;
  weight_limit = ceilf(sqrtf(((float)limit / (float)logcolor) / (float)(manhattan > 1 ? manhattan : 1)));
  for (int i = 0; i < 32; i++) {
    float factor = i == 0 ? SR_FRAC_1_SQRT_2 : 1.0f, wf;
    uint64_t wt;
    sigma_dct[i] = (float)sigma[i] * factor * weight_of[3] * inv_quant;
    wf = ceilf(inv_quant * (float)iabs64(sigma[i]));
    wt = as_u64(fminf(weight_limit, fmaxf(wf, 1.0f)));
    width += wt * wt * logcolor;
  }
  *area = width * manhattan;
  return 1;
}

/* draw_centripetal_catmull_rom_spline (:358-417): pts = n (x, y); returns the number of points (out may be NULL) */
int64_t sr_catmull_rom(const float* pts, int64_t n, float* out) {
  int64_t m = 0;
#define EMIT(X, Y) do { if (out) { out[2 * m] = (X); out[2 * m + 1] = (Y); } m++; } while (0)
  if (n == 0) return 0;
  if (n == 1) {
    EMIT(pts[0], pts[1]);
    return m;
  }
  /* window w: extended points w .. w + 3, where extended point 0 mirrors point 1 about point 0 and the last one
   * mirrors the last but one about the last; each with sqrt(|next - this|) */
  for (int64_t w = 0; w + 1 < n; w++) {
    float ex[5], ey[5], d[4], t[4];
    for (int k = 0; k < 5; k++) {
      int64_t j = w + k - 1; /* index into pts; -1 and n are the mirrored ones, n + 1 is the trailing (0, 0) */
      if (j < 0) {
        ex[k] = pts[0] + (pts[0] - pts[2]);
        ey[k] = pts[1] + (pts[1] - pts[3]);
      } else if (j < n) {
        ex[k] = pts[2 * j];
        ey[k] = pts[2 * j + 1];
      } else if (j == n) {
        ex[k] = pts[2 * (n - 1)] + (pts[2 * (n - 1)] - pts[2 * (n - 2)]);
        ey[k] = pts[2 * (n - 1) + 1] + (pts[2 * (n - 1) + 1] - pts[2 * (n - 2) + 1]);
      } else {
        ex[k] = 0.0f;
        ey[k] = 0.0f;
      }
    }
    for (int k = 0; k < 4; k++) d[k] = sqrtf(hypotf(ex[k + 1] - ex[k], ey[k + 1] - ey[k]));
    EMIT(ex[1], ey[1]);
    t[0] = 0.0f;
    for (int k = 0; k < 3; k++) t[k + 1] = t[k] + d[k];
    for (int i = 1; i < 16; i++) {
      float tt = d[0] + ((float)i / 16.0f) * d[1];
      float ax[3], ay[3], bx[2], by[2], f;
      for (int k = 0; k < 3; k++) {
        f = (tt - t[k]) / d[k];
        ax[k] = ex[k] + (ex[k + 1] - ex[k]) * f;
        ay[k] = ey[k] + (ey[k + 1] - ey[k]) * f;
      }
      for (int k = 0; k < 2; k++) {
        f = (tt - t[k]) / (d[k] + d[k + 1]);
        bx[k] = ax[k] + (ax[k + 1] - ax[k]) * f;
        by[k] = ay[k] + (ay[k + 1] - ay[k]) * f;
      }
      f = (tt - t[1]) / d[1];
      EMIT(bx[0] + (bx[1] - bx[0]) * f, by[0] + (by[1] - by[0]) * f);
    }
  }
  EMIT(pts[2 * (n - 1)], pts[2 * (n - 1) + 1]);
#undef EMIT
  return m;
}

/* for_each_equally_spaced_point (:419-451): out = (x, y, multiplier) each (may be NULL); returns their number */
int64_t sr_equally_spaced(const float* pts, int64_t n, float desired, float* out) {
  int64_t m = 0;
  float acc = 0.0f;
#define EMIT(X, Y, D) do { if (out) { out[3 * m] = (X); out[3 * m + 1] = (Y); out[3 * m + 2] = (D); } m++; } while (0)
  if (n == 0) return 0;
  EMIT(pts[0], pts[1], desired);
  if (n == 1) return m;
  for (int64_t i = 0; i + 1 < n; i++) {
    float x = pts[2 * i], y = pts[2 * i + 1];
    float sx = pts[2 * i + 2] - x, sy = pts[2 * i + 3] - y;
    float sl = hypotf(sx, sy);
    float inv = 1.0f / sl;
    float ux = sx * inv, uy = sy * inv;
    if (acc + sl >= desired) {
      float step = desired - acc;
      x = x + ux * step;
      y = y + uy * step;
      EMIT(x, y, desired);
      acc -= desired;
    }
    acc += sl;
    while (acc >= desired) {
      x = x + ux * desired;
      y = y + uy * desired;
      EMIT(x, y, desired);
      acc -= desired;
    }
  }
  EMIT(pts[2 * (n - 1)], pts[2 * (n - 1) + 1], acc);
#undef EMIT
  return m;
}

static uint32_t bits_of(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

/* add_segment (:658-696): 1 = a segment was written to out[8], 0 = filtered */
int sr_add_segment(float cx, float cy, float intensity, const float* color, float sigma, int high_precision, float* out) {
  float distance_exp = high_precision ? 5.0f : 3.0f, max_color, md;
  float ch[4];
  if (isinf(sigma) || sigma == 0.0f || isinf(1.0f / sigma) || isinf(intensity)) return 0;
  ch[0] = 0.01f;
  ch[1] = color[0];
  ch[2] = color[1];
  ch[3] = color[2];
  max_color = fabsf(ch[0] * intensity);
  for (int i = 1; i < 4; i++) { /* total_cmp on non-negative floats orders them like their bit patterns */
    float a = fabsf(ch[i] * intensity);
    if (bits_of(a) >= bits_of(max_color)) max_color = a;
  }
  md = sqrtf(-2.0f * sigma * sigma * (logf(0.1f) * distance_exp - logf(max_color)));
  out[0] = cx;
  out[1] = cy;
  out[2] = md;
  out[3] = 1.0f / sigma;
  out[4] = 0.25f * sigma * intensity;
  out[5] = color[0];
  out[6] = color[1];
  out[7] = color[2];
  return 1;
}

/* add_segments_from_points (:698-731): color_dct 96, sigma_dct 32 (dequantized), pts = (x, y, multiplier) each */
int64_t sr_segments_from_points(const float* color_dct, const float* sigma_dct, const float* pts, int64_t n, float length,
                                float desired, int high_precision, float* out) {
  int64_t m = 0;
  float inv_length = 1.0f / length;
  for (int64_t i = 0; i < n; i++) {
    float progress = fminf((float)i * desired * inv_length, 1.0f);
    float t = (32.0f - 1.0f) * progress;
    float color[3], sigma, seg[8];
    for (int c = 0; c < 3; c++) color[c] = sr_idct_fast(color_dct + 32 * c, t);
    sigma = sr_idct_fast(sigma_dct, t);
    if (sr_add_segment(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], color, sigma, high_precision, seg)) {
      if (out) memcpy(out + 8 * m, seg, sizeof seg);
      m++;
    }
  }
  return m;
}

/* Splines::initialize_draw_cache (:733-797) up to the segment list.  Splines packed: deltas of all splines one after
 * the other, npts[i] pairs each; color 96 and sigma 32 per spline; starts (x, y) per spline.  scratch: floats enough
 * for the intermediate points (the caller sizes it from sr_catmull_rom / sr_equally_spaced with out = NULL).
 * Returns the number of segments, -1 for one of the reference's errors. */
int64_t sr_build(const int64_t* deltas, const int64_t* npts, const int32_t* color, const int32_t* sigma,
                 const float* starts, int64_t nsplines, int32_t adjustment, float y_to_x, float y_to_b, uint64_t xsize,
                 uint64_t ysize, int high_precision, float* points, float* dcts, float* scratch_a, float* scratch_b,
                 float* out) {
  uint64_t area = xsize != 0 && ysize > UINT64_MAX / xsize ? UINT64_MAX : xsize * ysize;
  uint64_t limit = area_limit(area), total = 0;
  const int64_t* d = deltas;
  float* pt = points;
  int64_t m = 0;
  for (int64_t i = 0; i < nsplines; i++) { /* every spline is dequantized and checked before anything is drawn */
    uint64_t est;
    if (!sr_dequantize(d, npts[i], color + 96 * i, sigma + 32 * i, starts[2 * i], starts[2 * i + 1], adjustment, y_to_x,
                       y_to_b, area, pt, dcts + 128 * i, dcts + 128 * i + 96, &est))
      return -1;
    total += est;
    if (total > limit) return -1;
    for (int64_t k = 0; k < npts[i]; k++) /* validate_adjacent_point_coincidence (:107-125) */
      if (fabsf(pt[2 * k] - pt[2 * k + 2]) < 1e-3f && fabsf(pt[2 * k + 1] - pt[2 * k + 3]) < 1e-3f) return -1;
    d += 2 * npts[i];
    pt += 2 * (npts[i] + 1);
  }
  pt = points;
  for (int64_t i = 0; i < nsplines; i++) {
    int64_t ni = sr_catmull_rom(pt, npts[i] + 1, scratch_a);
    int64_t nd = sr_equally_spaced(scratch_a, ni, 1.0f, scratch_b);
    float length = (float)(nd - 2) * 1.0f + scratch_b[3 * (nd - 1) + 2];
    pt += 2 * (npts[i] + 1);
    if (length <= 0.0f) continue;
    m += sr_segments_from_points(dcts + 128 * i, dcts + 128 * i + 96, scratch_b, nd, length, 1.0f, high_precision,
                                 out ? out + 8 * m : NULL);
  }
  return m;
}
