// Host side of the splines stage, plain C++ with no device include (tests/cpp/splines_host_check.cc compiles it alone):
//  - the segment as the kernel reads it, with the four integer bounds of the reference's per-pixel rule
//    (add_segment, features/spline.rs:690-694, and draw_segment_simd, :612-622) worked out here with explicit
//    saturating conversions -- Rust's `as` saturates, a C++ float-to-int conversion out of range is undefined;
//  - the binner: consecutive segments cut into batches under an entry budget, each batch binned into the 64 x 4 px bins
//    some segment of it touches, indices ascending inside a bin (the order the reference's stable sort by row gives);
//  - the builder: QuantizedSplines -> segments, a restatement of Splines::initialize_draw_cache (:733-797), scalar,
//    unfused, sums in index order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/jxl_hip.h"

namespace jxlh {

// bin geometry: kSplineBinW x kSplineBinH = the 256 threads of a workgroup (overridable for A/B builds)
#ifndef JXLH_SPLINE_BIN_W
#define JXLH_SPLINE_BIN_W 64
#define JXLH_SPLINE_BIN_H 4
#endif
constexpr int kSplineBinW = JXLH_SPLINE_BIN_W, kSplineBinH = JXLH_SPLINE_BIN_H;
static_assert(kSplineBinW * kSplineBinH == 256 && (kSplineBinW & (kSplineBinW - 1)) == 0, "one thread per pixel of a bin");
constexpr uint32_t kSplineMaxAxis = 2147483520u;  // the largest float below 2^31: longer planes are refused
constexpr uint64_t kSplineDefaultBudget = 1ull << 24;  // bin entries per batch (64 MB of indices)

// one segment as k_splines reads it (workgroup-uniform: scalar loads).  Pixel (x, y) of a w x h plane is touched iff
// x0 <= x < min(w, x1) and y0 <= y < min(h, y1).
struct SplineDev {
  float cx, cy, inv_sigma, s4i;
  float color[3];
  int32_t x0, x1, y0, y1;
  int32_t pad;
};

// round half away from zero, then Rust's saturating `as`, held to [lo, 2^31 - 2] (planes are shorter than 2^31 on
// both axes, and the bound + 1 must fit): NaN -> 0.  A bound of 2147483520 or more becomes 2^31 - 2: planes are held
// below kSplineMaxAxis on both axes (jxlh_stage_splines refuses longer ones), where that changes nothing.
inline int32_t spline_round_sat(float v, int32_t lo) {
  const float r = std::round(v);
  if (r != r) return lo > 0 ? lo : 0;
  if (r <= (float)lo) return lo;
  if (r >= 2147483520.0f) return INT32_MAX - 1;  // (largest float below 2^31 and everything above)
  return (int32_t)r;
}

inline SplineDev spline_dev(const jxlh_spline_segment& s) {
  SplineDev d{};
  d.cx = s.center_x;
  d.cy = s.center_y;
  d.inv_sigma = s.inv_sigma;
  d.s4i = s.sigma_over_4_times_intensity;
  for (int c = 0; c < 3; c++) d.color[c] = s.color[c];
  // columns: `as usize` (negative -> 0), then + 1.  Rows: `as i64`, y0 clamped at 0, y1 = ... + 1 may be <= 0 (no
  // row).  A value beyond the integer type's range saturates; the reference's `+ 1` on it would overflow (a panic in
  // its checked builds), here it stays "every column / row from there on".
  d.x0 = spline_round_sat(s.center_x - s.maximum_distance, 0);
  d.x1 = spline_round_sat(s.center_x + s.maximum_distance, 0) + 1;
  d.y0 = spline_round_sat(s.center_y - s.maximum_distance, 0);
  d.y1 = spline_round_sat(s.center_y + s.maximum_distance, -1) + 1;
  return d;
}

// bins [tx0, tx1) x [ty0, ty1) of a w x h plane that hold a touched pixel of d; false: none
inline bool spline_bin_span(const SplineDev& d, int w, int h, int* tx0, int* tx1, int* ty0, int* ty1) {
  const int x1 = std::min(w, d.x1), y1 = std::min(h, d.y1);
  if (d.x0 >= x1 || d.y0 >= y1) return false;
  *tx0 = d.x0 / kSplineBinW;
  *tx1 = (x1 - 1) / kSplineBinW + 1;
  *ty0 = d.y0 / kSplineBinH;
  *ty1 = (y1 - 1) / kSplineBinH + 1;
  return true;
}

// first[b] .. first[b + 1]: the segments of batch b.  Batches are runs of consecutive segments, each with at most
// `budget` bin entries -- except a single segment that alone has more, which is the only one of its batch with entries.
inline void spline_plan_batches(const SplineDev* d, uint32_t n, int w, int h, uint64_t budget,
                                std::vector<uint32_t>& first) {
  first.assign(1, 0);
  uint64_t in_batch = 0;
  for (uint32_t i = 0; i < n; i++) {
    int tx0, tx1, ty0, ty1;
    const uint64_t e = spline_bin_span(d[i], w, h, &tx0, &tx1, &ty0, &ty1) ? (uint64_t)(tx1 - tx0) * (ty1 - ty0) : 0;
    if (in_batch > 0 && in_batch + e > budget) {
      first.push_back(i);
      in_batch = 0;
    }
    in_batch += e;
  }
  if (n > 0) first.push_back(n);
}

// the bins of one batch: words = bin ids (ty * ntx + tx, ascending) | starts (nbins + 1) | segment indices;
// row_first[r] = first listed bin of bin row r (nty + 1 values)
struct SplineBins {
  int ntx = 0, nty = 0;
  uint32_t nbins = 0;
  std::vector<uint32_t> words, row_first, count;
};

inline void spline_build_bins(const SplineDev* d, uint32_t s0, uint32_t s1, int w, int h, SplineBins& b) {
  b.ntx = (w + kSplineBinW - 1) / kSplineBinW;
  b.nty = (h + kSplineBinH - 1) / kSplineBinH;
  const size_t nt = (size_t)b.ntx * b.nty;
  std::vector<uint32_t>& pos = b.count;  // per bin: entries, then where its next entry goes
  pos.assign(nt, 0);
  size_t entries = 0;
  for (uint32_t i = s0; i < s1; i++) {
    int tx0, tx1, ty0, ty1;
    if (!spline_bin_span(d[i], w, h, &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty < ty1; ty++)
      for (int tx = tx0; tx < tx1; tx++) pos[(size_t)ty * b.ntx + tx]++;
    entries += (size_t)(tx1 - tx0) * (ty1 - ty0);
  }
  uint32_t nbins = 0;
  for (size_t t = 0; t < nt; t++) nbins += pos[t] != 0;
  b.nbins = nbins;
  b.words.assign((size_t)2 * nbins + 1 + entries, 0);
  uint32_t* ids = b.words.data();
  uint32_t* start = ids + nbins;
  uint32_t* list = start + nbins + 1;
  b.row_first.assign((size_t)b.nty + 1, nbins);
  uint32_t k = 0, at = 0;
  for (size_t t = 0; t < nt; t++) {
    const uint32_t c = pos[t];
    if (!c) continue;
    const int ty = (int)(t / b.ntx);
    if (b.row_first[ty] == nbins) b.row_first[ty] = k;
    ids[k] = (uint32_t)t;
    start[k] = at;
    pos[t] = at;
    at += c;
    k++;
  }
  start[nbins] = at;
  for (int r = b.nty - 1; r >= 0; r--)  // rows without a listed bin start where the next row does
    if (b.row_first[r] == nbins || b.row_first[r] > b.row_first[r + 1]) b.row_first[r] = b.row_first[r + 1];
  for (uint32_t i = s0; i < s1; i++) {
    int tx0, tx1, ty0, ty1;
    if (!spline_bin_span(d[i], w, h, &tx0, &tx1, &ty0, &ty1)) continue;
    for (int ty = ty0; ty < ty1; ty++)
      for (int tx = tx0; tx < tx1; tx++) list[pos[(size_t)ty * b.ntx + tx]++] = i;
  }
}

// ---------------------------------------------------------------- builder (features/spline.rs:107-125, :235-451,
// :491-520, :658-797; fast_cos, util/fast_math.rs:18-44)
namespace spline_build {

struct Pt {
  float x, y;
};
inline Pt operator+(Pt a, Pt b) { return {a.x + b.x, a.y + b.y}; }
inline Pt operator-(Pt a, Pt b) { return {a.x - b.x, a.y - b.y}; }
inline Pt operator*(Pt a, float s) { return {a.x * s, a.y * s}; }
inline Pt div(Pt a, float s) {
  const float inv = 1.0f / s;
  return {a.x * inv, a.y * inv};
}
inline float len(Pt a) { return hypotf(a.x, a.y); }

constexpr float kPi = 3.14159265358979323846f;
constexpr float kSqrt2 = 1.41421356237309504880f;
constexpr float kFrac1Sqrt2 = 0.70710678118654752440f;

inline float fast_cos(float x) {
  const float pi2 = kPi * 2.0f;
  const float pi2_inv = 0.5f / kPi;
  const float npi2 = floorf(x * pi2_inv) * pi2;
  const float xmodpi2 = x - npi2;
  const float x_pi = fminf(xmodpi2, pi2 - xmodpi2);
  const bool above_pihalf = x_pi >= kPi / 2.0f;
  const float x_pihalf = above_pihalf ? kPi - x_pi : x_pi;
  const float xs = x_pihalf * 0.25f;
  const float x2 = xs * xs;
  const float x4 = x2 * x2;
  const float pre = x4 * 0.06960438f + (x2 * -0.84087373f + 1.68179268f);
  const float s1 = pre * pre - kSqrt2;
  const float s2 = s1 * s1 - 1.0f;
  return above_pihalf ? -s2 : s2;
}

inline uint64_t sat_u64(float v) {  // Rust's `as u64`
  if (!(v > 0.0f)) return 0;
  if (v >= 18446744073709551616.0f) return UINT64_MAX;
  return (uint64_t)v;
}

inline uint64_t area_limit(uint64_t image_size) {
  const uint64_t lim = 1ull << 42;
  if (image_size > (lim >> 10)) return lim;  // 1024 * size alone is past the cap
  return std::min<uint64_t>(1024 * image_size + (1ull << 32), lim);
}

inline bool pos_ok(int64_t x, int64_t y) {
  const int64_t r = 1ll << 23;
  return x >= -r && x < r && y >= -r && y < r;
}

struct Spline {
  std::vector<Pt> points;
  float color_dct[3][32];
  float sigma_dct[32];
  uint64_t estimated_area = 0;
};

inline bool dequantize(const jxlh_quantized_spline& q, int32_t adjustment, float y_to_x, float y_to_b,
                       uint64_t image_size, Spline& out) {
  const uint64_t limit = area_limit(image_size);
  const float px = std::round(q.start_x), py = std::round(q.start_y);
  // (the reference converts to i32 first and fails on what does not fit)
  if (!(px >= -2147483648.0f && px < 2147483648.0f && py >= -2147483648.0f && py < 2147483648.0f)) return false;
  if (!pos_ok((int64_t)px, (int64_t)py)) return false;
  int64_t cur_x = (int64_t)px, cur_y = (int64_t)py;
  out.points.clear();
  out.points.push_back({(float)cur_x, (float)cur_y});
  int64_t ddx = 0, ddy = 0;
  uint64_t manhattan = 0;
  for (uint32_t i = 0; i < q.n_points; i++) {
    const int64_t dx = q.control_points[2 * (size_t)i], dy = q.control_points[2 * (size_t)i + 1];
    const int64_t lim = 1ll << 30;  // QuantizedSpline::read's DELTA_LIMIT
    if (dx <= -lim || dx >= lim || dy <= -lim || dy >= lim) return false;
    ddx += dx;
    ddy += dy;
    if (!pos_ok(ddx, ddy)) return false;
    manhattan += (uint64_t)(ddx < 0 ? -ddx : ddx) + (uint64_t)(ddy < 0 ? -ddy : ddy);
    if (manhattan > limit) return false;
    cur_x += ddx;
    cur_y += ddy;
    if (!pos_ok(cur_x, cur_y)) return false;
    out.points.push_back({(float)cur_x, (float)cur_y});
  }
  const float inv_quant = adjustment >= 0 ? 1.0f / (1.0f + 0.125f * (float)adjustment) : 1.0f - 0.125f * (float)adjustment;
  static const float kWeight[4] = {0.0042f, 0.075f, 0.07f, 0.3333f};
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) {
      const float f = i == 0 ? kFrac1Sqrt2 : 1.0f;
      out.color_dct[c][i] = (float)q.color_dct[32 * c + i] * f * kWeight[c] * inv_quant;
    }
  for (int i = 0; i < 32; i++) {
    out.color_dct[0][i] += y_to_x * out.color_dct[1][i];
    out.color_dct[2][i] += y_to_b * out.color_dct[1][i];
  }
  uint64_t color[3] = {0, 0, 0};
  for (int c = 0; c < 3; c++)
    for (int i = 0; i < 32; i++) {
      const int64_t v = q.color_dct[32 * c + i];
      color[c] += sat_u64(ceilf(inv_quant * (float)(v < 0 ? -v : v)));
    }
  color[0] += sat_u64(ceilf(fabsf(y_to_x))) * color[1];
  color[2] += sat_u64(ceilf(fabsf(y_to_b))) * color[1];
  const uint64_t max_color = std::max(color[0], std::max(color[1], color[2]));
  uint64_t logcolor = 0;  // ceil_log2(1 + max_color), at least 1
  {
    const uint64_t v = 1 + max_color;
    while (logcolor < 63 && (1ull << logcolor) < v) logcolor++;
    if (logcolor < 1) logcolor = 1;
  }
  const float weight_limit =
      ceilf(sqrtf(((float)limit / (float)logcolor) / (float)std::max<uint64_t>(manhattan, 1)));
  uint64_t width_estimate = 0;
  for (int i = 0; i < 32; i++) {
    const float f = i == 0 ? kFrac1Sqrt2 : 1.0f;
    out.sigma_dct[i] = (float)q.sigma_dct[i] * f * kWeight[3] * inv_quant;
    const int64_t v = q.sigma_dct[i];
    const float weight_f = ceilf(inv_quant * (float)(v < 0 ? -v : v));
    const uint64_t weight = sat_u64(fminf(weight_limit, fmaxf(weight_f, 1.0f)));
    width_estimate += weight * weight * logcolor;
  }
  out.estimated_area = width_estimate * manhattan;
  return true;
}

inline void catmull_rom(const std::vector<Pt>& pts, std::vector<Pt>& out) {
  out.clear();
  const size_t n = pts.size();
  if (n == 0) return;
  if (n == 1) {
    out.push_back(pts[0]);
    return;
  }
  // the points with one prepended and one appended, each with the square root of the distance to the next one (the
  // last one's is never read)
  std::vector<Pt> e(n + 2);
  e[0] = pts[0] + (pts[0] - pts[1]);
  for (size_t i = 0; i < n; i++) e[i + 1] = pts[i];
  e[n + 1] = pts[n - 1] + (pts[n - 1] - pts[n - 2]);
  std::vector<float> dl(n + 2, 0.0f);
  for (size_t i = 0; i + 1 < n + 2; i++) dl[i] = sqrtf(len(e[i + 1] - e[i]));
  for (size_t w0 = 0; w0 + 3 < n + 2; w0++) {
    const Pt* p = &e[w0];
    const float* d = &dl[w0];
    out.push_back(p[1]);
    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; k++) t[k + 1] = t[k] + d[k];
    for (int i = 1; i < 16; i++) {
      const float tt = d[0] + ((float)i / 16.0f) * d[1];
      Pt a[3], b[2];
      for (int k = 0; k < 3; k++) a[k] = p[k] + (p[k + 1] - p[k]) * ((tt - t[k]) / d[k]);
      for (int k = 0; k < 2; k++) b[k] = a[k] + (a[k + 1] - a[k]) * ((tt - t[k]) / (d[k] + d[k + 1]));
      out.push_back(b[0] + (b[1] - b[0]) * ((tt - t[1]) / d[1]));
    }
  }
  out.push_back(pts[n - 1]);
}

struct Drawn {
  Pt p;
  float mult;
};

inline void equally_spaced(const std::vector<Pt>& pts, float desired, std::vector<Drawn>& out) {
  out.clear();
  if (pts.empty()) return;
  float acc = 0.0f;
  out.push_back({pts[0], desired});
  if (pts.size() == 1) return;
  for (size_t i = 0; i + 1 < pts.size(); i++) {
    Pt cur = pts[i];
    const Pt seg = pts[i + 1] - cur;
    const float seg_len = len(seg);
    const Pt unit = div(seg, seg_len);
    if (acc + seg_len >= desired) {
      cur = cur + unit * (desired - acc);
      out.push_back({cur, desired});
      acc -= desired;
    }
    acc += seg_len;
    while (acc >= desired) {
      cur = cur + unit * desired;
      out.push_back({cur, desired});
      acc -= desired;
    }
  }
  out.push_back({pts.back(), acc});
}

inline uint32_t fbits(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  return u;
}

// add_segment (:658-696): false = filtered out
inline bool make_segment(Pt center, float intensity, const float color[3], float sigma, bool high_precision,
                         jxlh_spline_segment* s) {
  if (std::isinf(sigma) || sigma == 0.0f || std::isinf(1.0f / sigma) || std::isinf(intensity)) return false;
  const float distance_exp = high_precision ? 5.0f : 3.0f;
  const float chans[4] = {0.01f, color[0], color[1], color[2]};
  float max_color = 0.0f;
  for (int i = 0; i < 4; i++) {  // max by total_cmp of absolute values: their bit patterns as unsigned
    const float a = fabsf(chans[i] * intensity);
    if (i == 0 || fbits(a) >= fbits(max_color)) max_color = a;
  }
  const float md = sqrtf(-2.0f * sigma * sigma * (logf(0.1f) * distance_exp - logf(max_color)));
  s->center_x = center.x;
  s->center_y = center.y;
  s->maximum_distance = md;
  s->inv_sigma = 1.0f / sigma;
  s->sigma_over_4_times_intensity = 0.25f * sigma * intensity;
  for (int c = 0; c < 3; c++) s->color[c] = color[c];
  return true;
}

// the 32 cosines of PrecomputedCosines::new(t), then continuous_idct_fast: products summed in index order (Rust's
// float Sum starts from -0.0, so the first product comes through unchanged)
inline void cosines(float t, float out[32]) {
  const float th = t + 0.5f;
  for (int i = 0; i < 32; i++) out[i] = fast_cos((kPi / 32.0f * (float)i) * th);
}
inline float idct(const float coeffs[32], const float cs[32]) {
  float acc = coeffs[0] * cs[0];
  for (int i = 1; i < 32; i++) acc = acc + coeffs[i] * cs[i];
  return acc * kSqrt2;
}

inline void segments_from_points(const Spline& sp, const std::vector<Drawn>& pts, float length, float desired,
                                 bool high_precision, std::vector<jxlh_spline_segment>& out) {
  const float inv_length = 1.0f / length;
  for (size_t i = 0; i < pts.size(); i++) {
    const float progress = fminf((float)i * desired * inv_length, 1.0f);
    const float t = (32.0f - 1.0f) * progress;
    float cs[32], color[3];
    cosines(t, cs);
    for (int c = 0; c < 3; c++) color[c] = idct(sp.color_dct[c], cs);
    const float sigma = idct(sp.sigma_dct, cs);
    jxlh_spline_segment s;
    if (make_segment(pts[i].p, pts[i].mult, color, sigma, high_precision, &s)) out.push_back(s);
  }
}

}  // namespace spline_build

// Splines::initialize_draw_cache up to the segment list; false = one of the reference's errors
inline bool spline_build_segments(const jxlh_quantized_spline* splines, uint32_t n, int32_t quantization_adjustment,
                                  float y_to_x_lf, float y_to_b_lf, uint64_t image_xsize, uint64_t image_ysize,
                                  bool high_precision, std::vector<jxlh_spline_segment>& out) {
  using namespace spline_build;
  out.clear();
  uint64_t image_area = image_xsize * image_ysize;
  if (image_xsize != 0 && image_area / image_xsize != image_ysize) image_area = UINT64_MAX;  // saturating_mul
  const uint64_t limit = area_limit(image_area);
  std::vector<Spline> deq(n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (splines[i].n_points > 0 && !splines[i].control_points) return false;
    if (!dequantize(splines[i], quantization_adjustment, y_to_x_lf, y_to_b_lf, image_area, deq[i])) return false;
    total += deq[i].estimated_area;
    if (total > limit) return false;
    const std::vector<Pt>& p = deq[i].points;
    for (size_t k = 0; k + 1 < p.size(); k++)  // adjacent control points that coincide (Point's ==, 1e-3)
      if (fabsf(p[k].x - p[k + 1].x) < 1e-3f && fabsf(p[k].y - p[k + 1].y) < 1e-3f) return false;
  }
  std::vector<Pt> inter;
  std::vector<Drawn> pts;
  for (uint32_t i = 0; i < n; i++) {
    catmull_rom(deq[i].points, inter);
    equally_spaced(inter, 1.0f, pts);
    const float length = (float)((ptrdiff_t)pts.size() - 2) * 1.0f + pts.back().mult;
    if (length <= 0.0f) continue;
    segments_from_points(deq[i], pts, length, 1.0f, high_precision, out);
  }
  return true;
}

}  // namespace jxlh
