// Stand-alone check of jxl_rs_amd/csrc/splines_host.h (plain C++, no device), meant to be built with
// -fsanitize=address,undefined,float-cast-overflow: the builder on the reference's draw-cache input against segments
// computed elsewhere (read from the file argv[1] names), the bounds on not-a-number, infinite, huge and 2^23-scale
// values, the binner's invariants against a brute-force evaluation of the per-pixel rule, and the kernel's walk over
// batches and bins against the plain walk in segment order.
//   file: int64 n_splines, n_segments; per spline int64 n_points, n_points x 2 int64, 96 int32, 32 int32, 2 float;
//         then n_segments x 8 float
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "splines_host.h"

using namespace jxlh;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static jxlh_spline_segment seg(float cx, float cy, float md) {
  jxlh_spline_segment s{};
  s.center_x = cx;
  s.center_y = cy;
  s.maximum_distance = md;
  s.inv_sigma = 1.0f;
  s.sigma_over_4_times_intensity = 0.25f;
  s.color[0] = s.color[1] = s.color[2] = 1.0f;
  return s;
}

// the rule in long double, on values that are exact there: round half away from zero, saturate, clamp
static bool touches(const jxlh_spline_segment& s, long x, long y, long w, long h) {
  auto rnd = [](float v, long lo) -> long {
    if (std::isnan(v)) return lo > 0 ? lo : 0;
    const long double r = std::roundl((long double)v);
    if (r <= (long double)lo) return lo;
    if (r >= 2147483646.0L) return 2147483646L;
    return (long)r;
  };
  const long x0 = rnd(s.center_x - s.maximum_distance, 0), x1 = rnd(s.center_x + s.maximum_distance, 0) + 1;
  const long y0 = rnd(s.center_y - s.maximum_distance, 0), y1 = rnd(s.center_y + s.maximum_distance, -1) + 1;
  return x >= x0 && x < std::min(w, x1) && y >= y0 && y < std::min(h, y1);
}

static void check_builder(const char* path) {
  FILE* f = std::fopen(path, "rb");
  CHECK(f);
  int64_t hdr[2];
  CHECK(std::fread(hdr, sizeof hdr, 1, f) == 1);
  std::vector<jxlh_quantized_spline> q((size_t)hdr[0]);
  std::vector<std::vector<int64_t>> deltas((size_t)hdr[0]);
  for (size_t i = 0; i < q.size(); i++) {
    int64_t np;
    CHECK(std::fread(&np, sizeof np, 1, f) == 1);
    deltas[i].resize((size_t)np * 2);
    CHECK(np == 0 || std::fread(deltas[i].data(), 16, (size_t)np, f) == (size_t)np);
    q[i].control_points = deltas[i].data();
    q[i].n_points = (uint32_t)np;
    CHECK(std::fread(q[i].color_dct, 4, 96, f) == 96);
    CHECK(std::fread(q[i].sigma_dct, 4, 32, f) == 32);
    float st[2];
    CHECK(std::fread(st, 4, 2, f) == 2);
    q[i].start_x = st[0];
    q[i].start_y = st[1];
  }
  std::vector<jxlh_spline_segment> want((size_t)hdr[1]), got;
  CHECK(std::fread(want.data(), sizeof(jxlh_spline_segment), want.size(), f) == want.size());
  std::fclose(f);
  CHECK(spline_build_segments(q.data(), (uint32_t)q.size(), 0, 0.0f, 0.0f, 1u << 15, 1u << 15, true, got));
  CHECK(got.size() == want.size());
  CHECK(std::memcmp(got.data(), want.data(), got.size() * sizeof(jxlh_spline_segment)) == 0);
  // inputs at the edges of what the checks let through, and past them
  jxlh_quantized_spline e = q[0];
  e.start_x = std::numeric_limits<float>::quiet_NaN();
  CHECK(!spline_build_segments(&e, 1, 0, 0.0f, 1.0f, 64, 64, false, got));
  e.start_x = std::numeric_limits<float>::infinity();
  CHECK(!spline_build_segments(&e, 1, 0, 0.0f, 1.0f, 64, 64, false, got));
  e.start_x = -3e38f;
  CHECK(!spline_build_segments(&e, 1, 0, 0.0f, 1.0f, 64, 64, false, got));
  e.start_x = 8388607.0f;  // 2^23 - 1: in range, the first delta takes it out
  CHECK(!spline_build_segments(&e, 1, 0, 0.0f, 1.0f, 64, 64, false, got));
  e = q[0];
  int64_t big[2] = {INT64_MAX, INT64_MIN};
  e.control_points = big;
  e.n_points = 1;
  CHECK(!spline_build_segments(&e, 1, 0, 0.0f, 1.0f, 64, 64, false, got));
  e = q[0];
  for (int i = 0; i < 96; i++) e.color_dct[i] = i & 1 ? INT32_MIN : INT32_MAX;
  for (int i = 0; i < 32; i++) e.sigma_dct[i] = i & 1 ? INT32_MAX : INT32_MIN;
  (void)spline_build_segments(&e, 1, INT32_MIN, 1e30f, -1e30f, UINT64_MAX, UINT64_MAX, true, got);  // whatever it says
  (void)spline_build_segments(&e, 1, INT32_MAX, std::numeric_limits<float>::quiet_NaN(), 0.0f, 0, 0, false, got);
  std::printf("builder: %zu segments equal\n", want.size());
}

static void check_bounds() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float vals[] = {nan, inf, -inf, 1e30f, -1e30f, 8388608.0f, -8388608.0f, 8388607.5f, 0.5f, -0.5f, 2.5f, 0.0f,
                        2147483520.0f, 2147483648.0f, -2147483648.0f, 3.4e38f, 1e-40f};
  const int nv = (int)(sizeof vals / sizeof vals[0]);
  for (int a = 0; a < nv; a++)
    for (int b = 0; b < nv; b++)
      for (int c = 0; c < nv; c++) {
        const SplineDev d = spline_dev(seg(vals[a], vals[b], vals[c]));
        CHECK(d.x0 >= 0 && d.x1 >= 1 && d.y0 >= 0 && d.y1 >= 0);
        int tx0, tx1, ty0, ty1;
        if (spline_bin_span(d, 300, 220, &tx0, &tx1, &ty0, &ty1))
          CHECK(tx0 >= 0 && tx0 < tx1 && tx1 <= (300 + kSplineBinW - 1) / kSplineBinW && ty0 >= 0 && ty0 < ty1 &&
                ty1 <= (220 + kSplineBinH - 1) / kSplineBinH);
      }
  SplineDev d = spline_dev(seg(5.0f, 5.0f, nan));  // only pixel (0, 0)
  CHECK(d.x0 == 0 && d.x1 == 1 && d.y0 == 0 && d.y1 == 1);
  d = spline_dev(seg(-50.0f, 10.0f, 3.0f));  // wholly left: column 0
  CHECK(d.x0 == 0 && d.x1 == 1 && d.y0 == 7 && d.y1 == 14);
  d = spline_dev(seg(10.0f, -50.0f, 3.0f));  // wholly above: no row
  CHECK(d.y1 <= 0);
  d = spline_dev(seg(4.5f, 4.5f, 2.0f));  // 2.5 -> 3, 6.5 -> 7
  CHECK(d.x0 == 3 && d.x1 == 8 && d.y0 == 3 && d.y1 == 8);
  d = spline_dev(seg(1.5f, 1.5f, 2.0f));  // -0.5 -> -1 -> 0
  CHECK(d.x0 == 0 && d.x1 == 5 && d.y0 == 0 && d.y1 == 5);
  d = spline_dev(seg(8388608.0f, 8388608.0f, 100.0f));
  CHECK(d.x0 == 8388508 && d.x1 == 8388709 && d.y0 == 8388508 && d.y1 == 8388709);
  d = spline_dev(seg(1e30f, 1e30f, 1.0f));  // far outside: an empty range on any plane
  int t[4];
  CHECK(!spline_bin_span(d, 1 << 20, 1 << 20, t, t + 1, t + 2, t + 3));
  d = spline_dev(seg(0.0f, 0.0f, inf));  // everything
  CHECK(spline_bin_span(d, 300, 220, t, t + 1, t + 2, t + 3) && t[0] == 0 && t[1] == (300 + kSplineBinW - 1) / kSplineBinW &&
        t[2] == 0 && t[3] == (220 + kSplineBinH - 1) / kSplineBinH);
  std::printf("bounds: ok\n");
}

static void check_binner(int w, int h, uint64_t budget, const std::vector<jxlh_spline_segment>& segs) {
  std::vector<SplineDev> d;
  for (const auto& s : segs) d.push_back(spline_dev(s));
  const uint32_t n = (uint32_t)d.size();
  std::vector<uint32_t> first;
  spline_plan_batches(d.data(), n, w, h, budget, first);
  CHECK(first.size() >= 2 && first.front() == 0 && first.back() == n);
  // how often (segment, pixel) is reached, over all batches
  std::vector<uint8_t> seen((size_t)n * w * h, 0);
  SplineBins b;
  for (size_t k = 0; k + 1 < first.size(); k++) {
    CHECK(first[k] < first[k + 1]);
    spline_build_bins(d.data(), first[k], first[k + 1], w, h, b);
    const uint32_t* ids = b.words.data();
    const uint32_t* start = ids + b.nbins;
    const uint32_t* list = start + b.nbins + 1;
    CHECK(b.words.size() == (size_t)2 * b.nbins + 1 + start[b.nbins]);
    {  // over the budget only when a single segment of the batch has entries at all
      int with_entries = 0, t4[4];
      for (uint32_t s = first[k]; s < first[k + 1]; s++)
        with_entries += spline_bin_span(d[s], w, h, t4, t4 + 1, t4 + 2, t4 + 3) ? 1 : 0;
      CHECK(start[b.nbins] <= budget || with_entries == 1);
    }
    CHECK(b.ntx == (w + kSplineBinW - 1) / kSplineBinW && b.nty == (h + kSplineBinH - 1) / kSplineBinH);
    CHECK(b.row_first.size() == (size_t)b.nty + 1 && b.row_first[b.nty] == b.nbins);
    for (uint32_t t = 0; t < b.nbins; t++) {
      CHECK(ids[t] < (uint32_t)(b.ntx * b.nty) && (t == 0 || ids[t - 1] < ids[t]));
      CHECK(start[t] < start[t + 1]);
      const int ty = (int)(ids[t] / b.ntx), tx = (int)(ids[t] % b.ntx);
      CHECK(b.row_first[ty] <= t && t < b.row_first[ty + 1]);
      for (uint32_t e = start[t]; e < start[t + 1]; e++) {
        const uint32_t s = list[e];
        CHECK(s >= first[k] && s < first[k + 1] && (e == start[t] || list[e - 1] < s));
        bool any = false;
        for (int yy = 0; yy < kSplineBinH; yy++)
          for (int xx = 0; xx < kSplineBinW; xx++) {
            const int x = tx * kSplineBinW + xx, y = ty * kSplineBinH + yy;
            if (x >= w || y >= h) continue;
            // what the kernel tests per pixel
            if (x >= d[s].x0 && x < d[s].x1 && y >= d[s].y0 && y < d[s].y1) {
              seen[((size_t)s * h + y) * w + x]++;
              any = true;
            }
          }
        CHECK(any);  // no entry for a bin the segment does not touch
      }
    }
    for (int r = 0; r < b.nty; r++) CHECK(b.row_first[r] <= b.row_first[r + 1]);
  }
  size_t pairs = 0;
  for (uint32_t s = 0; s < n; s++)
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const int want = touches(segs[s], x, y, w, h) ? 1 : 0;
        CHECK(seen[((size_t)s * h + y) * w + x] == want);
        pairs += want;
      }
  std::printf("binner %d x %d, budget %" PRIu64 ": %zu batches, %zu pairs\n", w, h, budget, first.size() - 1, pairs);
}

// The walk the kernel makes -- batch by batch, bin by bin, a pixel's segments in list order, values kept across a bin's
// segments and stored once -- against the plain walk in segment order, with one pixel function: the same bits.
static float pixel_term(const SplineDev& d, int x, int y, int c, float px) {
  const float dy = (float)y - d.cy, dx = (float)x - d.cx;
  const float dist = std::sqrt(std::fma(dx, dx, dy * dy));
  auto erf_like = [](float v) {
    const float t = std::fabs(v);
    const float p = std::fma(std::fma(std::fma(std::fma(t, 7.77394369e-02f, 2.05260015e-04f), t, 2.32120216e-01f), t, 2.77820801e-01f), t, 1.0f);
    const float q = 1.0f / (p * p);
    return std::copysign(1.0f - q * q, v);
  };
  const float f = erf_like(std::fma(dist, 0.5f, 0.35355338f) * d.inv_sigma) - erf_like(std::fma(dist, 0.5f, -0.35355338f) * d.inv_sigma);
  return std::fma(d.color[c], (d.s4i * f) * f, px);
}

static void check_walk(int w, int h, uint64_t budget, std::vector<jxlh_spline_segment> segs) {
  for (size_t i = 0; i < segs.size(); i++) {  // signs and magnitudes that make the order show
    const float m = (i & 1 ? -1.0f : 1.0f) * std::pow(10.0f, (float)(i % 7) - 3.0f);
    segs[i].color[0] = m;
    segs[i].color[1] = -0.5f * m;
    segs[i].color[2] = 3.0f * m;
    segs[i].inv_sigma = i % 3 == 0 ? -0.3f : 0.2f;
  }
  std::vector<SplineDev> d;
  for (const auto& s : segs) d.push_back(spline_dev(s));
  const size_t npx = (size_t)w * h;
  std::vector<float> plain(3 * npx), binned(3 * npx);
  for (size_t i = 0; i < 3 * npx; i++) plain[i] = binned[i] = i % 11 == 0 ? -0.0f : 0.001f * (float)(i % 977) - 0.4f;
  for (const SplineDev& s : d)
    for (int y = std::max(0, s.y0); y < std::min(h, s.y1); y++)
      for (int x = std::max(0, s.x0); x < std::min(w, s.x1); x++)
        for (int c = 0; c < 3; c++) plain[c * npx + (size_t)y * w + x] = pixel_term(s, x, y, c, plain[c * npx + (size_t)y * w + x]);
  std::vector<uint32_t> first;
  spline_plan_batches(d.data(), (uint32_t)d.size(), w, h, budget, first);
  SplineBins b;
  for (size_t k = 0; k + 1 < first.size(); k++) {
    spline_build_bins(d.data(), first[k], first[k + 1], w, h, b);
    const uint32_t* ids = b.words.data();
    const uint32_t* start = ids + b.nbins;
    const uint32_t* list = start + b.nbins + 1;
    for (uint32_t t = 0; t < b.nbins; t++)
      for (int l = 0; l < 256; l++) {
        const int x = (int)(ids[t] % b.ntx) * kSplineBinW + l % kSplineBinW, y = (int)(ids[t] / b.ntx) * kSplineBinH + l / kSplineBinW;
        if (x >= w || y >= h) continue;
        float px[3];
        for (int c = 0; c < 3; c++) px[c] = binned[c * npx + (size_t)y * w + x];
        bool hit = false;
        for (uint32_t e = start[t]; e < start[t + 1]; e++) {
          const SplineDev& s = d[list[e]];
          if (x < s.x0 || x >= s.x1 || y < s.y0 || y >= s.y1) continue;
          for (int c = 0; c < 3; c++) px[c] = pixel_term(s, x, y, c, px[c]);
          hit = true;
        }
        if (hit)
          for (int c = 0; c < 3; c++) binned[c * npx + (size_t)y * w + x] = px[c];
      }
  }
  CHECK(std::memcmp(plain.data(), binned.data(), plain.size() * sizeof(float)) == 0);
  std::printf("walk %d x %d, budget %" PRIu64 ": %zu batches, same bits\n", w, h, budget, first.size() - 1);
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  static_assert(sizeof(jxlh_spline_segment) == 32, "SplineSegment is 32 bytes");
  check_builder(argv[1]);
  check_bounds();
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  std::vector<jxlh_spline_segment> segs = {
      seg(10.0f, 10.0f, 3.0f),   seg(63.5f, 3.5f, 2.0f),   seg(64.0f, 4.0f, 0.0f),    seg(-50.0f, 10.0f, 3.0f),
      seg(10.0f, -50.0f, 3.0f),  seg(500.0f, 10.0f, 3.0f), seg(10.0f, 500.0f, 3.0f),  seg(5.0f, 5.0f, nan),
      seg(nan, 5.0f, 2.0f),      seg(5.0f, nan, 2.0f),     seg(100.0f, 30.0f, 90.0f), seg(0.0f, 0.0f, inf),
      seg(inf, 0.0f, 4.0f),      seg(-inf, 7.0f, 4.0f),    seg(3.0f, inf, 4.0f),      seg(3.0f, -inf, 4.0f),
      seg(1e30f, 1e30f, 1e30f),  seg(-1e30f, 2.0f, 5.0f),  seg(8388608.0f, 2.0f, 5.0f), seg(129.5f, 36.5f, 1.0f),
      seg(128.0f, 36.0f, 0.4f),  seg(127.0f, 35.0f, 0.6f), seg(70.0f, 20.0f, 40.0f),  seg(69.0f, 21.0f, 40.0f),
  };
  check_binner(130, 37, kSplineDefaultBudget, segs);
  check_binner(130, 37, 8, segs);
  check_binner(130, 37, 1, segs);
  check_binner(kSplineBinW, kSplineBinH, 3, segs);
  check_binner(kSplineBinW + 1, kSplineBinH + 1, 3, segs);
  check_binner(kSplineBinW - 1, kSplineBinH - 1, 3, segs);
  check_binner(1, 1, 2, segs);
  check_walk(130, 37, kSplineDefaultBudget, segs);
  check_walk(130, 37, 8, segs);
  check_walk(kSplineBinW + 1, kSplineBinH + 1, 1, segs);
  std::printf("splines host check: ok\n");
  return 0;
}
