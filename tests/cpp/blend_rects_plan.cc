// The plan of the rectangle-list blend (jxl_rs_amd/csrc/blend_rects_plan.h) against a per-pixel transcription, over
// random and hand-picked lists: the work list is walked the way k_blend_rects walks it (bisection for the rect, lanes of
// four pixels from x0 rounded down, a wave per row) and every pixel a lane would store is marked; the marks must be
// exactly the union of the rects -- every pixel of the union belongs to a lane of some piece, nothing outside a rect is
// ever stored, no piece lies wholly outside its rect, `first` ascends, the group count is the walk's.  Plus the
// refusals (the list checks, 2^31 workgroups) and the frame-to-image mapping of jxlh_blend_image_rects against a
// per-pixel restatement over negative and large origins.  Host only, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../jxl_rs_amd/csrc/blend_rects_plan.h"

namespace {

int g_fail = 0;
long g_cases = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (g_fail++ < 20) {                     \
        std::printf("FAIL %s: ", #c);          \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

using Rects = std::vector<jxlh_rect>;

uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u, s >> 8; }

size_t find(const std::vector<jxlh::BlendRectWork>& work, uint32_t g) {
  size_t lo = 0, hi = work.size();
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (work[mid].first <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

void one_case(const Rects& rects, long w, long h, const char* what) {
  g_cases++;
  CHECK(jxlh::check_blend_rects(rects.data(), (uint32_t)rects.size(), (uint32_t)w, (uint32_t)h) == JXLH_OK, "%s refused", what);
  // the union, per pixel
  std::vector<uint8_t> want((size_t)(w * h), 0), got(want);
  size_t nonempty = 0;
  for (const jxlh_rect& r : rects) {
    if (!r.w || !r.h) continue;
    nonempty++;
    for (long y = r.y0; y < std::min<long>(h, (long)r.y0 + (long)r.h); y++)
      for (long x = r.x0; x < std::min<long>(w, (long)r.x0 + (long)r.w); x++) want[(size_t)(y * w + x)] = 1;
  }
  const jxlh::BlendRectsPlan p = jxlh::plan_blend_rects(rects.data(), (uint32_t)rects.size(), (uint32_t)w, (uint32_t)h);
  CHECK(p.status == JXLH_OK && p.work.size() == nonempty, "%s: %zu work items for %zu rects", what, p.work.size(), nonempty);
  uint32_t g = 0;
  size_t k = 0;
  for (const jxlh_rect& r : rects) {  // list order is kept, the clip is the image's
    if (!r.w || !r.h || k >= p.work.size()) continue;
    const jxlh::BlendRectWork& q = p.work[k++];
    CHECK(q.x0 == r.x0 && q.y0 == r.y0 && q.w == std::min<uint64_t>(r.w, w - r.x0) && q.h == std::min<uint64_t>(r.h, h - r.y0),
          "%s: work item %zu is not its rect, clipped", what, k - 1);
  }
  for (size_t i = 0; i < p.work.size(); i++) {
    const jxlh::BlendRectWork& r = p.work[i];
    CHECK(r.first == g, "%s: rect %zu starts at workgroup %u, expected %u", what, i, r.first, g);
    if (i) CHECK(p.work[i - 1].first < r.first, "%s: first is not ascending at %zu", what, i);
    CHECK(r.w > 0 && r.h > 0 && (long)r.x0 + r.w <= w && (long)r.y0 + r.h <= h, "%s: rect %zu is not clipped", what, i);
    std::vector<uint8_t> seen((size_t)r.w * r.h, 0);
    const uint32_t nby = (r.h + jxlh::kBlendRectRows - 1) / jxlh::kBlendRectRows;
    for (uint32_t l = 0; l < r.nbx * nby; l++, g++) {
      CHECK(find(p.work, g) == i, "%s: workgroup %u does not find rect %zu", what, g, i);
      const uint32_t bx = l % r.nbx, by = l / r.nbx;
      size_t stored = 0;
      for (uint32_t wave = 0; wave < jxlh::kBlendRectRows; wave++) {
        const uint32_t row = by * jxlh::kBlendRectRows + wave;
        if (row >= r.h) continue;
        for (uint32_t lane = 0; lane < 64; lane++) {
          const long x4 = (long)(r.x0 & ~3u) + (long)(bx * 64 + lane) * 4, xl = r.x0, xr = (long)r.x0 + r.w;
          CHECK(x4 % 4 == 0, "a lane's x is 16-byte aligned");
          if (x4 >= xr || x4 + 4 <= xl) continue;
          for (int j = 0; j < 4; j++) {
            if (x4 + j < xl || x4 + j >= xr) continue;  // an edge lane stores singly, only inside
            const long x = x4 + j, y = (long)r.y0 + row;
            uint8_t& s = seen[(size_t)((y - r.y0) * r.w + (x - r.x0))];
            CHECK(s == 0, "%s: pixel %ld,%ld stored twice by one rect", what, x, y);
            s = 1;
            got[(size_t)(y * w + x)] = 1;
            stored++;
          }
        }
      }
      CHECK(stored > 0, "%s: piece %u of rect %zu lies wholly outside it", what, l, i);
    }
    size_t covered = 0;
    for (uint8_t s : seen) covered += s;
    CHECK(covered == seen.size(), "%s: rect %zu: %zu of %zu pixels stored", what, i, covered, seen.size());
  }
  CHECK(g == p.groups, "%s: %u workgroups walked, the plan says %u", what, g, p.groups);
  CHECK(got == want, "%s %ldx%ld: the stored pixels are not the union", what, w, h);
}

void plan_cases() {
  const long sizes[][2] = {{1, 1}, {5, 3}, {517, 11}, {1030, 9}, {70, 130}};
  for (const auto& sz : sizes) {
    const uint32_t w = (uint32_t)sz[0], h = (uint32_t)sz[1];
    one_case({}, w, h, "no rects");
    one_case({{0, 0, 0, 5}, {w + 7, h + 9, 0, 0}, {0, 0, 3, 0}}, w, h, "empty rects only");
    one_case({{0, 0, w, h}}, w, h, "whole image");
    one_case({{0, 0, 0xffffffffu, 0xffffffffu}}, w, h, "whole image, oversized");
    one_case({{w - 1, h - 1, 1, 1}}, w, h, "1x1 at the far corner");
    one_case({{0, 0, 1, 1}, {0, 0, 1, 1}}, w, h, "1x1 at the origin twice");
    one_case({{w / 2, h / 2, w, h}}, w, h, "clipped right and bottom");
    if (w > 3 && h > 2) {
      one_case({{1, 1, 3, 1}, {3, 0, w - 3, 2}}, w, h, "odd x0, odd width");
      one_case({{0, 0, w - 1, h - 1}, {1, 1, w - 1, h - 1}, {2, 0, 1, h}}, w, h, "overlapping");
      one_case({{3, 1, 2, 2}, {0, 0, 0, 0}, {3, 1, 2, 2}}, w, h, "duplicates and an empty one between");
    }
    if (w > 512) one_case({{253, 2, 7, 6}, {255, 0, 259, 9}, {1, 8, 516, 1}}, w, h, "across the piece seams");
    uint32_t s = w * 31 + h;
    for (int rep = 0; rep < 40; rep++) {  // random lists of 1 .. 24 rects
      Rects list;
      const uint32_t n = 1 + rnd(s) % 24;
      for (uint32_t i = 0; i < n; i++) {
        const uint32_t x0 = rnd(s) % w, y0 = rnd(s) % h;
        list.push_back({x0, y0, rnd(s) % 11 == 0 ? 0 : 1 + rnd(s) % (rep % 2 ? 9 : 2 * w), 1 + rnd(s) % (rep % 3 ? 5 : 2 * h)});
      }
      one_case(list, w, h, "random");
    }
    Rects many;
    for (int i = 0; i < JXLH_MAX_SAVE_RECTS; i++) {
      const uint32_t x0 = rnd(s) % w, y0 = rnd(s) % h;
      many.push_back({x0, y0, i % 97 == 0 ? 0 : 1 + rnd(s) % 9, 1 + rnd(s) % 5});
    }
    one_case(many, w, h, "4096 rects");
  }
}

void refusals() {
  const jxlh_rect ok = {0, 0, 1, 1};
  std::vector<jxlh_rect> many(JXLH_MAX_SAVE_RECTS + 1, ok);
  CHECK(jxlh::check_blend_rects(many.data(), JXLH_MAX_SAVE_RECTS, 8, 8) == JXLH_OK, "4096 rects are fine");
  CHECK(jxlh::check_blend_rects(many.data(), JXLH_MAX_SAVE_RECTS + 1, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "4097 rects");
  CHECK(jxlh::check_blend_rects(nullptr, 1, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "null list");
  CHECK(jxlh::check_blend_rects(nullptr, 0, 8, 8) == JXLH_OK, "no list, no rects");
  const jxlh_rect bad[] = {{8, 0, 1, 1}, {0, 8, 1, 1}, {100, 100, 1, 1}, {1, 1, 0xffffffffu, 1}, {1, 1, 1, 0xffffffffu},
                           {7, 7, 0xfffffff9u, 1}};
  for (const jxlh_rect& r : bad) {
    const jxlh_rect list[2] = {ok, r};
    CHECK(jxlh::check_blend_rects(list, 2, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "rect %u,%u %ux%u accepted", r.x0, r.y0, r.w, r.h);
  }
  const jxlh_rect fine[] = {{8, 8, 0, 1}, {9, 0, 1, 0}, {7, 7, 0xfffffff8u, 0xfffffff8u}, {0, 0, 0xffffffffu, 0xffffffffu}};
  for (const jxlh_rect& r : fine) CHECK(jxlh::check_blend_rects(&r, 1, 8, 8) == JXLH_OK, "rect %u,%u %ux%u refused", r.x0, r.y0, r.w, r.h);
  // the group count of image-sized rects: ceil(46340 / 256) * ceil(46340 / 4) each; 4096 of them pass 2^31, 64 do not
  std::vector<jxlh_rect> huge(JXLH_MAX_SAVE_RECTS, jxlh_rect{0, 0, 46340, 46340});
  const jxlh::BlendRectsPlan p = jxlh::plan_blend_rects(huge.data(), JXLH_MAX_SAVE_RECTS, 46340, 46340);
  CHECK(p.status == JXLH_ERR_UNSUPPORTED && p.work.empty() && p.groups == 0, "2^31 workgroups");
  const jxlh::BlendRectsPlan q = jxlh::plan_blend_rects(huge.data(), 64, 46340, 46340);
  CHECK(q.status == JXLH_OK && q.groups == 64u * 182u * 11585u, "64 image-sized rects: %u groups", q.groups);
  // exactly at the limit: 2^31 - 1 groups pass, 2^31 do not (rects of 1 x 4 * 2^20 rows: 2^20 groups each)
  std::vector<jxlh_rect> cols(2048, jxlh_rect{0, 0, 1, 1u << 22});
  const jxlh::BlendRectsPlan at = jxlh::plan_blend_rects(cols.data(), 2048, 4, 1u << 22);
  CHECK(at.status == JXLH_ERR_UNSUPPORTED, "2^31 workgroups exactly");
  cols.back().h -= 4;
  const jxlh::BlendRectsPlan below = jxlh::plan_blend_rects(cols.data(), 2048, 4, 1u << 22);
  CHECK(below.status == JXLH_OK && below.groups == 0x7fffffffu, "2^31 - 1 workgroups: %u", below.groups);
}

// jxlh_blend_image_rects' mapping: per pixel of the image, "in some output rect" == "the pixel's frame coordinate lies
// in some input rect and in the frame"; the outputs are non-empty, inside the image, and in list order
void mapping_cases() {
  const uint32_t frames[][2] = {{300, 260}, {9, 9}};
  const uint32_t images[][2] = {{1, 1}, {40, 28}, {517, 11}};
  const int32_t big = 1 << 30, min32 = INT32_MIN, max32 = INT32_MAX;
  uint32_t s = 12345;
  for (const auto& fr : frames)
    for (const auto& im : images) {
      const long fw = fr[0], fh = fr[1], iw = im[0], ih = im[1];
      std::vector<int32_t> xs = {min32, -big - 1, -big, -(int32_t)fw - 1, -(int32_t)fw, -(int32_t)fw + 1, -1, 0, 1, (int32_t)iw - 1,
                                 (int32_t)iw, (int32_t)iw + 1, (int32_t)iw - (int32_t)fw, big, big + 1, max32};
      std::vector<int32_t> ys = {min32, -big, -(int32_t)fh, -(int32_t)fh + 1, -2, 0, 3, (int32_t)ih - 1, (int32_t)ih, big, max32};
      for (int32_t x0 : xs)
        for (int32_t y0 : ys) {
          g_cases++;
          Rects in;
          in.push_back({0, 0, (uint32_t)fw, (uint32_t)fh});
          in.push_back({0, 0, 0xffffffffu, 0xffffffffu});
          in.push_back({(uint32_t)fw, 0, 5, 5});       // outside the frame
          in.push_back({(uint32_t)fw - 1, (uint32_t)fh - 1, 0xffffffffu, 0xffffffffu});
          in.push_back({0xfffffff0u, 0xfffffff0u, 0xffu, 0xffu});
          for (int i = 0; i < 6; i++)
            in.push_back({rnd(s) % (uint32_t)(fw + 3), rnd(s) % (uint32_t)(fh + 3), rnd(s) % 5 == 0 ? 0 : 1 + rnd(s) % (uint32_t)fw,
                          rnd(s) % (uint32_t)(fh + 2)});
          std::vector<jxlh_rect> out;
          jxlh::map_blend_image_rects(x0, y0, (uint32_t)iw, (uint32_t)ih, (uint32_t)fw, (uint32_t)fh, in.data(), (uint32_t)in.size(), out);
          const long long ox = std::min<long long>(std::max<long long>(x0, -(long long)big), big);
          const long long oy = std::min<long long>(std::max<long long>(y0, -(long long)big), big);
          // per input rect, the expected output (or none), by scanning the image's pixels
          size_t k = 0;
          for (const jxlh_rect& r : in) {
            long long lo_x = -1, hi_x = -1, lo_y = -1, hi_y = -1;
            for (long long x = 0; x < iw; x++) {
              const long long f = x - ox;
              if (f >= 0 && f < fw && f >= (long long)r.x0 && f < (long long)r.x0 + (long long)r.w) {
                if (lo_x < 0) lo_x = x;
                hi_x = x + 1;
              }
            }
            for (long long y = 0; y < ih; y++) {
              const long long f = y - oy;
              if (f >= 0 && f < fh && f >= (long long)r.y0 && f < (long long)r.y0 + (long long)r.h) {
                if (lo_y < 0) lo_y = y;
                hi_y = y + 1;
              }
            }
            if (lo_x < 0 || lo_y < 0) continue;  // dropped
            CHECK(k < out.size(), "origin %d,%d: a rect is missing", x0, y0);
            if (k >= out.size()) break;
            const jxlh_rect& o = out[k++];
            CHECK(o.x0 == lo_x && o.y0 == lo_y && o.w == hi_x - lo_x && o.h == hi_y - lo_y,
                  "frame %ldx%ld image %ldx%ld origin %d,%d: got %u,%u %ux%u want %lld,%lld %lldx%lld", fw, fh, iw, ih, x0, y0,
                  o.x0, o.y0, o.w, o.h, lo_x, lo_y, hi_x - lo_x, hi_y - lo_y);
          }
          CHECK(k == out.size(), "origin %d,%d: %zu rects, expected %zu", x0, y0, out.size(), k);
          CHECK(jxlh::check_blend_rects(out.data(), (uint32_t)out.size(), (uint32_t)iw, (uint32_t)ih) == JXLH_OK,
                "the mapped list is one jxlh_frame_blend_rects takes");
        }
    }
}

}  // namespace

int main() {
  plan_cases();
  refusals();
  mapping_cases();
  if (g_fail) {
    std::printf("blend rects plan: %d failures\n", g_fail);
    return 1;
  }
  std::printf("blend rects plan: ok (%ld cases)\n", g_cases);
  return 0;
}
