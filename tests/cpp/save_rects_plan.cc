// The plan of the rectangle-list save (jxl_rs_amd/csrc/save_rects_plan.h) against a brute-force transcription: a
// per-pixel membership scan of the list and a per-pixel display_pixel say which bytes of the oriented image must be
// written and with which pixel; the plan's work list is walked the way the kernels walk it (bisection for the rect, the
// row form's lanes of four pixels from x0 rounded down, the tile form's tiles from the rect's corner), each pixel is
// "stored" at origin + row * pitch, and a staged plan's blocks are then copied out as the host code copies them.  The
// two images of byte tags must be equal: every pixel of the union at its place, nothing else touched.  Plus the
// refusals, the workgroup numbering, and the geometry of jxlh_changed_rects.  Host only, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../jxl_rs_amd/csrc/save_rects_plan.h"

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

// headers/image_metadata.rs:85-96
void display_pixel(int o, long x, long y, long w, long h, long* ox, long* oy) {
  switch (o) {
    case 1: *ox = x, *oy = y; break;
    case 2: *ox = w - 1 - x, *oy = y; break;
    case 3: *ox = w - 1 - x, *oy = h - 1 - y; break;
    case 4: *ox = x, *oy = h - 1 - y; break;
    case 5: *ox = y, *oy = x; break;
    case 6: *ox = h - 1 - y, *oy = x; break;
    case 7: *ox = h - 1 - y, *oy = w - 1 - x; break;
    default: *ox = y, *oy = w - 1 - x; break;
  }
}

using Rects = std::vector<jxlh_rect>;

// the image of byte tags the call must leave: tag = 1 + pixel index for every byte of a pixel of the union, else 0
std::vector<uint32_t> brute(const Rects& rects, long w, long h, int o, long pb, long bpr) {
  const long oh = o >= 5 ? w : h;
  std::vector<uint32_t> img((size_t)(oh * bpr), 0u);
  for (long y = 0; y < h; y++)
    for (long x = 0; x < w; x++) {
      bool in = false;
      for (const jxlh_rect& r : rects)  // 64-bit: x0 + w may pass 2^32 only in refused lists, but stay safe
        in |= r.w && r.h && x >= (long)r.x0 && x < (long)r.x0 + (long)r.w && y >= (long)r.y0 && y < (long)r.y0 + (long)r.h;
      if (!in) continue;
      long ox, oy;
      display_pixel(o, x, y, w, h, &ox, &oy);
      for (long b = 0; b < pb; b++) img[(size_t)(oy * bpr + ox * pb + b)] = (uint32_t)(1 + y * w + x);
    }
  return img;
}

// the kernels' walk over the work list; `mem` is what SaveLaunch::out points at
struct Walk {
  const jxlh::SaveRectsPlan& p;
  long w, h, pb;
  int o;
  std::vector<uint32_t>& mem;
  std::vector<uint8_t> seen;  // per pixel of the current rect

  void store(const jxlh::SaveRectWork& r, long x, long y) {
    CHECK(x >= (long)r.x0 && x < (long)(r.x0 + r.w) && y >= (long)r.y0 && y < (long)(r.y0 + r.h), "pixel %ld,%ld outside its rect", x, y);
    uint8_t& s = seen[(size_t)((y - r.y0) * r.w + (x - r.x0))];
    CHECK(s == 0, "pixel %ld,%ld written twice by one rect", x, y);
    s = 1;
    long ox, oy;
    display_pixel(o, x, y, w, h, &ox, &oy);
    const long at = (long)r.origin + oy * (long)r.pitch + ox * pb;
    CHECK(at >= 0 && (size_t)(at + pb) <= mem.size(), "store at %ld outside the destination (%zu)", at, mem.size());
    if (at < 0 || (size_t)(at + pb) > mem.size()) return;
    for (long b = 0; b < pb; b++) mem[(size_t)(at + b)] = (uint32_t)(1 + y * w + x);
  }
  static size_t find(const std::vector<jxlh::SaveRectWork>& work, uint32_t g) {
    size_t lo = 0, hi = work.size();
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) >> 1;
      if (work[mid].first <= g) lo = mid;
      else hi = mid;
    }
    return lo;
  }
  void run() {
    const auto& work = p.work;
    uint32_t g = 0;
    for (size_t i = 0; i < work.size(); i++) {
      const jxlh::SaveRectWork& r = work[i];
      CHECK(r.first == g, "rect %zu starts at workgroup %u, expected %u", i, r.first, g);
      CHECK(r.w > 0 && r.h > 0 && (long)r.x0 + r.w <= w && (long)r.y0 + r.h <= h, "rect %zu is not clipped", i);
      seen.assign((size_t)r.w * r.h, 0);
      const uint32_t th = o >= 5 ? jxlh::rect_tile_rows((uint32_t)pb) : jxlh::kRectRowsPerGroup;
      const uint32_t nby = (r.h + th - 1) / th;
      for (uint32_t l = 0; l < r.nbx * nby; l++, g++) {
        CHECK(find(work, g) == i, "workgroup %u does not find rect %zu", g, i);
        const uint32_t bx = l % r.nbx, by = l / r.nbx;
        if (o < 5) {  // k_save_rows_rects
          for (uint32_t wave = 0; wave < 4; wave++) {
            const uint32_t row = by * 4 + wave;
            if (row >= r.h) continue;
            for (uint32_t lane = 0; lane < 64; lane++) {
              const long x4 = (long)(r.x0 & ~3u) + (long)(bx * 64 + lane) * 4, xl = r.x0, xr = (long)r.x0 + r.w;
              if (x4 >= xr || x4 + 4 <= xl) continue;
              for (int k = 0; k < 4; k++)
                if (x4 + k >= xl && x4 + k < xr) store(r, x4 + k, (long)r.y0 + row);
            }
          }
        } else {  // k_save_tiles_rects
          const long xa = (long)r.x0 + (long)bx * 64, ya = (long)r.y0 + (long)by * th;
          const long yb = std::min<long>(ya + th, (long)r.y0 + r.h), nc = std::min<long>(64, (long)r.x0 + r.w - xa);
          CHECK(nc > 0 && yb > ya, "empty tile %u of rect %zu", l, i);
          for (long c = 0; c < nc; c++)
            for (long y = ya; y < yb; y++) store(r, xa + c, y);
        }
      }
      size_t covered = 0;
      for (uint8_t s : seen) covered += s;
      CHECK(covered == seen.size(), "rect %zu: %zu of %zu pixels written", i, covered, seen.size());
    }
    CHECK(g == p.groups, "%u workgroups walked, the plan says %u", g, p.groups);
  }
};

void one_case(const Rects& rects, long w, long h, int o, long pb, const char* what) {
  g_cases++;
  const long ow = o >= 5 ? h : w, oh = o >= 5 ? w : h;
  const long bpr = ow * pb + 5;  // padding behind every row, no multiple of four
  CHECK(jxlh::check_save_rects(rects.data(), (uint32_t)rects.size(), (uint32_t)w, (uint32_t)h) == JXLH_OK, "%s refused", what);
  const std::vector<uint32_t> want = brute(rects, w, h, o, pb, bpr);
  size_t nonempty = 0;
  for (const jxlh_rect& r : rects) nonempty += r.w && r.h;
  for (int staged = 0; staged < 2; staged++) {
    const jxlh::SaveRectsPlan p = jxlh::plan_save_rects(rects.data(), (uint32_t)rects.size(), (uint32_t)w, (uint32_t)h,
                                                        (uint32_t)o, (uint32_t)pb, staged != 0, (uint64_t)bpr);
    CHECK(p.status == JXLH_OK && p.work.size() == nonempty && p.out.size() == nonempty, "%s: %zu work items for %zu rects",
          what, p.work.size(), nonempty);
    std::vector<uint32_t> image((size_t)(oh * bpr), 0u);
    if (!staged) {
      CHECK(p.staging_bytes == 0, "%s: a device destination stages nothing", what);
      Walk{p, w, h, pb, o, image, {}}.run();
    } else {
      std::vector<uint32_t> stage((size_t)p.staging_bytes, 0u);
      Walk{p, w, h, pb, o, stage, {}}.run();
      uint64_t at = 0, bytes = 0;
      for (const jxlh::SaveRectOut& r : p.out) {  // packed one after another, each at its own dword-rounded pitch
        CHECK(r.stage_off == at && r.stage_pitch == (r.row_bytes + 3) / 4 * 4 && r.row_bytes == r.ow * (uint64_t)pb,
              "%s: staging layout", what);
        at += r.stage_pitch * r.oh;
        bytes += r.row_bytes * r.oh;
        CHECK(r.ox0 + r.ow <= (uint64_t)ow && r.oy0 + r.oh <= (uint64_t)oh, "%s: oriented rect outside the image", what);
        for (uint64_t y = 0; y < r.oh; y++)  // the 2-D copy of exactly the pixel bytes
          for (uint64_t b = 0; b < r.row_bytes; b++) {
            const uint32_t tag = stage[(size_t)(r.stage_off + y * r.stage_pitch + b)];
            CHECK(tag != 0, "%s: a staged byte was never written", what);
            image[(size_t)((r.oy0 + y) * bpr + r.ox0 * pb + b)] = tag;
          }
      }
      CHECK(at == p.staging_bytes, "%s: staging size", what);
      uint64_t rect_bytes = 0;  // the bytes that cross the bus are the (clipped) rects' bytes
      for (const jxlh::SaveRectWork& k : p.work) rect_bytes += (uint64_t)k.w * k.h * pb;
      CHECK(bytes == rect_bytes, "%s: %llu bytes copied for %llu rect bytes", what, (unsigned long long)bytes,
            (unsigned long long)rect_bytes);
    }
    if (image != want) {
      size_t bad = 0, first = 0;
      for (size_t i = want.size(); i-- > 0;)
        if (image[i] != want[i]) bad++, first = i;
      CHECK(false, "%s %ldx%ld o%d pb%ld %s: %zu bytes differ, first at %zu (got %u want %u)", what, w, h, o, pb,
            staged ? "staged" : "device", bad, first, image[first], want[first]);
    }
  }
}

uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u, s >> 8; }

void plan_cases() {
  const long sizes[][2] = {{1, 1}, {5, 3}, {1030, 9}, {70, 130}};
  const long pbs[] = {1, 2, 3, 4, 6, 8, 16};
  for (const auto& sz : sizes) {
    const uint32_t w = (uint32_t)sz[0], h = (uint32_t)sz[1];
    std::vector<std::pair<const char*, Rects>> lists;
    lists.push_back({"no rects", {}});
    lists.push_back({"empty rects only", {{0, 0, 0, 5}, {w + 7, h + 9, 0, 0}, {0, 0, 3, 0}}});  // (skipped wherever they start)
    lists.push_back({"whole image", {{0, 0, w, h}}});
    lists.push_back({"whole image, oversized", {{0, 0, 0xffffffffu, 0xffffffffu}}});
    lists.push_back({"1x1 at the far corner", {{w - 1, h - 1, 1, 1}}});
    lists.push_back({"1x1 at the origin twice", {{0, 0, 1, 1}, {0, 0, 1, 1}}});
    lists.push_back({"clipped right and bottom", {{w / 2, h / 2, w, h}}});
    if (w > 3 && h > 2) {
      lists.push_back({"odd x0, odd width", {{1, 1, 3, 1}, {3, 0, w - 3, 2}}});
      lists.push_back({"overlapping", {{0, 0, w - 1, h - 1}, {1, 1, w - 1, h - 1}, {2, 0, 1, h}}});
      lists.push_back({"duplicates and an empty one between", {{2, 1, 2, 2}, {0, 0, 0, 0}, {2, 1, 2, 2}}});
    }
    if (w > 1024) lists.push_back({"across the 1024-pixel block", {{1021, 2, 7, 5}, {255, 0, 3, 9}, {1, 8, 1029, 1}}});
    if (w >= 70 && h >= 130)
      lists.push_back({"across the tile boundaries", {{63, 63, 2, 2}, {61, 30, 7, 70}, {0, 31, 70, 2}, {5, 127, 65, 3}}});
    Rects many;
    uint32_t s = w * 31 + h;
    for (int i = 0; i < JXLH_MAX_SAVE_RECTS; i++) {
      const uint32_t x0 = rnd(s) % w, y0 = rnd(s) % h;
      many.push_back({x0, y0, i % 97 == 0 ? 0 : 1 + rnd(s) % 9, 1 + rnd(s) % 5});
    }
    lists.push_back({"4096 rects", many});
    for (const auto& l : lists)
      for (long pb : pbs)
        for (int o = 1; o <= 8; o++) {
          if (l.second.size() > 100 && !((pb == 3 || pb == 16) && (o == 2 || o == 7))) continue;  // the long list: 4 forms
          one_case(l.second, w, h, o, pb, l.first);
        }
  }
}

void refusals() {
  const jxlh_rect ok = {0, 0, 1, 1};
  std::vector<jxlh_rect> many(JXLH_MAX_SAVE_RECTS + 1, ok);
  CHECK(jxlh::check_save_rects(many.data(), JXLH_MAX_SAVE_RECTS, 8, 8) == JXLH_OK, "4096 rects are fine");
  CHECK(jxlh::check_save_rects(many.data(), JXLH_MAX_SAVE_RECTS + 1, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "4097 rects");
  CHECK(jxlh::check_save_rects(nullptr, 1, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "null list");
  CHECK(jxlh::check_save_rects(nullptr, 0, 8, 8) == JXLH_OK, "no list, no rects");
  const jxlh_rect bad[] = {{8, 0, 1, 1}, {0, 8, 1, 1}, {100, 100, 1, 1}, {1, 1, 0xffffffffu, 1}, {1, 1, 1, 0xffffffffu},
                           {7, 7, 0xfffffff9u, 1}};
  for (const jxlh_rect& r : bad) {
    const jxlh_rect list[2] = {ok, r};
    CHECK(jxlh::check_save_rects(list, 2, 8, 8) == JXLH_ERR_INVALID_ARGUMENT, "rect %u,%u %ux%u accepted", r.x0, r.y0, r.w, r.h);
  }
  const jxlh_rect fine[] = {{8, 8, 0, 1}, {9, 0, 1, 0}, {7, 7, 0xfffffff8u, 0xfffffff8u}, {0, 0, 0xffffffffu, 0xffffffffu}};
  for (const jxlh_rect& r : fine) CHECK(jxlh::check_save_rects(&r, 1, 8, 8) == JXLH_OK, "rect %u,%u %ux%u refused", r.x0, r.y0, r.w, r.h);
  // a list that would take 2^31 workgroups or more is refused, whole
  std::vector<jxlh_rect> huge(JXLH_MAX_SAVE_RECTS, jxlh_rect{0, 0, 46340, 46340});
  for (uint32_t o : {1u, 6u}) {
    const jxlh::SaveRectsPlan p = jxlh::plan_save_rects(huge.data(), JXLH_MAX_SAVE_RECTS, 46340, 46340, o, 4, false, 46340 * 4);
    CHECK(p.status == JXLH_ERR_UNSUPPORTED && p.work.empty() && p.groups == 0, "2^31 workgroups, orientation %u", o);
    const jxlh::SaveRectsPlan q = jxlh::plan_save_rects(huge.data(), 64, 46340, 46340, o, 4, false, 46340 * 4);
    CHECK(q.status == JXLH_OK && q.groups > 0 && q.groups < (1u << 31), "64 image-sized rects, orientation %u", o);
  }
}

// jxlh_changed_rects' geometry: the union of the rects is the union of the listed groups widened by the reach, per pixel
void changed_cases() {
  struct F { uint32_t w, h, gab, epf, hs, vs, reach_x, reach_y; };
  const F frames[] = {{600, 520, 0, 0, 0, 0, 0, 0}, {600, 520, 1, 0, 0, 0, 1, 1}, {600, 520, 0, 1, 0, 0, 2, 2},
                      {600, 520, 1, 2, 0, 0, 4, 4}, {264, 300, 1, 3, 0, 0, 7, 7}, {600, 520, 0, 0, 1, 1, 1, 1},
                      {600, 520, 1, 2, 1, 0, 5, 4}, {257, 1, 1, 3, 0, 0, 7, 7}};
  for (const F& f : frames) {
    jxlh_frame_params p;
    std::memset(&p, 0, sizeof(p));
    p.abi_version = JXLH_ABI_VERSION;
    p.xsize = f.w, p.ysize = f.h, p.gab = f.gab, p.epf_iters = f.epf;
    p.hshift[0] = p.hshift[2] = f.hs, p.vshift[0] = p.vshift[2] = f.vs;
    const jxlh::ChangedReach reach = jxlh::changed_reach(p);
    CHECK(reach.x == f.reach_x && reach.y == f.reach_y && reach.x <= 8 && reach.y <= 8, "reach %u,%u", reach.x, reach.y);
    const uint32_t xg = (f.w + 255) / 256, yg = (f.h + 255) / 256, ng = xg * yg;
    for (uint32_t mask = 0; mask < (1u << ng) && mask < 512; mask++) {
      std::vector<uint32_t> ids;
      for (uint32_t g = ng; g-- > 0;)  // descending, with a duplicate
        if (mask >> g & 1) ids.push_back(g), ids.push_back(g);
      std::vector<jxlh_rect> rects;
      CHECK(jxlh::plan_changed_rects(p, ids.data(), (uint32_t)ids.size(), rects) == JXLH_OK, "mask %u", mask);
      std::vector<uint8_t> want((size_t)f.w * f.h, 0), got(want);
      size_t runs = 0;
      for (uint32_t g = 0; g < ng; g++) {
        if (!(mask >> g & 1)) continue;
        runs += g % xg == 0 || !(mask >> (g - 1) & 1);
        const long gx = g % xg, gy = g / xg;
        for (long y = std::max<long>(0, gy * 256 - reach.y); y < std::min<long>(f.h, gy * 256 + 256 + reach.y); y++)
          for (long x = std::max<long>(0, gx * 256 - reach.x); x < std::min<long>(f.w, gx * 256 + 256 + reach.x); x++)
            want[(size_t)(y * f.w + x)] = 1;
      }
      CHECK(rects.size() == runs, "mask %u: %zu rects for %zu runs", mask, rects.size(), runs);
      for (size_t i = 0; i < rects.size(); i++) {
        const jxlh_rect& r = rects[i];
        CHECK(r.w && r.h && r.x0 + r.w <= f.w && r.y0 + r.h <= f.h, "rect outside the frame");
        if (i) CHECK(rects[i - 1].y0 < r.y0 || (rects[i - 1].y0 == r.y0 && rects[i - 1].x0 < r.x0), "not ascending");
        for (uint32_t y = r.y0; y < r.y0 + r.h; y++)
          for (uint32_t x = r.x0; x < r.x0 + r.w; x++) got[(size_t)y * f.w + x] = 1;
      }
      CHECK(got == want, "%ux%u mask %u: the rects' union is not the widened groups'", f.w, f.h, mask);
    }
  }
}

}  // namespace

int main() {
  plan_cases();
  refusals();
  changed_cases();
  if (g_fail) {
    std::printf("save rects plan: %d failures\n", g_fail);
    return 1;
  }
  std::printf("save rects plan: ok (%ld cases)\n", g_cases);
  return 0;
}
