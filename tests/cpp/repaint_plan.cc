// The repaint planner (jxl_rs_amd/csrc/repaint_plan.h) over a sweep of frames: sizes around the 256 grid, every stage
// list, VarDCT / Modular, upsampling 1 / 2 / 4 / 8, noise, draws_in_place, chroma subsampling, rendered or not, random
// group lists.  Held to plan_rerender and plan_run (which it is built on) and to statements of its own rules made here
// per row and per pixel.  Host only, no device.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../jxl_rs_amd/csrc/repaint_plan.h"

using namespace jxlh;

namespace {

int failures = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      if (failures++ < 20) {                    \
        std::printf("FAIL %s: ", #cond);        \
        std::printf(__VA_ARGS__);               \
        std::printf("\n");                      \
      }                                         \
    }                                           \
  } while (0)

bool same_bands(const std::vector<RowBand>& a, const std::vector<RowBand>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].y_lo != b[i].y_lo || a[i].y_hi != b[i].y_hi || a[i].whole_frame != b[i].whole_frame) return false;
  return true;
}

// the rows of the result a plan's ranges cover, as a bitmap
std::vector<char> rows_of(const std::vector<RowRange>& r, int n) {
  std::vector<char> m((size_t)n, 0);
  for (const RowRange& x : r)
    for (int y = x.lo; y < x.hi; y++) m[(size_t)y] = 1;
  return m;
}

void check_ranges(const std::vector<RowRange>& r, int limit, const char* what) {
  for (size_t i = 0; i < r.size(); i++) {
    CHECK(0 <= r[i].lo && r[i].lo < r[i].hi && r[i].hi <= limit, "%s range %zu [%d, %d) of %d", what, i, r[i].lo, r[i].hi, limit);
    if (i) CHECK(r[i - 1].hi < r[i].lo, "%s ranges %zu and %zu touch or overlap", what, i - 1, i);
  }
}

void check_plan(const RunInputs& in, const std::vector<int>& groups, int out_h) {
  const RepaintPlan p = plan_repaint(in, groups, out_h);
  const int n = in.upsampling;
  if (!in.modular) {
    RunInputs coded = in;
    coded.upsampling = 1;
    const RerenderPlan r = plan_rerender(coded, groups);
    CHECK(r.route != RerenderPlan::kUnsupported, "unsharded VarDCT at upsampling 1 is never refused");
    if (n == 1) {  // the same answer as plan_rerender
      const RerenderPlan own = plan_rerender(in, groups);
      CHECK((own.route == RerenderPlan::kFullRun) == (p.route == RepaintPlan::kWholeRun), "route at upsampling 1");
      if (own.route == RerenderPlan::kBands) CHECK(same_bands(own.bands, p.bands), "bands at upsampling 1");
    }
    CHECK((r.route == RerenderPlan::kFullRun) == (p.route == RepaintPlan::kWholeRun), "route");
    if (r.route == RerenderPlan::kBands) {
      CHECK(p.route == RepaintPlan::kRerenderBands, "route bands");
      CHECK(same_bands(r.bands, p.bands), "coded bands equal plan_rerender's at upsampling 1");
    }
    CHECK(p.runs.empty(), "a VarDCT plan has no Modular runs");
  } else {
    // the maximal runs of listed group rows, stated on a bitmap of rows
    std::vector<char> listed((size_t)in.ygroups, 0);
    for (int g : groups) listed[(size_t)(g / in.xgroups)] = 1;
    std::vector<RunPlan> want;
    bool whole = !in.rendered || in.subsampled;
    for (int gy = 0; gy < in.ygroups;) {
      if (!listed[(size_t)gy]) {
        gy++;
        continue;
      }
      int e = gy;
      while (e < in.ygroups && listed[(size_t)e]) e++;
      want.push_back(plan_run(in, gy, e));
      whole |= want.back().whole;
      gy = e;
    }
    CHECK(whole == (p.route == RepaintPlan::kWholeRun), "Modular route");
    if (!whole) {
      CHECK(p.route == RepaintPlan::kModularBands && p.runs.size() == want.size() && p.bands.size() == want.size(), "runs");
      const int halo = in.stages.halo_px();
      for (size_t i = 0; i < want.size() && i < p.runs.size(); i++) {
        const RunPlan &a = want[i], &b = p.runs[i];
        CHECK(a.group_row0 == b.group_row0 && a.group_row1 == b.group_row1 && a.y_lo == b.y_lo && a.y_hi == b.y_hi &&
                  a.intake_y0 == b.intake_y0 && a.intake_y1 == b.intake_y1 && a.tiled == b.tiled && a.whole == b.whole &&
                  a.k1_row0 == b.k1_row0 && a.k1_row1 == b.k1_row1 && a.chroma_lazy == b.chroma_lazy,
              "run %zu equals plan_run's", i);
        CHECK(p.bands[i].y_lo == std::max(0, a.y_lo - halo) && p.bands[i].y_hi == std::min(in.ysize, a.y_hi + halo),
              "band %zu is the run widened by the reach", i);
        // the filters of the widened band read rows the intake has not taken in again: they must be unfiltered ones kept
        // from the whole run, i.e. the list must end in the other plane set
        if (halo > 0) CHECK(in.stages.result_in_tmp() == 1, "a band route with a halo needs the result in tmp");
        // every replaced sample (the run's rows) is inside the intake
        CHECK(b.intake_y0 <= a.y_lo && a.y_hi <= b.intake_y1, "intake covers the run");
        if (i) CHECK(p.bands[i - 1].y_hi < p.bands[i].y_lo, "bands disjoint");
      }
    }
  }
  if (p.route == RepaintPlan::kWholeRun) {
    CHECK(p.bands.empty() && p.centre_rows.empty() && p.noise_rows.empty(), "a whole run carries no rows");
    return;
  }
  if (n == 1) {
    CHECK(p.centre_rows.empty() && p.noise_rows.empty(), "no upsampling rows at factor 1");
    return;
  }
  // centre rows: the union of [y_lo - 2, y_hi + 2) clipped, disjoint and ascending (not even touching)
  check_ranges(p.centre_rows, in.ysize, "centre");
  std::vector<char> want((size_t)in.ysize, 0);
  for (const RowBand& b : p.bands)
    for (int y = std::max(0, b.y_lo - 2); y < std::min(in.ysize, b.y_hi + 2); y++) want[(size_t)y] = 1;
  CHECK(rows_of(p.centre_rows, in.ysize) == want, "centre rows are the union of the widened bands");
  // noise rows: n times the centre rows, clipped to the result height
  check_ranges(p.noise_rows, out_h, "noise");
  std::vector<char> nwant((size_t)out_h, 0);
  for (const RowRange& c : p.centre_rows)
    for (int y = c.lo * n; y < std::min(c.hi * n, out_h); y++) nwant[(size_t)y] = 1;
  CHECK(rows_of(p.noise_rows, out_h) == nwant, "noise rows are n times the centre rows, clipped");
}

void check_changed_rects(std::mt19937& rng, uint32_t xsize, uint32_t ysize, uint32_t n, bool modular, uint32_t gab,
                         uint32_t epf, bool sub, bool cut, const std::vector<uint32_t>& ids) {
  jxlh_frame_params p;
  std::memset(&p, 0, sizeof(p));
  p.abi_version = JXLH_ABI_VERSION;
  p.xsize = xsize, p.ysize = ysize, p.upsampling = n, p.gab = gab, p.epf_iters = epf;
  if (modular) p.flags |= JXLH_FRAME_MODULAR;
  if (sub) p.hshift[0] = p.hshift[2] = p.vshift[0] = p.vshift[2] = 1;
  if (cut && n > 1) {
    p.xsize_upsampled = xsize * n - 1 - rng() % (n - 1 ? n - 1 : 1);
    p.ysize_upsampled = ysize * n - (n - 1);
  }
  std::vector<jxlh_rect> rects;
  const jxlh_status st = plan_repaint_changed_rects(p, ids.data(), (uint32_t)ids.size(), rects);
  CHECK(st == JXLH_OK, "status %d", (int)st);
  if (st != JXLH_OK) return;
  if (!modular && n <= 1) {  // exactly jxlh_changed_rects' list
    std::vector<jxlh_rect> own;
    CHECK(plan_changed_rects(p, ids.data(), (uint32_t)ids.size(), own) == JXLH_OK && own.size() == rects.size() &&
              (own.empty() || !std::memcmp(own.data(), rects.data(), own.size() * sizeof(jxlh_rect))),
          "the list of plan_changed_rects");
    return;
  }
  uint32_t W, H;
  repaint_result_size(p, &W, &H);
  const uint32_t f = n > 1 ? n : 1;
  const ChangedReach reach = changed_reach(p);
  const uint32_t rx = reach.x + (f > 1 ? 2 : 0), ry = reach.y + (f > 1 ? 2 : 0);
  // per pixel: the union of the rects is the union of the widened, scaled cells; no pixel lies in two rects
  std::vector<uint8_t> want((size_t)W * H, 0), got((size_t)W * H, 0);
  const uint32_t xg = (xsize + 255) / 256;
  for (uint32_t g : ids) {
    const uint32_t gx = g % xg, gy = g / xg;
    const uint32_t x0 = gx * 256 > rx ? gx * 256 - rx : 0, x1 = std::min(xsize, std::min(xsize, gx * 256 + 256) + rx);
    const uint32_t y0 = gy * 256 > ry ? gy * 256 - ry : 0, y1 = std::min(ysize, std::min(ysize, gy * 256 + 256) + ry);
    for (uint32_t y = y0 * f; y < std::min(H, y1 * f); y++)
      for (uint32_t x = x0 * f; x < std::min(W, x1 * f); x++) want[(size_t)y * W + x] = 1;
  }
  for (const jxlh_rect& r : rects) {
    CHECK(r.w > 0 && r.h > 0 && r.x0 + r.w <= W && r.y0 + r.h <= H, "rect inside the %u x %u result", W, H);
    if (!(r.x0 + r.w <= W && r.y0 + r.h <= H)) return;
    for (uint32_t y = r.y0; y < r.y0 + r.h; y++)
      for (uint32_t x = r.x0; x < r.x0 + r.w; x++) got[(size_t)y * W + x]++;
  }
  bool disjoint = true;
  for (uint8_t v : got) disjoint &= v <= 1;
  CHECK(disjoint, "rects are disjoint (%ux%u n=%u)", xsize, ysize, n);
  CHECK(got == want || !disjoint, "the union is the widened cells' (%ux%u n=%u modular=%d)", xsize, ysize, n, (int)modular);
}

}  // namespace

int main() {
  std::mt19937 rng(20261020);
  const int sizes[][2] = {{8, 600}, {600, 8}, {255, 255}, {256, 256}, {257, 513}, {300, 600}, {264, 520}, {512, 768}, {700, 1030}};
  long plans = 0;
  for (const auto& sz : sizes)
    for (int gab = 0; gab < 2; gab++)
      for (int epf = 0; epf <= 3; epf++)
        for (int per_stage = 0; per_stage < 2; per_stage++)
          for (int modular = 0; modular < 2; modular++)
            for (int n : {1, 2, 4, 8})
              for (int flags = 0; flags < 32; flags++) {
                RunInputs in;
                in.stages = StageList{gab != 0, epf, per_stage != 0};
                in.xgroups = (sz[0] + 255) / 256, in.ygroups = (sz[1] + 255) / 256, in.ysize = sz[1];
                in.upsampling = n, in.modular = modular != 0;
                in.noise = flags & 1, in.draws_in_place = (flags & 2) != 0, in.subsampled = (flags & 4) != 0;
                in.rendered = !(flags & 8), in.strip_ran = (flags & 16) != 0 && !in.modular;
                const int ng = in.xgroups * in.ygroups;
                const int out_h = n > 1 && (flags & 1) ? sz[1] * n - (n - 1) : sz[1] * n;
                for (int rep = 0; rep < 4; rep++) {
                  std::vector<int> groups;
                  if (rep == 0) groups.push_back((int)(rng() % ng));
                  else if (rep == 1) for (int g = 0; g < ng; g++) groups.push_back(g);
                  else for (int g = 0; g < ng; g++) if (rng() % 3 == 0) groups.push_back(g);
                  if (groups.empty()) groups.push_back(ng - 1);
                  check_plan(in, groups, out_h);
                  plans++;
                }
              }
  long lists = 0;
  for (const auto& sz : sizes)
    for (uint32_t n : {1u, 2u, 4u, 8u})
      for (int modular = 0; modular < 2; modular++)
        for (uint32_t gab = 0; gab < 2; gab++)
          for (uint32_t epf = 0; epf <= 3; epf++)
            for (int sub = 0; sub < 2; sub++)
              for (int cut = 0; cut < 2; cut++) {
                if (n == 8 && sz[0] * sz[1] > 300 * 600) continue;  // (the per-pixel maps: keep the program quick)
                const uint32_t ng = (uint32_t)(((sz[0] + 255) / 256) * ((sz[1] + 255) / 256));
                std::vector<uint32_t> ids;
                for (uint32_t g = 0; g < ng; g++)
                  if (rng() % 2) ids.push_back(g);
                if (ids.empty()) ids.push_back(rng() % ng);
                ids.push_back(ids[0]);  // a duplicate counts once
                check_changed_rects(rng, (uint32_t)sz[0], (uint32_t)sz[1], n, modular != 0, gab, epf, sub != 0, cut != 0, ids);
                lists++;
              }
  // the argument checks are jxlh_changed_rects' (an id beyond the grid, a bad size), plus the factor
  {
    jxlh_frame_params p;
    std::memset(&p, 0, sizeof(p));
    p.abi_version = JXLH_ABI_VERSION;
    p.xsize = 300, p.ysize = 600, p.upsampling = 2;
    std::vector<jxlh_rect> rects;
    const uint32_t bad = 6, ok = 5;
    CHECK(plan_repaint_changed_rects(p, &bad, 1, rects) == JXLH_ERR_INVALID_ARGUMENT, "id beyond the grid");
    CHECK(plan_repaint_changed_rects(p, &ok, 1, rects) == JXLH_OK && rects.size() == 1, "last id");
    p.upsampling = 3;
    CHECK(plan_repaint_changed_rects(p, &ok, 1, rects) == JXLH_ERR_INVALID_ARGUMENT, "factor 3");
    p.upsampling = 2, p.xsize = 0;
    CHECK(plan_repaint_changed_rects(p, &ok, 1, rects) == JXLH_ERR_INVALID_ARGUMENT, "zero size");
    p.xsize = 300, p.abi_version = JXLH_ABI_VERSION + 1;
    CHECK(plan_repaint_changed_rects(p, &ok, 1, rects) == JXLH_ERR_INVALID_ARGUMENT, "abi version");
  }
  if (failures) {
    std::printf("repaint plans: %d failures\n", failures);
    return 1;
  }
  std::printf("repaint plans: ok (%ld plans, %ld rect lists)\n", plans, lists);
  return 0;
}
