// What the two preview plan programs (squeeze_preview_plan.cc, squeeze_tiles_plan.cc) share: the CHECK macro, the
// generator's random numbers, and the checks of a whole-level entry -- the same for a plan without grids and for the
// whole levels that stand beside cell-wise ones in a plan with grids.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../jxl_rs_amd/csrc/squeeze_preview_plan.h"

namespace {
using namespace jxlh;

int g_fail = 0;
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

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 24);
}
uint32_t rnd(uint32_t lo, uint32_t hi) { return lo + rnd() % (hi - lo + 1); }

bool same_loc(const SqueezeLoc& a, const SqueezeLoc& b) { return a.where == b.where && a.stride == b.stride; }
bool same_launch(const SqueezeLaunch& a, const SqueezeLaunch& b) {
  return a.kind == b.kind && a.level0 == b.level0 && a.n_levels == b.n_levels && a.vec == b.vec && a.ncw == b.ncw &&
         same_loc(a.src, b.src) && same_loc(a.dst, b.dst);
}

// A whole-level entry `e` (kind >= 0) of plan P of chain `in`: it reads a plane set that was written before it (written[]:
// the levels whose output exists when the entry is issued; n_pre: the plan's prefix), of the size it expects, and
// writes its own; nothing reaches past the arena; the RCT rides on the last level only, by the kernel that fits it.
void check_whole_entry(int id, const SqueezeChainIn& in, const PreviewEntry& e, int n_pre, const bool* written) {
  const int nl = in.n_levels, n_planes = in.n_planes, i = e.level;
  const jxlh_squeeze_level* lv = in.levels;
  const SqueezeArena A = squeeze_arena(n_planes, nl, lv);
  auto arena_addr = [&](int level, int p) { return in.arena + sizeof(int32_t) * (A.off[level] + (size_t)p * A.plane[level]); };
  // what is read: a 2-D level the planes level - 1 reads, anything else the level's own average
  const bool two_d = e.kind == JXLH_PREVIEW_SMOOTH_2D;
  const SqueezeLoc& rd = two_d ? e.src2 : e.src;
  const uint32_t rw = two_d ? e.src2_w : e.src_w, rh = two_d ? e.src2_h : e.src_h;
  const int s = rd.where == kSqBase ? -1 : rd.where;  // the level whose output is read (-1: the base)
  CHECK(s == (two_d ? i - 2 : i - 1), "chain %d level %d reads %d", id, i, s);
  CHECK(s == -1 || (s >= n_pre - 1 && s >= 0 && s < i && written[s]), "chain %d level %d reads level %d before it is written", id, i, s);
  // where: the base, or the arena's plane set of the level read; never `out` (only the last level writes it)
  if (s < 0) CHECK(rd.where == kSqBase && rd.stride == in.base_stride, "chain %d level %d: base", id, i);
  else CHECK(rd.where == s && s < nl - 1 && rd.stride == A.stride[s], "chain %d level %d: source plane set", id, i);
  if (s < -1 || s >= nl) return;
  const uint32_t sw = s < 0 ? in.base_w : lv[s].out_w, sh = s < 0 ? in.base_h : lv[s].out_h;
  CHECK(rw == sw && rh == sh, "chain %d level %d: reads %u x %u of a %u x %u plane", id, i, rw, rh, sw, sh);
  // the smooth kernels' geometry: the doubled axes halve (rounding up) to the source
  const bool fx = two_d || lv[i].horizontal, fy = two_d || !lv[i].horizontal;
  CHECK(sw == (fx ? (lv[i].out_w + 1) / 2 : lv[i].out_w) && sh == (fy ? (lv[i].out_h + 1) / 2 : lv[i].out_h), "chain %d level %d: geometry", id, i);
  if (e.kind != JXLH_PREVIEW_REGULAR)  // a complete pair on every doubled axis: the kernels write every sample
    CHECK((fx ? lv[i].out_w / 2 : lv[i].out_w) > 0 && (fy ? lv[i].out_h / 2 : lv[i].out_h) > 0, "chain %d level %d: no pair", id, i);
  if (i == nl - 1) CHECK(e.dst.where == kSqOut && e.dst.stride == in.out_stride, "chain %d: the last level writes out", id);
  else CHECK(e.dst.where == i && e.dst.stride == A.stride[i], "chain %d level %d: destination", id, i);
  // arena extents
  for (const SqueezeLoc* l : {&rd, &e.dst}) {
    if (l->where < 0) continue;
    const int a = l->where;
    CHECK(a < nl - 1 && lv[a].out_w <= A.stride[a] && A.stride[a] * (size_t)lv[a].out_h <= A.plane[a] &&
              A.off[a] + (size_t)n_planes * A.plane[a] <= A.total, "chain %d level %d: plane set %d leaves the arena", id, i, a);
    for (int p = 0; p < n_planes; p++)
      CHECK(squeeze_plane_addr(in, A, *l, p) == arena_addr(a, p) && arena_addr(a, p) + 4 * A.plane[a] <= in.arena + 4 * A.total, "chain %d", id);
  }
  // the RCT: on the last level alone, by the kernel that fits it
  const bool last_rct = i == nl - 1 && in.with_rct;
  CHECK(e.rct == last_rct, "chain %d level %d: RCT", id, i);
  CHECK(e.n_smooth == 0 && e.n_runs == 0, "chain %d level %d: lists of a whole level", id, i);
  if (e.kind == JXLH_PREVIEW_REGULAR) {
    const SqueezeStep st = squeeze_level_step(in, A, i, e.src, e.dst);
    SqueezeLaunch L[2];
    const int n = last_rct ? plan_squeeze_step_rct(st, in.separate_rct, L) : (L[0] = plan_squeeze_step(st), 1);
    CHECK(e.n_launch == n, "chain %d level %d: %d launches", id, i, e.n_launch);
    for (int j = 0; j < n && j < e.n_launch; j++) CHECK(same_launch(e.launch[j], L[j]), "chain %d level %d launch %d", id, i, j);
    const bool has_rct = e.launch[0].kind == SqueezeLaunch::kFusedRct ||
                         (e.n_launch == 2 && (e.launch[1].kind == SqueezeLaunch::kRctFlat || e.launch[1].kind == SqueezeLaunch::kRctRows));
    CHECK(has_rct == last_rct, "chain %d level %d: RCT launch", id, i);
  } else {
    CHECK(e.n_launch == 0, "chain %d level %d: launches of a smooth level", id, i);
  }
}

}  // namespace
