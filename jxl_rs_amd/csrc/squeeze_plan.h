// The route of an inverse squeeze: which kernel takes which levels of a chain (or a single step), in which variant,
// from which planes to which -- decided here, issued by abi_squeeze.hip through the launchers of k_squeeze.hip.
// Plain C++, fixed-size arrays, no heap: host logic, tested without a device (tests/cpp/squeeze_plan.cc).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/jxl_hip.h"

// Kernel geometry the decisions depend on (k_squeeze.hip ties its tiles to them)
#define JXLH_SQT_S 32       // tiled kernels: steps per chunk
#define JXLH_SQL_MAX 128    // k6_unsqueeze_levels: largest plane side handled in LDS
#define JXLH_SQL_LEVELS 16  // ... and the most levels one launch takes

namespace jxlh {

constexpr int kFlowMaxLevels = 16;   // k6_unsqueeze_flow: levels of one dataflow launch
constexpr int kFlowWordStride = 64;  // ints between two progress words: one 256-byte line each (polls spread over channels)
constexpr int kFlowRunCap = kFlowMaxLevels < 16 ? kFlowMaxLevels : 16;
constexpr int kSqueezeMaxLevels = 64;          // levels of one chain call
constexpr uint32_t kMaxModularDim = 1u << 20;  // the kernels take `int` line counts / lengths

// ---- one level: the average and residual planes behind an out_w x out_h output
struct SqueezeExtents { uint32_t avg_w, avg_h, res_w, res_h; bool has_res; };
inline SqueezeExtents squeeze_extents(bool horizontal, uint32_t out_w, uint32_t out_h) {
  const uint32_t rw = horizontal ? out_w / 2 : out_w, rh = horizontal ? out_h : out_h / 2;
  return {horizontal ? (out_w + 1) / 2 : out_w, horizontal ? out_h : (out_h + 1) / 2, rw, rh, (size_t)rw * rh > 0};
}

// a level whose residuals have not arrived (progressive previews, squeeze_preview_plan.h): it has residual samples and
// names no plane of them
inline bool squeeze_level_missing(int n_planes, const jxlh_squeeze_level& lv) {
  if (!squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h).has_res) return false;
  for (int p = 0; p < n_planes; p++)
    if (lv.res[p]) return false;
  return true;
}

// ---- a chain's arguments: every level doubles (up to the odd sample) the axis it squeezes, starting from the base;
// every plane that is read or written is a device pointer (is_dev).  allow_missing: a level may leave out ALL its
// residual planes (jxlh_unsqueeze_chain_preview); one that leaves out some is refused either way
template <class IsDev>
jxlh_status check_squeeze_chain(int n_planes, int n_levels, const jxlh_squeeze_level* levels, const int32_t* const base[],
                                size_t base_stride, uint32_t base_w, uint32_t base_h, int32_t* const out[],
                                size_t out_stride, IsDev is_dev, bool allow_missing = false) {
  if (!levels || !base || !out || n_planes < 1 || n_planes > 3 || n_levels < 1 || n_levels > kSqueezeMaxLevels ||
      base_w == 0 || base_h == 0 || base_stride < base_w)
    return JXLH_ERR_INVALID_ARGUMENT;
  uint32_t cw = base_w, ch = base_h;
  for (int i = 0; i < n_levels; i++) {
    const jxlh_squeeze_level& lv = levels[i];
    if (lv.out_w == 0 || lv.out_h == 0 || lv.out_w > kMaxModularDim || lv.out_h > kMaxModularDim)
      return JXLH_ERR_INVALID_ARGUMENT;
    const SqueezeExtents e = squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h);
    if (e.avg_w != cw || e.avg_h != ch) return JXLH_ERR_INVALID_ARGUMENT;
    const bool missing = allow_missing && squeeze_level_missing(n_planes, lv);
    for (int p = 0; p < n_planes && !missing; p++)
      if (e.has_res && (!lv.res[p] || !is_dev(lv.res[p]) || lv.res_stride < e.res_w)) return JXLH_ERR_INVALID_ARGUMENT;
    cw = lv.out_w;
    ch = lv.out_h;
  }
  if (out_stride < cw) return JXLH_ERR_INVALID_ARGUMENT;
  for (int p = 0; p < n_planes; p++)
    if (!base[p] || !out[p] || !is_dev(base[p]) || !is_dev(out[p])) return JXLH_ERR_INVALID_ARGUMENT;
  return JXLH_OK;
}

// ---- one step over n_planes planes of one geometry, as the qualifying rules read it (addresses: alignment only)
struct SqueezeStep {
  bool horizontal;
  int n_planes;
  uint32_t out_w, out_h;
  size_t avg_stride, res_stride, out_stride;
  uintptr_t avg[3], res[3], out[3];  // the launchers take these as the planes
};
// every sample offset inside the step's three planes is below 2^log2
inline bool squeeze_spans_below(const SqueezeStep& s, int log2) {
  const size_t lim = (size_t)1 << log2;
  return s.out_stride * (size_t)s.out_h < lim && s.avg_stride * (size_t)s.out_h < lim && s.res_stride * (size_t)s.out_h < lim;
}
// long lines go through the mover / chain workgroups (tiled, dataflow: 32-bit offsets); short ones keep the one-wave
// kernel: nothing to stream, and a 256-thread workgroup would idle three waves
inline bool squeeze_streamed(const SqueezeStep& s) {
  return (int)(s.horizontal ? s.out_w : s.out_h) / 2 >= 4 * JXLH_SQT_S && squeeze_spans_below(s, 31);
}
// rows and planes start on 16 bytes: what all three 16-byte movers below need
inline bool squeeze_quads(const SqueezeStep& s) {
  bool ok = s.avg_stride % 4 == 0 && s.res_stride % 4 == 0 && s.out_stride % 4 == 0;
  for (int p = 0; p < s.n_planes && p < 3; p++) ok = ok && s.avg[p] % 16 == 0 && s.res[p] % 16 == 0 && s.out[p] % 16 == 0;
  return ok;
}
// k6_unsqueeze<HVEC>: a lane walks along its row with int4 accesses, horizontal steps only
inline bool squeeze_onewave_hvec(const SqueezeStep& s) { return s.horizontal && squeeze_quads(s); }
// TiledLines::vec of the tiled / dataflow kernels: 16-byte buffer accesses; a vertical step's 64-column groups must be
// whole quads of the rows, and every byte offset from a plane's first sample fits 32 bits with room for the slots
inline bool squeeze_tiled_vec(const SqueezeStep& s) {
  return squeeze_quads(s) && (s.horizontal || s.out_w % 4 == 0) && squeeze_spans_below(s, 30);
}
// k6_unsqueeze_rct<false, VEC, NCW>: the vertical step's vector movers; wide planes take 32 columns per workgroup
inline bool squeeze_fused_vec(const SqueezeStep& s) { return !s.horizontal && s.out_w % 4 == 0 && squeeze_quads(s); }
inline int squeeze_fused_ncw(const SqueezeStep& s) { return squeeze_fused_vec(s) && s.out_w >= 4096 && s.out_w % 32 == 0 ? 2 : 1; }

// ---- k6_unsqueeze_levels: n levels from the base in one launch.  Every plane side <= JXLH_SQL_MAX, and every plane
// written to the kernel's half-size buffer (the base when n is odd, every second level counted from the end) and every
// residual tile fits it: rows * (width | 1) <= 128 * 65
inline bool squeeze_levels_fit(int n, const jxlh_squeeze_level* levels, uint32_t base_w, uint32_t base_h) {
  if (n < 1 || n > JXLH_SQL_LEVELS || base_w == 0 || base_h == 0 || base_w > JXLH_SQL_MAX || base_h > JXLH_SQL_MAX) return false;
  auto fits_half = [](uint32_t w, uint32_t h) { return (size_t)h * (w | 1u) <= (size_t)JXLH_SQL_MAX * (JXLH_SQL_MAX / 2 + 1); };
  for (int i = 0; i < n; i++) {
    const jxlh_squeeze_level& lv = levels[i];
    if (lv.out_w == 0 || lv.out_h == 0 || lv.out_w > JXLH_SQL_MAX || lv.out_h > JXLH_SQL_MAX) return false;
    const SqueezeExtents e = squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h);
    if (e.has_res && !fits_half(e.res_w, e.res_h)) return false;
  }
  if ((n & 1) && !fits_half(base_w, base_h)) return false;
  for (int i = n - 2; i >= 0; i -= 2)
    if (!fits_half(levels[i].out_w, levels[i].out_h)) return false;
  return true;
}

// ---- the intermediate planes of a chain, in samples: every level but the last writes its own plane set (levels overlap
// in the dataflow launch, so no ping-pong; about twice the largest one in all).  Rows are padded to whole 16 bytes and
// every plane starts on a 256-byte line: with residual planes laid out the same way every level moves in 16-byte accesses.
struct SqueezeArena { size_t off[kSqueezeMaxLevels], stride[kSqueezeMaxLevels], plane[kSqueezeMaxLevels], total; };
inline SqueezeArena squeeze_arena(int n_planes, int n_levels, const jxlh_squeeze_level* levels) {
  SqueezeArena a{};
  for (int i = 0; i < n_levels - 1; i++) {
    a.off[i] = a.total;
    a.stride[i] = ((size_t)levels[i].out_w + 3) & ~(size_t)3;
    a.plane[i] = (a.stride[i] * levels[i].out_h + 63) & ~(size_t)63;
    a.total += a.plane[i] * n_planes;
  }
  return a;
}
// ints of progress scratch for a dataflow launch of n levels
inline size_t squeeze_flow_words(int n_planes, int n, const jxlh_squeeze_level* levels) {
  size_t words = 2 * kFlowWordStride;  // the ticket; slack behind the last word (a peek may look one word past a level's groups)
  for (int i = 0; i < n; i++)
    words += (size_t)n_planes * (((levels[i].horizontal ? levels[i].out_h : levels[i].out_w) + 63) / 64) * kFlowWordStride;
  return words;
}

// ---- the plan.  A launch covers levels [level0, level0 + n_levels) (an RCT: none) and moves planes from src to dst.
enum : int { kSqBase = -1, kSqOut = -2 };
struct SqueezeLoc { int where; size_t stride; };  // where: kSqBase, kSqOut, or i: the arena's plane set of level i
struct SqueezeLaunch {
  enum Kind : int { kLevels, kFlow, kTiled, kOneWave, kFusedRct, kRctFlat, kRctRows };
  Kind kind;
  int level0, n_levels;
  int vec;  // kTiled: TiledLines::vec; kOneWave: HVEC; kFusedRct: VEC (kFlow: per level, SqueezePlan::vec)
  int ncw;  // kFusedRct: chain waves
  SqueezeLoc src, dst;
};

// a single step: streamed lines tiled, anything else on the one-wave kernel
inline SqueezeLaunch plan_squeeze_step(const SqueezeStep& s) {
  const bool tiled = squeeze_streamed(s);
  return {tiled ? SqueezeLaunch::kTiled : SqueezeLaunch::kOneWave, 0, 1, tiled ? squeeze_tiled_vec(s) : squeeze_onewave_hvec(s),
          1, {}, {}};
}
// a step of three planes with the RCT behind it: fused below 2^31 samples per plane (32-bit offsets) unless the separate
// route is asked for, else the step and the RCT -- with a row pitch when the rows are padded.  -> launches
inline int plan_squeeze_step_rct(const SqueezeStep& s, bool separate, SqueezeLaunch L[2]) {
  if (!separate && squeeze_spans_below(s, 31)) {
    L[0] = {SqueezeLaunch::kFusedRct, 0, 1, squeeze_fused_vec(s), squeeze_fused_ncw(s), {}, {}};
    return 1;
  }
  L[0] = plan_squeeze_step(s);
  L[1] = {s.out_stride == s.out_w ? SqueezeLaunch::kRctFlat : SqueezeLaunch::kRctRows, 0, 0, 0, 1, {}, {}};
  return 2;
}

// What the chain's route reads.  Addresses as integers: the route reads their alignment only.  separate_rct: JXLH_SEPARATE_RCT=1
// (tests: the two-pass route that planes of 2^31 samples and more need); flow: not JXLH_CHAIN_FLOW=0 (tests, A/B: one
// launch per streamed level instead of the dataflow launch).
struct SqueezeChainIn {
  int n_planes, n_levels;
  const jxlh_squeeze_level* levels;
  uint32_t base_w, base_h;
  size_t base_stride, out_stride;
  uintptr_t base[3], out[3], arena;
  bool with_rct, separate_rct, flow;
};
struct SqueezePlan {
  SqueezeArena arena;
  size_t flow_words;  // the largest dataflow launch's progress scratch (0: none)
  int n;
  SqueezeLaunch launch[kSqueezeMaxLevels + 1];
  uint8_t vec[kSqueezeMaxLevels];  // TiledLines::vec of the levels inside dataflow launches
};
// where plane p of `l` lives, and level i from src to dst as a step (a level without residuals names its averages)
inline uintptr_t squeeze_plane_addr(const SqueezeChainIn& in, const SqueezeArena& A, SqueezeLoc l, int p) {
  return l.where == kSqBase ? in.base[p] : l.where == kSqOut ? in.out[p]
         : in.arena + sizeof(int32_t) * (A.off[l.where] + (size_t)p * A.plane[l.where]);
}
inline SqueezeStep squeeze_level_step(const SqueezeChainIn& in, const SqueezeArena& A, int i, SqueezeLoc src, SqueezeLoc dst) {
  const jxlh_squeeze_level& lv = in.levels[i];
  SqueezeStep s{lv.horizontal != 0, in.n_planes, lv.out_w, lv.out_h, src.stride, lv.res_stride, dst.stride, {}, {}, {}};
  for (int p = 0; p < in.n_planes; p++) {
    s.avg[p] = squeeze_plane_addr(in, A, src, p);
    s.res[p] = lv.res[p] ? (uintptr_t)lv.res[p] : s.avg[p];
    s.out[p] = squeeze_plane_addr(in, A, dst, p);
  }
  return s;
}
// 1. while the planes fit LDS, the first levels are one launch: at least 2 (the last level stays out when an RCT follows
//    it), shortened from the end until it fits;
// 2. runs of 2 .. kFlowRunCap consecutive streamed levels are one dataflow launch (never the level an RCT follows);
// 3. anything else is one launch per level, the last one fused with the RCT or followed by it.
inline SqueezePlan plan_squeeze_chain(const SqueezeChainIn& in) {
  SqueezePlan P{};
  P.arena = squeeze_arena(in.n_planes, in.n_levels, in.levels);
  const int nl = in.n_levels;
  auto loc = [&](int i) { return i == nl - 1 ? SqueezeLoc{kSqOut, in.out_stride} : SqueezeLoc{i, P.arena.stride[i]}; };
  auto step = [&](int i, SqueezeLoc src) { return squeeze_level_step(in, P.arena, i, src, loc(i)); };
  auto push = [&](const SqueezeLaunch& L, int level0, SqueezeLoc src, SqueezeLoc dst) {
    P.launch[P.n++] = {L.kind, level0, L.n_levels, L.vec, L.ncw, src, dst};
  };
  int i = 0;
  SqueezeLoc cur{kSqBase, in.base_stride};
  int n_small = 0;
  while (n_small < nl - (in.with_rct ? 1 : 0) && n_small < JXLH_SQL_LEVELS && in.levels[n_small].out_w <= JXLH_SQL_MAX &&
         in.levels[n_small].out_h <= JXLH_SQL_MAX)
    n_small++;
  while (n_small >= 2 && !squeeze_levels_fit(n_small, in.levels, in.base_w, in.base_h)) n_small--;
  if (n_small >= 2) {
    push({SqueezeLaunch::kLevels, 0, n_small, 0, 1, {}, {}}, 0, cur, loc(n_small - 1));
    cur = loc(n_small - 1);
    i = n_small;
  }
  while (i < nl) {
    if (in.flow) {
      SqueezeLoc a = cur;
      int n = 0;
      for (int j = i; j < nl && n < kFlowRunCap && !(j == nl - 1 && in.with_rct); j++, n++) {
        const SqueezeStep s = step(j, a);
        if (!squeeze_streamed(s)) break;
        P.vec[j] = squeeze_tiled_vec(s);
        a = loc(j);
      }
      if (n >= 2) {
        push({SqueezeLaunch::kFlow, 0, n, 0, 1, {}, {}}, i, cur, a);
        P.flow_words = std::max(P.flow_words, squeeze_flow_words(in.n_planes, n, in.levels + i));
        cur = a;
        i += n;
        continue;
      }
    }
    SqueezeLaunch L[2];
    const SqueezeStep s = step(i, cur);
    const bool rct = i == nl - 1 && in.with_rct;
    const int k = rct ? plan_squeeze_step_rct(s, in.separate_rct, L) : (L[0] = plan_squeeze_step(s), 1);
    push(L[0], i, cur, loc(i));
    if (k == 2) push(L[1], i, loc(i), loc(i));
    cur = loc(i);
    i++;
  }
  return P;
}

}  // namespace jxlh
