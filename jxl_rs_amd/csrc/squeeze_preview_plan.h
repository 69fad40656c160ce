// The route of a progressive preview of a squeezed image (jxlh_unsqueeze_chain_preview): which levels of the chain
// are regular steps, which are smooth (their residuals have not arrived), which of them the final planes depend on,
// and the launches in order.  Plain C++, fixed-size arrays, no heap: host logic, tested without a device
// (tests/cpp/squeeze_preview_plan.cc).
//
// The rule is the reference's for whole channels (meta_apply.rs:150-161 links a step to the step of the other axis
// that feeds it; step.rs:138-150 picks the kind from the two residuals' DataStatus):
//   regular    the level's residual is there;
//   SMOOTH_2D  it is missing, level L - 1 squeezes the other axis and is missing too: the level upsamples the average
//              that level L - 1 reads (the output of level L - 2, or the base) in both axes at once;
//   SMOOTH_1D  it is missing otherwise: smooth_h / smooth_v on its own average, the output of level L - 1.
// A 2-D level does not read level L - 1's output, so that level may be dead: nothing the final planes depend on.
// The reference computes dead levels all the same; here they are not launched.
#pragma once
#include "squeeze_plan.h"

namespace jxlh {

// ---- kinds[i]: JXLH_PREVIEW_*; live[i] (may be null): 1 when the last level's planes depend on level i's
inline void squeeze_preview_kinds(int n_planes, int n_levels, const jxlh_squeeze_level* levels, uint8_t* kinds, uint8_t* live) {
  for (int i = 0; i < n_levels; i++) {
    if (!squeeze_level_missing(n_planes, levels[i])) kinds[i] = JXLH_PREVIEW_REGULAR;
    else if (i > 0 && (levels[i - 1].horizontal != 0) != (levels[i].horizontal != 0) && squeeze_level_missing(n_planes, levels[i - 1]))
      kinds[i] = JXLH_PREVIEW_SMOOTH_2D;
    else kinds[i] = JXLH_PREVIEW_SMOOTH_1D;
  }
  if (!live) return;
  for (int i = 0; i < n_levels; i++) live[i] = 0;
  for (int i = n_levels - 1; i >= 0; i -= kinds[i] == JXLH_PREVIEW_SMOOTH_2D ? 2 : 1) live[i] = 1;
}

// ---- one launch group behind the regular prefix: level `level` from src to dst
struct PreviewEntry {
  int level, kind;             // kind: JXLH_PREVIEW_*
  int src_level;               // the level whose output is read (-1: the base)
  SqueezeLoc src, dst;
  uint32_t src_w, src_h;       // the planes read
  bool rct;                    // smooth: the fused kernel applies the RCT (regular: the launches below say)
  int n_launch;                // regular: 1 or 2 (step, or fused step + RCT, or step and RCT)
  SqueezeLaunch launch[2];
};
struct SqueezePreviewPlan {
  uint8_t kinds[kSqueezeMaxLevels], live[kSqueezeMaxLevels];
  SqueezeArena arena;          // of the WHOLE chain: the prefix's plane sets are its first ones
  int n_prefix;                // levels [0, n_prefix): the longest regular prefix, through plan_squeeze_chain
  SqueezeChainIn prefix_in;    // ... as that chain: its `out` is the arena's plane set of level n_prefix - 1 unless nothing follows
  SqueezePlan prefix;
  int n;
  PreviewEntry entry[kSqueezeMaxLevels];
};

// `in` as for plan_squeeze_chain, levels checked with allow_missing (check_squeeze_chain)
inline SqueezePreviewPlan plan_squeeze_preview(const SqueezeChainIn& in) {
  SqueezePreviewPlan P{};
  const int nl = in.n_levels;
  squeeze_preview_kinds(in.n_planes, nl, in.levels, P.kinds, P.live);
  P.arena = squeeze_arena(in.n_planes, nl, in.levels);
  auto loc = [&](int i) {
    return i < 0 ? SqueezeLoc{kSqBase, in.base_stride} : i == nl - 1 ? SqueezeLoc{kSqOut, in.out_stride} : SqueezeLoc{i, P.arena.stride[i]};
  };
  while (P.n_prefix < nl && P.kinds[P.n_prefix] == JXLH_PREVIEW_REGULAR) P.n_prefix++;
  if (P.n_prefix > 0) {
    P.prefix_in = in;
    P.prefix_in.n_levels = P.n_prefix;
    if (P.n_prefix < nl) {  // something follows: the prefix ends in the arena, and the RCT is not its business
      const SqueezeLoc d = loc(P.n_prefix - 1);
      for (int p = 0; p < in.n_planes; p++) P.prefix_in.out[p] = squeeze_plane_addr(in, P.arena, d, p);
      P.prefix_in.out_stride = d.stride;
      P.prefix_in.with_rct = false;
    }
    P.prefix = plan_squeeze_chain(P.prefix_in);
  }
  for (int i = P.n_prefix; i < nl; i++) {
    if (!P.live[i]) continue;
    PreviewEntry& e = P.entry[P.n++];
    const jxlh_squeeze_level& lv = in.levels[i];
    e.level = i;
    e.kind = P.kinds[i];
    e.src_level = e.kind == JXLH_PREVIEW_SMOOTH_2D ? i - 2 : i - 1;
    e.src = loc(e.src_level);
    e.dst = loc(i);
    const bool last_rct = i == nl - 1 && in.with_rct;
    if (e.kind == JXLH_PREVIEW_REGULAR) {
      const SqueezeExtents x = squeeze_extents(lv.horizontal != 0, lv.out_w, lv.out_h);
      e.src_w = x.avg_w;
      e.src_h = x.avg_h;
      const SqueezeStep s = squeeze_level_step(in, P.arena, i, e.src, e.dst);
      e.n_launch = last_rct ? plan_squeeze_step_rct(s, in.separate_rct, e.launch) : (e.launch[0] = plan_squeeze_step(s), 1);
    } else {
      const bool fx = e.kind == JXLH_PREVIEW_SMOOTH_2D || lv.horizontal, fy = e.kind == JXLH_PREVIEW_SMOOTH_2D || !lv.horizontal;
      e.src_w = fx ? (lv.out_w + 1) / 2 : lv.out_w;
      e.src_h = fy ? (lv.out_h + 1) / 2 : lv.out_h;
      e.rct = last_rct;
    }
  }
  return P;
}

}  // namespace jxlh
