// jxlh_frame_repaint_groups and jxlh_repaint_changed_rects (jxl_hip_repaint.h), decided here and issued by
// frame_run.hip / abi_save.hip: which route a repaint of listed 256 x 256 cells takes on a VarDCT or Modular frame of
// any upsampling factor, the coded row bands it rewrites, the coded rows whose upsampled patches are computed again and
// the result rows that receive their noise again.  Built on plan_rerender and plan_run (run_plan.h) and on changed_reach
// (save_rects_plan.h): what those decide is not restated.  Plain C++: host logic, tested without a device
// (tests/cpp/repaint_plan.cc).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "run_plan.h"
#include "save_rects_plan.h"

namespace jxlh {

struct RowRange { int lo, hi; };

// Upsample<N> reads a 5 x 5 window (BORDER 2): a rewritten coded row changes the patches of the two rows on either side
constexpr int kUpsampleBorder = 2;

// route kWholeRun: jxlh_frame_run(0, all).  kRerenderBands (VarDCT): the transforms of the listed groups, then the stage
// list on `bands`.  kModularBands: runs[i] is plan_run's answer for the i-th maximal run of listed group rows (its
// intake), and bands[i] the rows its stage list runs on: the run's own rows widened by the stage list's reach, because a
// replaced sample changes the filtered rows of the neighbouring band too (the unfiltered rows the filters read there are
// still in `planes`: such a frame's list ends in `tmp`, or plan_run has made the run whole).
// centre_rows (upsampling > 1, disjoint, ascending): the coded rows whose N x N patches are computed again -- every
// band widened by kUpsampleBorder, clipped, merged where they overlap or touch.  noise_rows: the result rows those
// patches cover, [n * lo, min(n * hi, out_h)): they hold bare pixels afterwards and receive the noise again, once.
// At upsampling 1 both are empty: the band's own post stages add the noise on the band (run_post_stages).
struct RepaintPlan {
  enum Route { kWholeRun, kRerenderBands, kModularBands } route = kWholeRun;
  std::vector<RowBand> bands;
  std::vector<RunPlan> runs;
  std::vector<RowRange> centre_rows, noise_rows;
};

// in: the frame as run_inputs gives it (never sharded: refused by the caller); out_h: the height of the result
inline RepaintPlan plan_repaint(const RunInputs& in, const std::vector<int>& sorted_unique_groups, int out_h) {
  RepaintPlan p;
  if (sorted_unique_groups.empty()) {
    p.route = in.modular ? RepaintPlan::kModularBands : RepaintPlan::kRerenderBands;
    return p;
  }
  if (in.modular) {
    // A frame that was never rendered whole has no finished rows to keep.  A chroma-subsampled frame stays out of the
    // band route: its chroma upsampling reads one sub-sampled row across the band edge, which a band run does not redo.
    if (!in.rendered || in.subsampled) return p;
    const int halo = in.stages.halo_px();
    p.route = RepaintPlan::kModularBands;
    for (size_t i = 0; i < sorted_unique_groups.size();) {
      const int gy0 = sorted_unique_groups[i] / in.xgroups;
      int gy1 = gy0 + 1;
      for (; i < sorted_unique_groups.size() && sorted_unique_groups[i] / in.xgroups <= gy1; i++)
        gy1 = std::max(gy1, sorted_unique_groups[i] / in.xgroups + 1);
      const RunPlan r = plan_run(in, gy0, gy1);
      if (r.whole) return RepaintPlan{};  // asked for, or plan_run's decision: one whole run serves every listed row
      p.runs.push_back(r);
      p.bands.push_back({std::max(0, r.y_lo - halo), std::min(in.ysize, r.y_hi + halo), false});
    }
  } else {
    RunInputs coded = in;
    coded.upsampling = 1;  // the coded-size part is a re-render's; what upsampling adds follows below
    RerenderPlan r = plan_rerender(coded, sorted_unique_groups);
    if (r.route != RerenderPlan::kBands) return p;  // (kUnsupported: sharded, which never gets here)
    p.route = RepaintPlan::kRerenderBands;
    p.bands = std::move(r.bands);
  }
  if (in.upsampling > 1) {
    for (const RowBand& b : p.bands) {
      const int lo = std::max(0, b.y_lo - kUpsampleBorder), hi = std::min(in.ysize, b.y_hi + kUpsampleBorder);
      if (!p.centre_rows.empty() && p.centre_rows.back().hi >= lo) p.centre_rows.back().hi = std::max(p.centre_rows.back().hi, hi);
      else p.centre_rows.push_back({lo, hi});
    }
    for (const RowRange& c : p.centre_rows) {
      const int lo = c.lo * in.upsampling, hi = std::min(c.hi * in.upsampling, out_h);
      if (lo < hi) p.noise_rows.push_back({lo, hi});
    }
  }
  return p;
}

// ---- jxlh_repaint_changed_rects
// The size of the result of a frame with these parameters
inline void repaint_result_size(const jxlh_frame_params& p, uint32_t* w, uint32_t* h) {
  const uint32_t n = p.upsampling > 1 ? p.upsampling : 1;
  *w = n > 1 && p.xsize_upsampled ? p.xsize_upsampled : p.xsize * n;
  *h = n > 1 && p.ysize_upsampled ? p.ysize_upsampled : p.ysize * n;
}

// The rects into `rects`; returns the status jxlh_repaint_changed_rects returns apart from the cap protocol.
// VarDCT at upsampling <= 1: plan_changed_rects' list as it is.  Otherwise every listed cell, clipped to the frame,
// widened by changed_reach and (upsampling n > 1) by the upsampling window's 2 coded pixels, clipped to the coded size,
// scaled by n and clipped to the result -- as DISJOINT rects of exactly their union: per band of rows between two rect
// edges one rect per maximal run of covered columns, bands with the same columns joined.
inline jxlh_status plan_repaint_changed_rects(const jxlh_frame_params& p, const uint32_t* group_ids, uint32_t count,
                                              std::vector<jxlh_rect>& rects) {
  const bool modular = (p.flags & JXLH_FRAME_MODULAR) != 0;
  if (!modular && p.upsampling <= 1) return plan_changed_rects(p, group_ids, count, rects);
  // the argument checks and the cells widened by changed_reach, one rect per run of neighbours in a group row: those
  // of the same frame as a VarDCT frame without upsampling (changed_reach reads neither)
  jxlh_frame_params coded = p;
  coded.upsampling = 1;
  coded.flags &= ~(uint32_t)JXLH_FRAME_MODULAR;
  if (jxlh_status st = plan_changed_rects(coded, group_ids, count, rects)) return st;
  const uint32_t n = p.upsampling > 1 ? p.upsampling : 1;
  if (n != 1 && n != 2 && n != 4 && n != 8) {
    rects.clear();
    return JXLH_ERR_INVALID_ARGUMENT;
  }
  uint32_t W, H;
  repaint_result_size(p, &W, &H);
  const uint32_t border = n > 1 ? (uint32_t)kUpsampleBorder : 0;
  struct Box { uint32_t x0, y0, x1, y1; };
  std::vector<Box> boxes;
  std::vector<uint32_t> ys;
  for (const jxlh_rect& r : rects) {
    Box b;
    b.x0 = (r.x0 > border ? r.x0 - border : 0) * n;
    b.y0 = (r.y0 > border ? r.y0 - border : 0) * n;
    b.x1 = std::min(W, std::min(p.xsize, r.x0 + r.w + border) * n);
    b.y1 = std::min(H, std::min(p.ysize, r.y0 + r.h + border) * n);
    if (b.x0 >= b.x1 || b.y0 >= b.y1) continue;  // (cut off whole by xsize_upsampled / ysize_upsampled)
    boxes.push_back(b);
    ys.push_back(b.y0);
    ys.push_back(b.y1);
  }
  rects.clear();
  std::sort(ys.begin(), ys.end());
  ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
  size_t prev_first = 0, prev_end = 0;  // the rects of the band above, for joining
  for (size_t k = 0; k + 1 < ys.size(); k++) {
    const uint32_t ya = ys[k], yb = ys[k + 1];
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    for (const Box& b : boxes)
      if (b.y0 <= ya && yb <= b.y1) spans.push_back({b.x0, b.x1});
    std::sort(spans.begin(), spans.end());
    std::vector<std::pair<uint32_t, uint32_t>> merged;
    for (const auto& s : spans) {
      if (!merged.empty() && merged.back().second >= s.first) merged.back().second = std::max(merged.back().second, s.second);
      else merged.push_back(s);
    }
    // the same columns as the band above, which ends where this one starts: grow its rects
    bool same = prev_end - prev_first == merged.size() && !merged.empty();
    for (size_t i = 0; same && i < merged.size(); i++) {
      const jxlh_rect& a = rects[prev_first + i];
      same = a.x0 == merged[i].first && a.x0 + a.w == merged[i].second && a.y0 + a.h == ya;
    }
    if (same) {
      for (size_t i = prev_first; i < prev_end; i++) rects[i].h += yb - ya;
      continue;
    }
    prev_first = rects.size();
    for (const auto& s : merged) rects.push_back(jxlh_rect{s.first, ya, s.second - s.first, yb - ya});
    prev_end = rects.size();
  }
  return JXLH_OK;
}

}  // namespace jxlh
