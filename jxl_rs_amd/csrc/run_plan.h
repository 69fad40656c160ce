// The routing of a frame run: what jxlh_frame_run, jxlh_frame_rerender_groups, a Modular frame's run and a sharded run
// launch, on which rows, and where the result ends up -- decided here, issued by frame_run.hip, abi_modular_frame.hip
// and comm.hip.  Plain C++: the planner is host logic, tested without a device (tests/cpp/run_plan.cc).
#pragma once
#include <algorithm>
#include <vector>

namespace jxlh {

// The frame's stage list (frame/render.rs:569-622): Gaborish, EPF0, EPF1, EPF2.  The only place that knows how many
// there are, their borders, and in which plane set (`planes`, the one the transforms write, or `tmp`) the list ends.
struct StageList {
  bool gab = false;
  int epf_iters = 0;
  bool per_stage = false;  // JXLH_FRAME_UNFUSED_FILTERS: one launch per stage, ping-pong planes <-> tmp
  enum Kind : int { kGaborish = -1, kEpf0, kEpf1, kEpf2 };  // (an EPF stage's kind is its launch_epf index)
  struct Stage { int kind, border; };
  // the per-stage sequence, in order; -> count
  int sequence(Stage s[4]) const {
    int n = 0;
    if (gab) s[n++] = {kGaborish, 1};
    if (epf_iters >= 3) s[n++] = {kEpf0, 3};
    if (epf_iters >= 1) s[n++] = {kEpf1, 2};
    if (epf_iters >= 2) s[n++] = {kEpf2, 1};
    return n;
  }
  int count() const { Stage s[4]; return sequence(s); }
  // rows the stages behind stage i read beyond its output: a single stage runs on its band widened by it
  int reach_after(int i) const {
    Stage s[4];
    int reach = 0;
    for (int n = sequence(s), k = i + 1; k < n; k++) reach += s[k].border;
    return reach;
  }
  int halo_px() const { return reach_after(-1); }  // rows the filters read beyond a band
  // production path: the whole list in one pass over HBM (two for epf_iters == 3), K1 writing the 8x8-tiled layout
  bool fused() const { return !per_stage && count() > 0; }
  // Where the list leaves the finished planes (1 = tmp, 0 = planes): a property of the frame, so a rank that filtered
  // nothing (empty band) still knows where the gathered frame lives.  Fused: one pass planes -> tmp; epf_iters == 3 is
  // Gaborish + EPF0 planes -> tmp, then EPF1 + EPF2 back tmp -> planes.
  int result_in_tmp() const { return count() == 0 ? 0 : per_stage ? count() & 1 : epf_iters >= 3 ? 0 : 1; }
  // launch_fused_filters' return code, whatever per_stage says: 0 = nothing to do, 1 = result in tmp, 2 = in planes
  int fused_where() const { return count() == 0 ? 0 : epf_iters >= 3 ? 2 : 1; }
};

// What the decisions read from the context and the frame parameters (frame_run.hip: run_inputs), and nothing else.
// noise: the flag is set and the LUT is not all zero.  draws_in_place: patches or splines, drawn IN PLACE on the finished
// planes.  strip_requested: JXLH_FRAME_STRIP, or the JXLH_STRIP environment hook.  lf_only: a group is marked
// (jxlh_frame_set_groups_lf_only).  rendered: a whole-frame run has happened in this frame; strip_ran: the last run went
// through the strip kernel.
struct RunInputs {
  StageList stages;
  int xgroups = 1, ygroups = 1, ysize = 1, upsampling = 1, nranks = 1;
  bool subsampled = false, modular = false, noise = false, draws_in_place = false, strip_requested = false;
  bool lf_only = false, rendered = false, strip_ran = false;
};

// A run of group rows [group_row0, group_row1) (whole: the whole frame): the transforms on group rows [k1_row0,
// k1_row1), the stage list on pixel rows [y_lo, y_hi), a Modular frame's intake on [intake_y0, intake_y1).
// strip_candidate: the run would go through the strip kernel, so the epoch must leave dense slabs.  tiled: K1 writes the
// 8x8-tiled layout (whenever the fused filter kernel is its only consumer).  chroma_lazy: the chroma upsampling waits
// until somebody asks for the planes.  exchange: a rank's band whose edge block rows come from its neighbours.
// sparse_k1 (the transforms read a bucketed form instead of the dense slabs) and strip (the strip kernel runs) are the
// coefficient epoch's answer: resolve_strip.
struct RunPlan {
  StageList stages;
  bool whole = false, strip_candidate = false, tiled = false, chroma_lazy = false, exchange = false;
  int group_row0 = 0, group_row1 = 0, k1_row0 = 0, k1_row1 = 0;
  int y_lo = 0, y_hi = 0, intake_y0 = 0, intake_y1 = 0;
  bool sparse_k1 = false, strip = false;
};

// Whole-frame runs of a 4:4:4 frame with Gaborish and / or EPF1 (+ EPF2) may go through the strip kernel (k_strip.hip):
// opt-in (JXLH_FRAME_STRIP), see the flag's comment in jxl_hip.h
inline bool strip_eligible(const RunInputs& in) {
  const StageList& s = in.stages;
  return in.strip_requested && !s.per_stage && !in.subsampled && s.epf_iters <= 2 && s.count() > 0 && in.nranks <= 1;
}

// group rows [r0, r1) with the transforms on [k0, k1): what every kind of run shares
inline RunPlan band_plan(const RunInputs& in, int r0, int r1, int k0, int k1) {
  const StageList& s = in.stages;
  RunPlan p{s};
  p.whole = r0 == 0 && r1 == in.ygroups;
  p.group_row0 = r0, p.group_row1 = r1, p.k1_row0 = k0, p.k1_row1 = k1;
  p.tiled = !in.modular && s.fused();  // (a Modular frame's intake writes raster planes)
  p.y_lo = r0 * 256;
  p.y_hi = std::min(r1 * 256, in.ysize);
  // the filters read up to 7 rows beyond the band, and the first pass of epf_iters == 3 starts on a multiple of 4: 8
  const int intake_halo = s.halo_px() > 0 ? 8 : 0;
  p.intake_y0 = std::max(0, p.y_lo - intake_halo);
  p.intake_y1 = std::min(in.ysize, p.y_hi + intake_halo);
  // A sub-sampled channel is reconstructed at its own resolution into tmp[c] and brought to full resolution into
  // planes[c] before any filter (frame/render.rs:569-576) -- or, when no stage follows at all, only when the planes are
  // asked for (materialise_chroma).  A sharded frame gathers planes[c] band by band (jxlh_frame_allgather): the
  // full-resolution chroma must exist on every rank before the gather, and a deferred upsampling would cover only this
  // rank's band afterwards.  (A Modular frame's run always upsamples.)
  const bool stages_follow = s.count() > 0 || in.upsampling > 1 || in.noise || in.draws_in_place;
  p.chroma_lazy = !in.modular && in.subsampled && !stages_follow && in.nranks <= 1;
  return p;
}

// jxlh_frame_run(group_row0, group_row1) (clamped and checked by the caller), VarDCT or Modular
inline RunPlan plan_run(const RunInputs& in, int group_row0, int group_row1) {
  const StageList& s = in.stages;
  const bool whole = group_row0 == 0 && group_row1 == in.ygroups;  // as asked for
  // VarDCT: patches and splines are drawn in place on the result.  When the result lives in the planes K1 writes and K1
  // rewrites a group row beyond the band (the filters' or the chroma upsampling's halo), a band run would overwrite
  // the neighbouring band's drawn pixels with bare ones: such a frame is rendered whole.
  // Modular: a band's halo rows are taken in again with every run.  When the stage list ends in the planes the intake
  // writes (no stage would be fine, but it has no halo; the two-pass list of epf_iters == 3; an even number of single
  // stages) that undoes the neighbouring band's finished rows -- drawn patches and splines included --, and the single
  // stages of JXLH_FRAME_UNFUSED_FILTERS write their intermediate halo rows over the neighbour's result in either set
  // of planes.  A sub-sampled channel is taken into tmp[c], the other set: with a halo its rows land on the neighbour's
  // result when the list ends THERE.  So a sub-sampled frame with a filter has no safe set at all.  Such frames are
  // rendered whole.
  const bool widen = in.modular ? s.halo_px() > 0 && (s.result_in_tmp() == 0 || (s.per_stage && s.count() > 1) || in.subsampled)
                                : in.draws_in_place && (s.halo_px() > 0 || in.subsampled) && s.result_in_tmp() == 0;
  if (!whole && widen) group_row0 = 0, group_row1 = in.ygroups;
  // K1 on the band plus one halo group row on each side (filters read across it; vertical chroma upsampling reads one
  // sub-sampled row beyond the band as well)
  const bool need_halo = s.halo_px() > 0 || in.subsampled;
  RunPlan p = band_plan(in, group_row0, group_row1, group_row0 - (need_halo && group_row0 > 0),
                        group_row1 + (need_halo && group_row1 < in.ygroups));
  // (a frame with a group whose HF has not arrived takes the two-kernel path: the strip kernel transforms every tile;
  // a run that became the whole frame only above ends in `planes`, which no list the strip kernel takes does)
  p.strip_candidate = !in.modular && whole && !in.lf_only && strip_eligible(in);
  return p;
}

// The strip kernel reads the dense slabs: candidacy is an INPUT of the coefficient epoch (coeff_epoch.h: want_strip
// keeps the epoch from leaving a bucketed form), and whether the slabs are what the frame is resident in is its OUTPUT.
inline RunPlan resolve_strip(RunPlan plan, bool sparse_k1) {
  plan.sparse_k1 = sparse_k1;
  plan.strip = plan.strip_candidate && !sparse_k1;
  return plan;
}

// jxlh_frame_rerender_groups: the frame is run again whole, or the stage list runs on the bands (disjoint, ascending)
struct RowBand { int y_lo, y_hi; bool whole_frame; };
struct RerenderPlan {
  enum Route { kBands, kFullRun, kUnsupported } route;
  std::vector<RowBand> bands;
};
inline RerenderPlan plan_rerender(const RunInputs& in, const std::vector<int>& sorted_unique_groups) {
  const StageList& s = in.stages;
  // A progressive Modular decode sets the changed rects and runs again.  Like a band run, the 5x5 upsampling window
  // crosses groups.  A rank of a sharded frame holds only its band: progressive re-renders run on unsharded contexts.
  if (in.modular || in.upsampling > 1 || in.nranks > 1) return {RerenderPlan::kUnsupported, {}};
  const int ns = s.count(), halo = s.halo_px();
  // Re-rendering a group needs its neighbours' UNFILTERED pixels (the filters read across the group edge).  They
  // are still in `planes` when the stage list leaves its result in `tmp` (the fused path with up to two EPF passes,
  // or no filter at all); a stage list that ends in `planes` has overwritten them (the single stages ping-pong
  // planes <-> tmp: kept only for one stage; the strip kernel leaves no unfiltered pixels at all), a sub-sampled frame
  // keeps them in another form, and a frame that was never rendered has none: those render the frame again.
  const bool unfiltered_kept = !in.strip_ran && (ns == 0 || (s.per_stage ? ns == 1 : s.result_in_tmp() != 0));
  // Noise is added IN PLACE to the result planes.  Without a filter stage the result lives in `planes`, the planes K1
  // writes: the groups that are not re-transformed would receive their noise a second time.
  // The same holds for patches and splines: they are drawn in place (an Add would reach the other groups twice).
  const bool noise_in_place = ns == 0 && (in.noise || in.draws_in_place);
  if (!in.rendered || !unfiltered_kept || in.subsampled || noise_in_place) return {RerenderPlan::kFullRun, {}};
  // The filters on every pixel row the listed groups influence: their own rows widened by the stage list's reach
  // (mark_group_to_rerender's 3x3 neighbourhood, restricted to what can actually change), merged into bands
  RerenderPlan p{RerenderPlan::kBands, {}};
  for (int g : sorted_unique_groups) {
    const int gy = g / in.xgroups, lo = std::max(0, gy * 256 - halo), hi = std::min(in.ysize, (gy + 1) * 256 + halo);
    if (!p.bands.empty() && p.bands.back().y_hi >= lo) p.bands.back().y_hi = std::max(p.bands.back().y_hi, hi);
    else p.bands.push_back({lo, hi, false});
  }
  for (RowBand& b : p.bands) b.whole_frame = b.y_lo == 0 && b.y_hi == in.ysize;
  return p;
}

// A rank's band [r0, r1) of a sharded frame (possibly empty).  The ranks trade the block rows at their band edges
// between the transforms and the filters.  Chroma-subsampled frames keep the recomputed halo group row instead (their
// vertical upsampling reads across the band edge in the sub-sampled domain): the transforms then take one more group
// row on either side.  Frames without filters need no halo at all.
inline RunPlan plan_shard(const RunInputs& in, int r0, int r1) {
  const bool exchange = in.stages.halo_px() > 0 && !in.subsampled;
  const bool recompute = r0 < r1 && !exchange && (in.stages.halo_px() > 0 || in.subsampled);
  RunPlan p = band_plan(in, r0, r1, recompute ? std::max(0, r0 - 1) : r0, recompute ? std::min(in.ygroups, r1 + 1) : r1);
  p.exchange = exchange;
  return p;
}

}  // namespace jxlh
