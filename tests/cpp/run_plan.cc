// The frame run's planner (jxl_rs_amd/csrc/run_plan.h) over its whole input space, against the expressions it replaced:
// those stood between the launches of jxlh_frame_run, jxlh_frame_rerender_groups, modular_frame_run and the sharded
// runs, and are transcribed below as they were, one function per place they came from; none of them calls the header.
// Plus the invariants that tie the former copies together.  Host only, no device.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../jxl_rs_amd/csrc/run_plan.h"

using namespace jxlh;

namespace {

// what the former expressions read: FrameDev f, jxlh_frame_params p and the context's flags, by their old names
struct Old {
  int gab, epf_iters;
  bool unfused;  // p.flags & JXLH_FRAME_UNFUSED_FILTERS
  bool subsampled, modular, draws_in_place, noise, strip_flag, lf_only, rendered, strip_ran;
  int nranks, upsampling, xgroups, ygroups, ysize;
};
constexpr int kGroupDim = 256;

// ---- jxlh_ctx.h: result_in_tmp
int old_result_in_tmp(const Old& f) {
  const int ns = (f.gab ? 1 : 0) + (f.epf_iters >= 3 ? 1 : 0) + (f.epf_iters >= 1 ? 1 : 0) + (f.epf_iters >= 2 ? 1 : 0);
  if (ns == 0) return 0;
  if (!f.unfused) return f.epf_iters >= 3 ? 0 : 1;
  return ns & 1;
}
// ---- abi_frame.hip: run_prologue
int old_halo_px(const Old& f) {
  return (f.gab ? 1 : 0) + (f.epf_iters >= 3 ? 3 : 0) + (f.epf_iters >= 1 ? 2 : 0) + (f.epf_iters >= 2 ? 1 : 0);
}
bool old_will_fuse(const Old& f) { return !f.unfused && (f.gab || f.epf_iters > 0); }
// ---- abi_frame.hip: strip_eligible
bool old_strip_eligible(const Old& f) {
  return f.strip_flag && !f.unfused && !f.subsampled && f.epf_iters <= 2 && (f.gab || f.epf_iters >= 1) && f.nranks <= 1;
}
// ---- k_filters_fused.hip: launch_fused_filters (its return value)
int old_fused_where(const Old& f) {
  const bool gab = f.gab != 0, e0 = f.epf_iters >= 3, e1 = f.epf_iters >= 1, e2 = f.epf_iters >= 2;
  if (!gab && !e1 && !e2) return 0;
  if (e0) return 2;
  return 1;
}
// ---- abi_frame.hip: run_stages_rows (the single stages: kind, and the rows stage s runs on for [y_lo, y_hi))
struct OldStage { int kind, y0, y1; };
std::vector<OldStage> old_single_stages(const Old& f, int y_lo, int y_hi) {
  int stages[4], borders[4], ns = 0;
  if (f.gab) { stages[ns] = -1; borders[ns++] = 1; }
  if (f.epf_iters >= 3) { stages[ns] = 0; borders[ns++] = 3; }
  if (f.epf_iters >= 1) { stages[ns] = 1; borders[ns++] = 2; }
  if (f.epf_iters >= 2) { stages[ns] = 2; borders[ns++] = 1; }
  std::vector<OldStage> out;
  for (int s = 0; s < ns; s++) {
    int later = 0;
    for (int k = s + 1; k < ns; k++) later += borders[k];
    out.push_back({stages[s], std::max(0, y_lo - later), std::min(f.ysize, y_hi + later)});
  }
  return out;
}
// ---- abi_frame.hip: jxlh_frame_run + run_stages (+ run_k1 for the chroma upsampling)
struct OldRun {
  bool whole, want_strip_in;  // want_strip as the coefficient epoch is asked
  int group_row0, group_row1, gr0, gr1, y_lo, y_hi;
  bool chroma_lazy, tiled;
};
OldRun old_frame_run(const Old& f, int group_row0, int group_row1) {
  OldRun r;
  bool whole = group_row0 == 0 && group_row1 == f.ygroups;
  r.want_strip_in = whole && !f.lf_only && old_strip_eligible(f);
  const int halo_px = old_halo_px(f);
  if (!whole && f.draws_in_place && (halo_px > 0 || f.subsampled) && old_result_in_tmp(f) == 0) {
    group_row0 = 0;
    group_row1 = f.ygroups;
    whole = true;
  }
  const bool need_halo = halo_px > 0 || f.subsampled;
  r.gr0 = need_halo && group_row0 > 0 ? group_row0 - 1 : group_row0;
  r.gr1 = need_halo && group_row1 < f.ygroups ? group_row1 + 1 : group_row1;
  r.group_row0 = group_row0;
  r.group_row1 = group_row1;
  r.whole = group_row0 == 0 && group_row1 == f.ygroups;  // run_stages, and `rendered`
  r.y_lo = group_row0 * kGroupDim;
  r.y_hi = std::min(group_row1 * kGroupDim, f.ysize);
  // run_k1
  const bool stages_follow = f.gab || f.epf_iters > 0 || f.upsampling > 1 || f.noise || f.draws_in_place;
  r.chroma_lazy = f.subsampled && !(stages_follow || f.nranks > 1);
  r.tiled = old_will_fuse(f);
  return r;
}
// ---- abi_modular_frame.hip: modular_frame_run
struct OldModularRun {
  bool whole;
  int y_lo, y_hi, ya, yb;
};
OldModularRun old_modular_run(const Old& f, int group_row0, int group_row1) {
  const int ns = (f.gab ? 1 : 0) + (f.epf_iters >= 3 ? 1 : 0) + (f.epf_iters >= 1 ? 1 : 0) + (f.epf_iters >= 2 ? 1 : 0);
  const int halo_px = (f.gab ? 1 : 0) + (f.epf_iters >= 3 ? 3 : 0) + (f.epf_iters >= 1 ? 2 : 0) + (f.epf_iters >= 2 ? 1 : 0);
  const bool per_stage = f.unfused;
  bool whole = group_row0 == 0 && group_row1 == f.ygroups;
  if (!whole && halo_px > 0 && (old_result_in_tmp(f) == 0 || (per_stage && ns > 1) || f.subsampled)) {
    group_row0 = 0;
    group_row1 = f.ygroups;
    whole = true;
  }
  OldModularRun r;
  r.whole = whole;
  r.y_lo = group_row0 * kGroupDim;
  r.y_hi = std::min(group_row1 * kGroupDim, f.ysize);
  const int halo = halo_px > 0 ? 8 : 0;
  r.ya = std::max(0, r.y_lo - halo);
  r.yb = std::min(f.ysize, r.y_hi + halo);
  return r;
}
// ---- abi_frame.hip: jxlh_frame_rerender_groups
struct OldRerender {
  bool unsupported = false, full_run = false;
  std::vector<RowBand> bands;  // run_stages_rows calls, in order
};
OldRerender old_rerender(const Old& f, const std::vector<int>& upload) {
  OldRerender r;
  if (f.modular) { r.unsupported = true; return r; }
  if (f.upsampling > 1) { r.unsupported = true; return r; }
  if (f.nranks > 1) { r.unsupported = true; return r; }
  const int ns = (f.gab ? 1 : 0) + (f.epf_iters >= 3 ? 1 : 0) + (f.epf_iters >= 1 ? 1 : 0) + (f.epf_iters >= 2 ? 1 : 0);
  const bool per_stage = f.unfused;
  const bool unfiltered_kept = !f.strip_ran && (ns == 0 || (per_stage ? ns == 1 : old_result_in_tmp(f) != 0));
  const bool noise_in_place = ns == 0 && (f.noise || f.draws_in_place);
  if (!f.rendered || !unfiltered_kept || f.subsampled || noise_in_place) { r.full_run = true; return r; }
  const int halo_px = old_halo_px(f);  // run_prologue
  const int n = (int)upload.size();
  int prev_lo = -1, prev_hi = -1;
  for (int i = 0; i <= n; i++) {
    int lo = -1, hi = -1;
    if (i < n) {
      const int gy = upload[i] / f.xgroups;
      lo = std::max(0, gy * kGroupDim - halo_px);
      hi = std::min(f.ysize, (gy + 1) * kGroupDim + halo_px);
    }
    if (i < n && prev_hi >= lo) {
      prev_hi = std::max(prev_hi, hi);
      continue;
    }
    if (prev_lo >= 0) r.bands.push_back({prev_lo, prev_hi, prev_lo == 0 && prev_hi == f.ysize});
    prev_lo = lo;
    prev_hi = hi;
  }
  return r;
}
// ---- comm.hip: exchange_applies, shard_k1
bool old_exchange_applies(const Old& f) { return old_halo_px(f) > 0 && !f.subsampled; }
void old_shard_k1_rows(const Old& f, int r0, int r1, int* g0, int* g1) {
  *g0 = r0;
  *g1 = r1;
  if (!old_exchange_applies(f) && (old_halo_px(f) > 0 || f.subsampled)) {
    *g0 = std::max(0, *g0 - 1);
    *g1 = std::min(f.ygroups, *g1 + 1);
  }
}

int failures = 0;
#define CHECK(cond, f)                                                                                                  \
  do {                                                                                                                  \
    if (!(cond) && failures++ < 20)                                                                                     \
      std::printf("line %d: %s  [gab %d epf %d unfused %d sub %d modular %d draws %d noise %d strip %d lf_only %d "     \
                  "rendered %d strip_ran %d nranks %d upsampling %d ygroups %d]\n",                                      \
                  __LINE__, #cond, f.gab, f.epf_iters, f.unfused, f.subsampled, f.modular, f.draws_in_place, f.noise,   \
                  f.strip_flag, f.lf_only, f.rendered, f.strip_ran, f.nranks, f.upsampling, f.ygroups);                 \
  } while (0)

RunInputs inputs_of(const Old& f) {
  RunInputs in;
  in.stages.gab = f.gab != 0;
  in.stages.epf_iters = f.epf_iters;
  in.stages.per_stage = f.unfused;
  in.xgroups = f.xgroups;
  in.ygroups = f.ygroups;
  in.ysize = f.ysize;
  in.subsampled = f.subsampled;
  in.modular = f.modular;
  in.upsampling = f.upsampling;
  in.noise = f.noise;
  in.draws_in_place = f.draws_in_place;
  in.strip_requested = f.strip_flag;
  in.nranks = f.nranks;
  in.lf_only = f.lf_only;
  in.rendered = f.rendered;
  in.strip_ran = f.strip_ran;
  return in;
}

void check_stage_list(const Old& f) {
  const StageList s = inputs_of(f).stages;
  CHECK(s.halo_px() == old_halo_px(f), f);
  CHECK(s.fused() == old_will_fuse(f), f);
  CHECK(s.result_in_tmp() == old_result_in_tmp(f), f);
  CHECK(s.fused_where() == old_fused_where(f), f);
  // the fused launcher's code and the plane set say the same thing
  if (s.fused()) CHECK(s.fused_where() == (s.result_in_tmp() ? 1 : 2), f);
  StageList::Stage seq[4];
  const int n = s.sequence(seq);
  CHECK(n == s.count(), f);
  for (int y_lo : {0, 256})
    for (int y_hi : {256, f.ysize}) {
      const std::vector<OldStage> old = old_single_stages(f, y_lo, y_hi);
      CHECK((int)old.size() == n, f);
      for (int i = 0; i < n && i < (int)old.size(); i++) {
        CHECK(seq[i].kind == old[i].kind, f);
        CHECK(std::max(0, y_lo - s.reach_after(i)) == old[i].y0 && std::min(f.ysize, y_hi + s.reach_after(i)) == old[i].y1, f);
      }
    }
}

void check_runs(const Old& f) {
  const RunInputs in = inputs_of(f);
  for (int r0 = 0; r0 < f.ygroups; r0++)
    for (int r1 = r0 + 1; r1 <= f.ygroups; r1++) {
      const RunPlan p = plan_run(in, r0, r1);
      if (f.modular) {
        const OldModularRun o = old_modular_run(f, r0, r1);
        CHECK(p.whole == o.whole && p.y_lo == o.y_lo && p.y_hi == o.y_hi, f);
        CHECK(p.intake_y0 == o.ya && p.intake_y1 == o.yb, f);
        CHECK(!p.tiled && !p.chroma_lazy && !p.strip_candidate, f);  // f.tiled = 0, chroma_lazy = false, no strip path
      } else {
        const OldRun o = old_frame_run(f, r0, r1);
        CHECK(p.whole == o.whole && p.group_row0 == o.group_row0 && p.group_row1 == o.group_row1, f);
        CHECK(p.strip_candidate == o.want_strip_in, f);
        CHECK(p.k1_row0 == o.gr0 && p.k1_row1 == o.gr1, f);
        CHECK(p.y_lo == o.y_lo && p.y_hi == o.y_hi, f);
        CHECK(p.chroma_lazy == o.chroma_lazy && p.tiled == o.tiled, f);
        for (bool sparse_k1 : {false, true}) {  // run_prologue: want_strip = want_strip && !sparse_k1
          const RunPlan q = resolve_strip(p, sparse_k1);
          CHECK(q.sparse_k1 == sparse_k1 && q.strip == (o.want_strip_in && !sparse_k1), f);
        }
      }
      // a widened run is a whole run; the transforms' rows contain the stage rows' group rows
      if (p.group_row0 != r0 || p.group_row1 != r1) CHECK(p.whole, f);
      CHECK(p.whole == (p.group_row0 == 0 && p.group_row1 == f.ygroups), f);
      CHECK(p.k1_row0 <= p.group_row0 && p.group_row1 <= p.k1_row1 && p.k1_row0 >= 0 && p.k1_row1 <= f.ygroups, f);
      CHECK(p.y_lo == p.group_row0 * kGroupDim && p.y_hi > p.y_lo && p.y_hi <= f.ysize, f);
      CHECK(p.stages.count() == in.stages.count() && p.stages.per_stage == in.stages.per_stage, f);
      // a rank's band (an empty one included: r0 == r1 below)
      const RunPlan sp = plan_shard(in, r0, r1);
      int g0, g1;
      old_shard_k1_rows(f, r0, r1, &g0, &g1);
      CHECK(sp.exchange == old_exchange_applies(f), f);
      CHECK(sp.k1_row0 == g0 && sp.k1_row1 == g1, f);
      CHECK(sp.group_row0 == r0 && sp.group_row1 == r1 && !sp.strip_candidate, f);
      CHECK(sp.y_lo == r0 * kGroupDim && sp.y_hi == std::min(r1 * kGroupDim, f.ysize), f);
      CHECK(sp.whole == (r0 == 0 && r1 == f.ygroups) && sp.tiled == (!f.modular && old_will_fuse(f)), f);
      if (!f.modular) CHECK(sp.chroma_lazy == old_frame_run(f, r0, r1).chroma_lazy, f);
      CHECK(sp.k1_row0 <= r0 && r1 <= sp.k1_row1, f);
    }
  const RunPlan empty = plan_shard(in, f.ygroups, f.ygroups);  // shard_k1 returns before the transforms
  CHECK(empty.group_row0 >= empty.group_row1 && empty.k1_row0 >= empty.k1_row1 && empty.exchange == old_exchange_applies(f), f);
}

void check_rerenders(const Old& f) {
  const RunInputs in = inputs_of(f);
  for (int mask = 1; mask < (1 << f.ygroups); mask++) {
    std::vector<int> groups;  // every group of the chosen rows: sorted, unique, several per row
    for (int gy = 0; gy < f.ygroups; gy++)
      if (mask >> gy & 1)
        for (int gx = 0; gx < f.xgroups; gx++) groups.push_back(gy * f.xgroups + gx);
    const RerenderPlan p = plan_rerender(in, groups);
    const OldRerender o = old_rerender(f, groups);
    CHECK((p.route == RerenderPlan::kUnsupported) == o.unsupported, f);
    CHECK((p.route == RerenderPlan::kFullRun) == o.full_run, f);
    if (p.route != RerenderPlan::kBands) {
      CHECK(p.bands.empty(), f);
      continue;
    }
    CHECK(p.bands.size() == o.bands.size() && !p.bands.empty(), f);
    for (size_t i = 0; i < p.bands.size() && i < o.bands.size(); i++)
      CHECK(p.bands[i].y_lo == o.bands[i].y_lo && p.bands[i].y_hi == o.bands[i].y_hi &&
                p.bands[i].whole_frame == o.bands[i].whole_frame, f);
    // disjoint, ascending, inside the frame
    int prev_hi = -1;
    for (const RowBand& b : p.bands) {
      CHECK(b.y_lo >= 0 && b.y_lo < b.y_hi && b.y_hi <= f.ysize && b.y_lo > prev_hi, f);
      prev_hi = b.y_hi;
    }
  }
}

}  // namespace

int main() {
  long n = 0;
  for (int bits = 0; bits < (1 << 12); bits++)
    for (int epf = 0; epf <= 3; epf++)
      for (int ygroups = 1; ygroups <= 3; ygroups++) {
        auto bit = [bits](int i) { return (bits >> i & 1) != 0; };
        Old f;
        f.gab = bit(0);
        f.epf_iters = epf;
        f.unfused = bit(1);
        f.subsampled = bit(2);
        f.modular = bit(3);
        f.draws_in_place = bit(4);
        f.noise = bit(5);
        f.strip_flag = bit(6);
        f.lf_only = bit(7);
        f.rendered = bit(8);
        f.strip_ran = bit(9);
        f.nranks = bit(10) ? 2 : 1;
        f.upsampling = bit(11) ? 2 : 1;
        f.xgroups = 2;
        f.ygroups = ygroups;
        f.ysize = (ygroups - 1) * kGroupDim + 88;  // 88, 344, 600: no multiple of 256
        check_stage_list(f);
        check_runs(f);
        check_rerenders(f);
        n++;
      }
  if (failures) {
    std::printf("run plans: %d FAILED checks over %ld inputs\n", failures, n);
    return 1;
  }
  std::printf("run plans: ok (%ld inputs)\n", n);
  return 0;
}
