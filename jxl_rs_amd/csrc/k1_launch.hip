// K1's host side: one call enqueues the launches k1_plan.h plans for it, each through the launcher of the file that
// holds its kernel (k_vardct_scan.hip, k_vardct.hip, k_vardct_special.hip, k_vardct_large.hip, k_coeffs.hip).
#include <atomic>

#include "k_vardct_common.h"

namespace jxlh {

// the environment switches of the plan (K1Inputs), read once
static int env_override(const char* name, bool empty_is_unset) {
  const char* e = getenv(name);
  return e && (*e || !empty_is_unset) ? atoi(e) : -1;
}

void launch_vardct_groups(hipStream_t s, const FrameDev& f_in, int group_row0, int group_row1,
                          void* worklist_mem, uint32_t* launch_parity, int* error_flag, int32_t* dense_coeffs,
                          const int* group_list, int n_list, bool has_special, bool has_large, int n_dense_route) {
  const int ngroups = k1_ngroups(group_list != nullptr, n_list, group_row0, group_row1, f_in.xgroups);
  if (ngroups <= 0) return;
  // The value that flags a batch for the fallback launch: unique per launch across the process, never 0.  The flag words
  // are zeroed when the work list is allocated or its layout moves (vardct_worklist_clear_flags), so a stale word holds an
  // earlier launch's epoch and never this one's.
  static std::atomic<uint32_t> epoch_counter{0};
  FrameDev f = f_in;
  uint32_t epoch = ++epoch_counter;
  if (epoch == 0) epoch = ++epoch_counter;
  f.fb_epoch = (int)epoch;
  // carve the work-list memory (vardct_worklist_layout): [two sets of counters, one 128-byte line each] [class 0 items] ...
  WorkLists wl;
  const uint32_t set = (*launch_parity)++ & 1u;
  wl.counts = reinterpret_cast<int*>(reinterpret_cast<char*>(worklist_mem) + set * kCountBytes);
  int* next_counts = reinterpret_cast<int*>(reinterpret_cast<char*>(worklist_mem) + (set ^ 1u) * kCountBytes);
  char* const base = reinterpret_cast<char*>(worklist_mem);
  const size_t nblocks = (size_t)f.xblocks * f.yblocks;
  const WorklistLayout L = vardct_worklist_layout(nblocks);
  for (int c = 0; c < kNumClasses; c++) wl.items[c] = reinterpret_cast<WorkItem*>(base + L.off[kWlItems0 + c]);
  for (int c = 0; c < kClsSpecial; c++) {
    wl.eitems[c] = reinterpret_cast<EntryItem*>(base + L.off[kWlEItems0 + c]);
    wl.ditems[c] = reinterpret_cast<WorkItem*>(base + L.off[kWlDItems0 + c]);
    wl.fallback[c] = reinterpret_cast<uint32_t*>(base + L.off[kWlFallback0 + c]);
  }
  wl.fb_any = reinterpret_cast<uint32_t*>(base + L.off[kWlFbAny]);
  uint32_t* large_units = reinterpret_cast<uint32_t*>(base + L.off[kWlLargeUnits]);  // behind the last list

  static const int force_inline = env_override("JXLH_K1_INLINE", true);
  static const int force_dense1632 = env_override("JXLH_K1_DENSE1632", true);
  static const int force_large_fused = env_override("JXLH_LARGE_FUSED", false);
  K1Inputs in{};
  in.ngroups = ngroups;
  in.frame_groups = f.xgroups * f.ygroups;
  in.nblocks = nblocks;
  // entries form: the direct kernels (+ the fallback launch) when a zero coefficient provably reconstructs to +0.0f
  in.form = f.se_entries ? (f.se_direct_ok ? kFormDirect : kFormEntries) : f.sp_sorted ? kFormSorted : kFormDense;
  in.subsampled = f.subsampled != 0;
  in.se_dense_hint = f.se_dense_hint;
  in.has_special = has_special;
  in.has_large = has_large;
  in.n_dense_route = n_dense_route;
  in.dense_slab = dense_coeffs != nullptr;
  in.group_route = f.group_route != nullptr;
  in.strip = f.strip_desc != nullptr;
  in.strip_all_closed = f.strip_all_closed != 0;
  in.force_inline = force_inline;
  in.force_dense1632 = force_dense1632;
  in.force_large_fused = force_large_fused;
  const K1Plan plan = plan_k1(in);

  for (int i = 0; i < plan.n; i++) {
    const K1Step& st = plan.step[i];
    if (st.lists == kK1DenseRouteLists) {
      // the routed groups' lists and counters, read from the dense slabs (at most one such step in a plan)
      WorkLists wd = wl;
      for (int c = 0; c < kClsSpecial; c++) wd.items[c] = wl.ditems[c];
      wd.counts = wl.counts + kCntDense0 * kCountPitch;
      FrameDev fd = f;
      fd.se_entries = nullptr;
      launch_k1_dct(s, st, fd, wd);
    } else if (st.kernel < kK1ExpandEntries) {
      launch_k1_scan(s, st, f, wl, group_row0, error_flag, group_list, ngroups, next_counts);
    } else if (st.kernel == kK1ExpandEntries) {
      launch_expand_entries(s, dense_coeffs, f.se_entries, f.se_counts, f.se_runs, f.group_dense, st.grid);
    } else if (st.kernel == kK1ExpandSorted) {
      launch_expand_sorted(s, dense_coeffs, f.sp_sorted, f.sp_slot_start, f.group_dense, st.grid);
    } else if (st.kernel < kK1Special0) {
      launch_k1_dct(s, st, f, wl);
    } else if (st.kernel < kK1ClassEnd) {
      launch_k1_special(s, st, f, wl);
    } else {
      launch_k1_large(s, st, plan.large_fuse, f, wl, large_units, nblocks);
    }
  }
}

}  // namespace jxlh
