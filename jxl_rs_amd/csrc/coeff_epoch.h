// The coefficient epoch: the submissions between two jxlh_frame_run calls, the form the frame is resident in, and the
// plan that takes the one to the other at the next run (frame_run.hip: apply_coeff_epoch issues it).  Plain C++: the
// planner is host logic, tested without a device (tests/cpp/coeff_epoch_plan.cc).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace jxlh {

// sparse coefficient transport (k_coeffs.hip): one descriptor per submitted group
struct SparseGroup {
  uint32_t group;   // group id
  uint32_t offset;  // index of the group's first pair in the pair buffer (X pairs, then Y, then B)
  uint32_t n[3];    // pairs per channel
  uint32_t flags;   // bit 0: add the pairs to the group's current slab instead of starting from zero
};
struct WideValue { uint32_t pos, val; };  // a value outside the pairs' / entries' range (the device reads uint2)
constexpr uint32_t kEpochGroupCoeffs = 3 * 256 * 256;  // coefficients of a group (3 x kGroupArea)

// a group's submission in this epoch: none (it keeps what it holds), a dense slab (jxlh_submit_group), pair words in
// the pair buffer (jxlh_submit_group(s)_sparse, _sparse8, _sparse4), entries in the pending set (jxlh_submit_groups_slots)
enum class Sub : uint8_t { kKept, kDense, kPairs, kSlots };
// what the transforms read the frame from: the dense slabs, the pair words bucketed by slot (sp_sorted + sp_slot_start:
// K1 mode 1), or the live set of slot-bucketed entries in place (the routed groups from their slabs)
enum class Resident : uint8_t { kDense, kSortedPairs, kEntries };
struct Residence {
  Resident form = Resident::kDense;
  std::vector<uint8_t> route;  // kEntries: route[g] != 0 = group g is read from its slab (empty = none) ...
  int n_route = 0;             // ... and how many (0 unless kEntries)
  int se_dense_hint = 0;       // kEntries: FrameDev::se_dense_hint of the groups read in place
};

struct EpochGroup {
  Sub sub = Sub::kKept;
  bool accumulate = false;  // JXLH_GROUP_ACCUMULATE: the pairs / entries add to what the group holds
  bool wide = false;        // a pending wide value addresses the group
  uint64_t entries = 0;     // pairs / entries of its submission
};
struct EpochInputs {
  std::vector<EpochGroup> groups;
  size_t n_desc = 0, n_wide = 0;         // pending pair descriptors and wide values
  bool expand_sparse = false;            // JXLH_FRAME_EXPAND_SPARSE
  bool want_strip = false;               // the caller would run the strip kernel (it reads the dense slabs)
  Residence before;
};
// which pair descriptors are uploaded; they are expanded into the slabs together with the wide values, or sorted
enum class Descs : uint8_t { kNone, kAll, kRouted };
struct EpochPlan {
  Residence after;               // kEntries: the live and pending sets trade places
  std::vector<uint8_t> rebuild;  // groups whose slab is rebuilt from the old resident form first (empty = none)
  std::vector<uint8_t> widen;    // slot groups whose entries become pair words (empty = none)
  Descs descs = Descs::kNone;
  bool sort = false;             // kAll: k_sort_sparse instead of the expansion
  bool pending_read = false;     // the pending set has been read by the widening (and stays the pending one)
  bool trade_sets() const { return after.form == Resident::kEntries; }
};

inline EpochPlan plan_coeff_epoch(const EpochInputs& in) {
  const size_t n = in.groups.size();
  size_t n_sparse = 0, n_slots = 0, n_kept = 0, n_accum = 0;
  for (const EpochGroup& g : in.groups) {
    n_sparse += g.sub == Sub::kPairs || g.sub == Sub::kSlots;
    n_slots += g.sub == Sub::kSlots;
    n_kept += g.sub == Sub::kKept;
    n_accum += g.accumulate;
  }
  const bool dense_run = in.expand_sparse || in.want_strip;
  // K1 reads the pairs themselves (bucketed by slot) when every group arrived sparse in this epoch, self-contained ...
  const bool all_pairs = in.n_wide == 0 && in.n_desc == n && !dense_run && n_sparse == n && n_accum == 0;
  // ... and, every group slot-bucketed, the pending set holds the frame the way the transforms read it
  const bool all_slots = all_pairs && n_slots == n;
  // per-group routing: every group arrived in this epoch and MOST of them slot-bucketed and self-contained -- the
  // others (a dense slab, plain pairs, a wide value, a pass added to earlier content) are brought into their slabs
  // and read from there, the slot-bucketed ones are still read in place
  EpochPlan p;
  std::vector<uint8_t>& route = p.after.route;
  size_t n_inplace = 0;
  if (n_slots && !all_slots && !dense_run && n_kept == 0) {
    route.resize(n);
    for (size_t g = 0; g < n; g++) {
      const EpochGroup& e = in.groups[g];
      route[g] = !(e.sub == Sub::kSlots && !e.accumulate && !e.wide);
      n_inplace += !route[g];
    }
  }
  const bool routed = n_inplace && 2 * n_inplace >= n;
  if (!routed) route.clear();
  // leaving a bucketed form: groups not resubmitted now (or only added to) need their slab -- unless the slab already
  // was where they lived (a routed group)
  if (in.before.form != Resident::kDense && !all_pairs) {
    const std::vector<uint8_t>& had = in.before.route;
    p.rebuild.resize(n);
    for (size_t g = 0; g < n; g++)
      p.rebuild[g] = (in.groups[g].sub == Sub::kKept || in.groups[g].accumulate) && !(had.size() == n && had[g]);
  }
  // slot groups that take the general route become pair words at their reserved places of the pair buffer
  if (n_slots && !all_slots) {
    p.widen.resize(n);
    for (size_t g = 0; g < n; g++) p.widen[g] = in.groups[g].sub == Sub::kSlots && (!routed || route[g]);
    p.pending_read = !routed;
  }
  for (std::vector<uint8_t>* v : {&p.rebuild, &p.widen})
    if (std::count(v->begin(), v->end(), 1) == 0) v->clear();
  if (all_slots || routed) {
    p.after.form = Resident::kEntries;
    p.descs = routed ? Descs::kRouted : Descs::kNone;
    p.after.n_route = routed ? (int)(n - n_inplace) : 0;
    // entries per coefficient of the groups read in place: from about three times d1's share (0.086 on the synthetic
    // frame) the 8x8 class is better off running its over-depth batches inline, and from about 1.5 times most
    // 16..32-point batches are beyond the direct path's depth (profiles/r06_c_density.txt, r06_p_density.txt)
    uint64_t entries = 0, groups = 0;
    for (size_t g = 0; g < n; g++) {
      if (routed && route[g]) continue;
      entries += in.groups[g].entries;
      groups++;
    }
    const double share = groups ? (double)entries / (double)(groups * kEpochGroupCoeffs) : 0.0;
    p.after.se_dense_hint = share > 0.25 ? 2 : share > 0.125 ? 1 : 0;
  } else {
    p.after.form = all_pairs ? Resident::kSortedPairs : Resident::kDense;
    p.descs = Descs::kAll;
    p.sort = all_pairs;
  }
  return p;
}

// A context's coefficient state (jxlh_ctx::epoch, under sp_mutex)
struct CoeffEpoch {
  std::vector<EpochGroup> groups;            // this epoch's submission per group (sub, accumulate)
  std::vector<SparseGroup> pending, upload;  // pair descriptors of this epoch / of the last run (its copies read them)
  std::vector<WideValue> wide, wide_upload;  // wide values, the same way
  size_t pairs_used = 0;                     // pairs reserved in this epoch (pair buffer, pending entries set)
  bool dirty = false;                        // something was submitted in this epoch
  Residence live;                            // the form the frame is resident in
  EpochPlan plan;  // the last run's plan: its route / rebuild / widen arrays are what that run's copies read
  // Groups whose HF has not arrived (jxlh_frame_set_groups_lf_only; the reference's channel_status == DataStatus::Zero):
  // state of the FRAME, not of the epoch -- reset() leaves it alone, a new frame calls clear_lf_only(), and any
  // submission of a group takes its mark away (record()).  Empty until a group is marked in the frame.
  std::vector<uint8_t> lf_only;
  size_t n_lf_only = 0;

  void clear_lf_only() {
    lf_only.clear();
    n_lf_only = 0;
  }
  void mark_lf_only(uint32_t g) {
    if (lf_only.size() != groups.size()) lf_only.assign(groups.size(), 0);
    n_lf_only += !lf_only[g];
    lf_only[g] = 1;
  }
  // a new frame (nothing resident) / after a run has consumed the epoch (the caller then installs the plan's outcome)
  void reset(size_t ngroups) {
    groups.assign(ngroups, EpochGroup{});
    pending.clear();
    wide.clear();
    pairs_used = 0;
    dirty = false;
    live = Residence{};
  }
  bool sparse(uint32_t g) const { return groups[g].sub == Sub::kPairs || groups[g].sub == Sub::kSlots; }
  // a submission of group g; a dense slab replaces whatever the group was given earlier in the epoch, its wide
  // values included
  void record(uint32_t g, Sub kind, bool accumulate) {
    if (kind == Sub::kDense) {
      pending.erase(std::remove_if(pending.begin(), pending.end(), [g](const SparseGroup& d) { return d.group == g; }),
                    pending.end());
      wide.erase(std::remove_if(wide.begin(), wide.end(), [g](const WideValue& w) { return w.pos / kEpochGroupCoeffs == g; }),
                 wide.end());
    }
    groups[g].sub = kind;
    groups[g].accumulate = accumulate;
    dirty = true;
    if (n_lf_only && lf_only[g]) {  // the moment channel_status leaves Zero
      lf_only[g] = 0;
      n_lf_only--;
    }
  }
  // what the planner needs of the epoch whose descriptors / wide values have been moved to upload / wide_upload
  EpochInputs inputs(bool expand_sparse, bool want_strip) const {
    EpochInputs in{groups, upload.size(), wide_upload.size(), expand_sparse, want_strip, live};
    for (const SparseGroup& d : upload) in.groups[d.group].entries += (uint64_t)d.n[0] + d.n[1] + d.n[2];
    for (const WideValue& w : wide_upload) in.groups[w.pos / kEpochGroupCoeffs].wide = true;  // (validated at submission)
    return in;
  }
};

}  // namespace jxlh
