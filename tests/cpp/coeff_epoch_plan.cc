// The coefficient-epoch planner (jxl_rs_amd/csrc/coeff_epoch.h) on a table of 4-group epochs: what the run does with
// each submission history -- resident form, routes, rebuilt / widened groups, descriptors, sort, density hint.  Host
// only, no device.
#include <cstdio>
#include <string>
#include <vector>

#include "../../jxl_rs_amd/csrc/coeff_epoch.h"

using namespace jxlh;

namespace {

struct Row {
  const char* what;
  // epoch: resident form and live routes before it, per group K(ept) D(ense) P(airs) S(lots), accumulate bits, the
  // group a wide value addresses (-1: none), entries per sparse group, JXLH_FRAME_EXPAND_SPARSE, want_strip
  Resident before;
  const char* route_before;
  const char* subs;
  const char* accum;
  int wide_group;
  uint64_t entries;
  bool expand_sparse, want_strip;
  // expected plan ("" = empty vector)
  Resident resident;
  const char* route;
  int n_route;
  const char* rebuild;
  const char* widen;
  Descs descs;
  bool sort;
  int hint;
  bool pending_read;
};

constexpr Resident kD = Resident::kDense, kSP = Resident::kSortedPairs, kE = Resident::kEntries;
constexpr uint64_t kE1 = 1000;  // entries of a d1-like group: share 0.005

const Row kRows[] = {
    {"all slots", kD, "", "SSSS", "0000", -1, kE1, false, false, kE, "", 0, "", "", Descs::kNone, false, 0, false},
    {"all slots, JXLH_FRAME_EXPAND_SPARSE", kD, "", "SSSS", "0000", -1, kE1, true, false, kD, "", 0, "", "1111",
     Descs::kAll, false, 0, true},
    {"all slots, want_strip", kD, "", "SSSS", "0000", -1, kE1, false, true, kD, "", 0, "", "1111", Descs::kAll, false, 0,
     true},
    {"3 slots + 1 dense", kD, "", "SSSD", "0000", -1, kE1, false, false, kE, "0001", 1, "", "", Descs::kRouted, false, 0,
     false},
    {"2 slots + 2 dense", kD, "", "SSDD", "0000", -1, kE1, false, false, kE, "0011", 2, "", "", Descs::kRouted, false, 0,
     false},
    {"1 slots + 3 dense", kD, "", "SDDD", "0000", -1, kE1, false, false, kD, "", 0, "", "1000", Descs::kAll, false, 0,
     true},
    {"all slots, a wide value in group 2", kD, "", "SSSS", "0000", 2, kE1, false, false, kE, "0010", 1, "", "0010",
     Descs::kRouted, false, 0, false},
    {"entries resident -> all slots, group 1 accumulates", kE, "", "SSSS", "0100", -1, kE1, false, false, kE, "0100", 1,
     "0100", "0100", Descs::kRouted, false, 0, false},
    {"all pairs", kD, "", "PPPP", "0000", -1, kE1, false, false, kSP, "", 0, "", "", Descs::kAll, true, 0, false},
    {"2 slots + 2 pairs", kD, "", "SSPP", "0000", -1, kE1, false, false, kE, "0011", 2, "", "", Descs::kRouted, false, 0,
     false},
    {"1 slots + 3 pairs", kD, "", "SPPP", "0000", -1, kE1, false, false, kSP, "", 0, "", "1000", Descs::kAll, true, 0,
     true},
    {"sorted pairs resident -> 3 pairs + group 3 kept", kSP, "", "PPPK", "0000", -1, kE1, false, false, kD, "", 0, "0001",
     "", Descs::kAll, false, 0, false},
    {"entries resident, group 3 routed -> 3 pairs + group 3 kept", kE, "0001", "PPPK", "0000", -1, kE1, false, false, kD,
     "", 0, "", "", Descs::kAll, false, 0, false},
    {"entries resident -> 3 slots + group 3 kept", kE, "", "SSSK", "0000", -1, kE1, false, false, kD, "", 0, "0001", "1110",
     Descs::kAll, false, 0, true},
    {"entries resident -> all dense", kE, "", "DDDD", "0000", -1, kE1, false, false, kD, "", 0, "", "", Descs::kAll, false,
     0, false},
    // FrameDev::se_dense_hint: entries per in-place coefficient (3 x 65536 per group) above 0.125 / 0.25
    {"share just below 0.125", kD, "", "SSSS", "0000", -1, 24575, false, false, kE, "", 0, "", "", Descs::kNone, false, 0,
     false},
    {"share just above 0.125", kD, "", "SSSS", "0000", -1, 24577, false, false, kE, "", 0, "", "", Descs::kNone, false, 1,
     false},
    {"share just below 0.25", kD, "", "SSSS", "0000", -1, 49151, false, false, kE, "", 0, "", "", Descs::kNone, false, 1,
     false},
    {"share just above 0.25", kD, "", "SSSS", "0000", -1, 49153, false, false, kE, "", 0, "", "", Descs::kNone, false, 2,
     false},
    {"share of the in-place groups only", kD, "", "SSSD", "0000", -1, 30000, false, false, kE, "0001", 1, "", "",
     Descs::kRouted, false, 1, false},
};

std::vector<uint8_t> bits(const char* s) {
  std::vector<uint8_t> v;
  for (; *s; s++) v.push_back(*s == '1' ? 1 : 0);
  return v;
}

std::string str(const std::vector<uint8_t>& v) {
  std::string s;
  for (uint8_t x : v) s += x ? '1' : '0';
  return s;
}

EpochInputs inputs(const Row& r) {
  EpochInputs in;
  for (int g = 0; r.subs[g]; g++) {
    EpochGroup e;
    const char k = r.subs[g];
    e.sub = k == 'D' ? Sub::kDense : k == 'P' ? Sub::kPairs : k == 'S' ? Sub::kSlots : Sub::kKept;
    e.accumulate = r.accum[g] == '1';
    e.wide = g == r.wide_group;
    const bool sparse = k == 'P' || k == 'S';
    e.entries = sparse ? r.entries : 0;
    in.n_desc += sparse ? 1 : 0;
    in.groups.push_back(e);
  }
  in.n_wide = r.wide_group >= 0 ? 1 : 0;
  in.expand_sparse = r.expand_sparse;
  in.want_strip = r.want_strip;
  in.before.form = r.before;
  in.before.route = bits(r.route_before);
  return in;
}

}  // namespace

int main() {
  int bad = 0;
  for (const Row& r : kRows) {
    const EpochPlan p = plan_coeff_epoch(inputs(r));
    const Residence& a = p.after;
    const bool ok = a.form == r.resident && str(a.route) == r.route && a.n_route == r.n_route &&
                    str(p.rebuild) == r.rebuild && str(p.widen) == r.widen && p.descs == r.descs && p.sort == r.sort &&
                    a.se_dense_hint == r.hint && p.pending_read == r.pending_read &&
                    p.trade_sets() == (r.resident == Resident::kEntries);
    if (!ok) {
      bad++;
      std::printf("MISMATCH %s: resident %d route '%s' (%d) rebuild '%s' widen '%s' descs %d sort %d hint %d "
                  "pending_read %d\n",
                  r.what, (int)a.form, str(a.route).c_str(), a.n_route, str(p.rebuild).c_str(), str(p.widen).c_str(),
                  (int)p.descs, (int)p.sort, a.se_dense_hint, (int)p.pending_read);
    }
  }
  if (bad) return 1;
  std::printf("coeff epoch plans: ok (%zu epochs)\n", sizeof kRows / sizeof kRows[0]);
  return 0;
}
