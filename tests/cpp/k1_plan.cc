// K1's launch planner (jxl_rs_amd/csrc/k1_plan.h) against the decision code it replaced: the bottom of
// launch_vardct_groups (k_vardct.hip) and launch_vardct_large (k_vardct_large.hip), transcribed below as they were --
// their expressions and their own constants, none of them from the header -- with every launch turned into a
// (kernel id, grid, block, list set) record.  Plus the invariants of a plan.  Host only, no device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../jxl_rs_amd/csrc/k1_plan.h"

namespace {

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

struct Rec {
  int kernel, grid, block, lists;
  bool operator==(const Rec& o) const { return kernel == o.kernel && grid == o.grid && block == o.block && lists == o.lists; }
};

// ---- the old code's world: its constants, what it read of FrameDev, and a launch macro that records
namespace old {
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kScanGroups = 4;
constexpr int kScanThreads = kScanGroups * kThreads;
constexpr int kGroupBlocks = 32;
constexpr int kSpecWaves = 2;
constexpr int kSpecThreads = kSpecWaves * 64;
constexpr int kSpecChunk = 512;
constexpr int kLargeThreads = 256;
constexpr int kLargeWaves = kLargeThreads / 64;
constexpr int kLlfGrid = 1024;  // JXLH_LLF_GRID
struct S8x8 { static constexpr int NB = 8; };  // Shape<8, 8>: NB = 64 / min(R, C)
struct dim3 {
  unsigned x;
  dim3(unsigned v) : x(v) {}
  dim3(int v) : x((unsigned)v) {}
};
struct FrameDev {
  const void *strip_desc, *se_entries, *group_route, *sp_sorted;
  int se_direct_ok, subsampled, se_dense_hint, strip_all_closed, xgroups, ygroups;
};
// the instantiations by name: k1_scan<STRIP, ENT, ROUTE>, k1_dct8<SPARSE, SUB, INLINE>, k1_dct16_32<SPARSE, FB, ALL>,
// k1_special<BIN0, BIN1>
constexpr int scan_f = 0, scan_ft = 1, scan_ftt = 2, scan_t = 3, expand_entries = 4, expand_sorted = 5,  //
    dct8_0 = 6, dct8_1 = 7, dct8_2 = 8, dct8_3 = 9, dct8_3_f_t = 10, dct8_0_t = 11, dct8_1_t = 12, dct8_2_t = 13, dct8_3_t_t = 14,
              dct1632_0 = 15, dct1632_1 = 16, dct1632_2 = 17, dct1632_3 = 18, dct1632_2_t = 19, dct1632_0_f_t = 20,  //
    special_0_5 = 21, special_5_9 = 22, large_units = 23, large_llf = 24, large_fused = 25, large_pass1 = 26, large_pass2 = 27,
              n_kernels = 28;
std::vector<Rec>* g_out;
void LAUNCH(int kernel, dim3 grid, dim3 block, int lists = 0) { g_out->push_back({kernel, (int)grid.x, (int)block.x, lists}); }

// k_vardct_large.hip: launch_vardct_large (the launches; `fuse` was a function-local static read from JXLH_LARGE_FUSED)
void launch_vardct_large(int nblk, const char* env_large_fused) {
  auto grid_for = [](long work_items, int items_per_wg, int cap) {
    long g = (work_items + items_per_wg - 1) / items_per_wg;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
  };
  const int fuse = [&] {
    const char* e = env_large_fused;
    return e ? atoi(e) : 1;
  }();
  LAUNCH(large_units, dim3(grid_for(nblk / 64 + 1, 256, 64)), dim3(256));
  LAUNCH(large_llf, dim3(grid_for(3L * (nblk / 32 + 1), kLargeWaves, kLlfGrid)), dim3(kLargeThreads));
  const dim3 glarge(grid_for(3L * (nblk / 32 + 1), kLargeWaves, 512));
  if (fuse) LAUNCH(large_fused, glarge, dim3(kLargeThreads));
  LAUNCH(large_pass1, glarge, dim3(kLargeThreads));
  LAUNCH(large_pass2, glarge, dim3(kLargeThreads));
}
// k_vardct_large.hip: the unit lists behind each other; k_vardct.hip: large_unit_capacity
void large_lists(size_t nblocks, size_t off[4], size_t* capacity) {
  const size_t nb = nblocks;
  off[0] = 0;
  off[1] = off[0] + (nb / 32 + 16);
  off[2] = off[1] + (nb / 32 + 16);
  off[3] = off[2] + (nb / 128 + 16);
  *capacity = nblocks / 8 + 64;
}

// k_vardct.hip: launch_vardct_groups from `const int ngroups` on, without the epoch and the carving of the lists
void launch_vardct_groups(const FrameDev& f, int group_row0, int group_row1, const void* dense_coeffs, const void* group_list,
                          int n_list, bool has_special, bool has_large, int n_dense_route, const char* env_inline,
                          const char* env_dense1632, const char* env_large_fused) {
  const int ngroups = group_list ? n_list : (group_row1 - group_row0) * f.xgroups;
  if (ngroups <= 0) return;
  const dim3 gscan((ngroups + kScanGroups - 1) / kScanGroups);
  if (f.strip_desc)
    LAUNCH(scan_t, gscan, dim3(kScanThreads));
  else if (f.se_entries && f.group_route)
    LAUNCH(scan_ftt, gscan, dim3(kScanThreads));
  else if (f.se_entries)
    LAUNCH(scan_ft, gscan, dim3(kScanThreads));
  else
    LAUNCH(scan_f, gscan, dim3(kScanThreads));
  if (f.strip_desc && f.strip_all_closed) return;
  const int nblk = ngroups * kGroupBlocks * kGroupBlocks;
  auto grid_for = [](long work_items, int items_per_wg, int cap) {
    long g = (work_items + items_per_wg - 1) / items_per_wg;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
  };
  const int sparse = f.se_entries ? (f.se_direct_ok ? 3 : 2) : f.sp_sorted ? 1 : 0;
  if (sparse && dense_coeffs && (has_special || has_large)) {
    if (sparse >= 2)
      LAUNCH(expand_entries, dim3(f.xgroups * f.ygroups), dim3(0));
    else
      LAUNCH(expand_sorted, dim3(f.xgroups * f.ygroups), dim3(0));
  }
  const dim3 g8(grid_for(nblk, kWaves * S8x8::NB * 2, 4096)), g16(grid_for(nblk / 2, kWaves * 8 * 2, 2048)),
      g32(grid_for(nblk / 4, kWaves * 4 * 2, 2048));
  bool inline8 = false, dense1632 = false;
  if (f.subsampled) {
    if (sparse == 3) LAUNCH(dct8_3_t_t, g8, dim3(kThreads));
    else if (sparse == 2) LAUNCH(dct8_2_t, g8, dim3(kThreads));
    else if (sparse == 1) LAUNCH(dct8_1_t, g8, dim3(kThreads));
    else LAUNCH(dct8_0_t, g8, dim3(kThreads));
  } else {
    const dim3 g1632(std::min(4096u, g16.x + g32.x));
    if (sparse == 3) {
      const int force_inline = [&] {
        const char* e = env_inline;
        return e && *e ? atoi(e) : -1;
      }();
      const int force_dense1632 = [&] {
        const char* e = env_dense1632;
        return e && *e ? atoi(e) : -1;
      }();
      inline8 = force_inline >= 0 ? force_inline != 0 : f.se_dense_hint >= 2;
      dense1632 = force_dense1632 >= 0 ? force_dense1632 != 0 : f.se_dense_hint >= 1;
      if (inline8) LAUNCH(dct8_3_f_t, g8, dim3(kThreads));
      else LAUNCH(dct8_3, g8, dim3(kThreads));
      if (dense1632) LAUNCH(dct1632_2, g1632, dim3(kThreads));
      else LAUNCH(dct1632_3, g1632, dim3(kThreads));
    } else if (sparse == 2) {
      LAUNCH(dct8_2, g8, dim3(kThreads));
      LAUNCH(dct1632_2, g1632, dim3(kThreads));
    } else if (sparse == 1) {
      LAUNCH(dct8_1, g8, dim3(kThreads));
      LAUNCH(dct1632_1, g1632, dim3(kThreads));
    } else {
      LAUNCH(dct8_0, g8, dim3(kThreads));
      LAUNCH(dct1632_0, g1632, dim3(kThreads));
    }
  }
  if (sparse == 3 && !f.subsampled && !(inline8 && dense1632))
    LAUNCH(dct1632_2_t, dim3(std::min(512, std::max(1, nblk / 2048))), dim3(kThreads));
  if (sparse >= 2 && n_dense_route > 0) {
    // (wd: the ditems lists and the kCntDense0 counters; fd: se_entries cleared) -> list set 1
    const long dblk = (long)std::min(n_dense_route, ngroups) * kGroupBlocks * kGroupBlocks;
    const dim3 d8(grid_for(dblk, kWaves * S8x8::NB * 2, 4096));
    if (f.subsampled) {
      LAUNCH(dct8_0_t, d8, dim3(kThreads), 1);
    } else {
      LAUNCH(dct1632_0_f_t, dim3(std::min(8192u, d8.x + (unsigned)grid_for(dblk / 2, kWaves * 8 * 2, 4096))),
             dim3(kThreads), 1);
    }
  }
  if (has_special)
  {
    LAUNCH(special_0_5, dim3(grid_for((long)(nblk / kSpecChunk + 1) * 5, kSpecWaves, 2048)),
           dim3(kSpecThreads));
    LAUNCH(special_5_9, dim3(grid_for((long)(nblk / kSpecChunk + 1) * 4, kSpecWaves, 2048)),
           dim3(kSpecThreads));
  }
  if (has_large) launch_vardct_large(nblk, env_large_fused);
}
}  // namespace old

using namespace jxlh;
static_assert(kK1ScanPlain == old::scan_f && kK1ScanEntries == old::scan_ft && kK1ScanEntriesRoute == old::scan_ftt &&
                  kK1ScanStrip == old::scan_t && kK1ExpandEntries == old::expand_entries && kK1ExpandSorted == old::expand_sorted &&
                  kK1Dct8Dense == old::dct8_0 && kK1Dct8Sorted == old::dct8_1 && kK1Dct8Entries == old::dct8_2 &&
                  kK1Dct8Direct == old::dct8_3 && kK1Dct8DirectInline == old::dct8_3_f_t && kK1Dct8DenseSub == old::dct8_0_t &&
                  kK1Dct8SortedSub == old::dct8_1_t && kK1Dct8EntriesSub == old::dct8_2_t && kK1Dct8DirectSub == old::dct8_3_t_t &&
                  kK1Dct1632Dense == old::dct1632_0 && kK1Dct1632Sorted == old::dct1632_1 && kK1Dct1632Entries == old::dct1632_2 &&
                  kK1Dct1632Direct == old::dct1632_3 && kK1Dct1632Fallback == old::dct1632_2_t &&
                  kK1Dct1632DenseAll == old::dct1632_0_f_t && kK1SpecialLow == old::special_0_5 && kK1SpecialAfv == old::special_5_9 &&
                  kK1LargeUnits == old::large_units && kK1LargeLlf == old::large_llf && kK1LargeFused == old::large_fused &&
                  kK1LargePass1 == old::large_pass1 && kK1LargePass2 == old::large_pass2 && kK1NumKernels == old::n_kernels,
              "the kernels by number");
static_assert(kFormDense == 0 && kFormSorted == 1 && kFormEntries == 2 && kFormDirect == 3, "the forms by the old `sparse`");

// the cap a kernel's grid must respect (0: the expansion steps, whose launcher sizes them)
int cap_of(int k, int lists) {
  if (k < kK1ExpandEntries) return (10922 + 3) / 4;  // a frame has at most 10922 groups
  if (k < kK1Class0) return 0;
  if (lists == kK1DenseRouteLists) return k == kK1Dct8DenseSub ? 4096 : 8192;
  if (k < kK1Dct1632Dense) return 4096;
  if (k == kK1Dct1632Fallback) return 512;
  if (k < kK1SpecialLow) return 4096;
  if (k < kK1LargeUnits) return 2048;
  if (k == kK1LargeUnits) return 64;
  if (k == kK1LargeLlf) return JXLH_LLF_GRID;
  return 512;
}

const char* env_of(int v) { return v < 0 ? nullptr : v == 0 ? "0" : "1"; }
int count_of(const K1Plan& P, int k0, int k1, int lists = -1) {
  int n = 0;
  for (int i = 0; i < P.n; i++) n += P.step[i].kernel >= k0 && P.step[i].kernel < k1 && (lists < 0 || P.step[i].lists == lists);
  return n;
}

long g_plans = 0;
void one(const K1Inputs& in, bool listed) {
  // ---- the old code on the same launch
  old::FrameDev f{};
  static const int dummy = 0;
  f.strip_desc = in.strip ? &dummy : nullptr;
  f.se_entries = in.form >= kFormEntries ? &dummy : nullptr;
  f.se_direct_ok = in.form == kFormDirect;
  f.sp_sorted = in.form == kFormSorted ? &dummy : nullptr;
  f.group_route = in.group_route ? &dummy : nullptr;
  f.subsampled = in.subsampled;
  f.se_dense_hint = in.se_dense_hint;
  f.strip_all_closed = in.strip_all_closed;
  // rows: ngroups as rows x xgroups (two rows when it is even); the frame's other groups lie above and below
  const int rows = in.ngroups % 2 == 0 ? 2 : 1;
  f.xgroups = listed ? 7 : in.ngroups / rows;
  f.ygroups = listed ? (in.ngroups + 6) / 7 + 1 : rows + 4;
  K1Inputs q = in;
  q.frame_groups = f.xgroups * f.ygroups;
  q.ngroups = k1_ngroups(listed, in.ngroups, 3, 3 + rows, f.xgroups);
  static std::vector<Rec> want;
  want.clear();
  old::g_out = &want;
  old::launch_vardct_groups(f, 3, 3 + rows, in.dense_slab ? &dummy : nullptr, listed ? &dummy : nullptr, in.ngroups, in.has_special,
                            in.has_large, in.n_dense_route, env_of(in.force_inline), env_of(in.force_dense1632),
                            env_of(in.force_large_fused));
  const K1Plan P = plan_k1(q);
  g_plans++;
  CHECK(q.ngroups == in.ngroups, "ngroups %d listed %d", in.ngroups, (int)listed);
  CHECK(P.n == (int)want.size() && P.n <= kK1MaxSteps, "steps %d != %d (ngroups %d form %d)", P.n, (int)want.size(), in.ngroups, (int)in.form);
  for (int i = 0; i < P.n && i < (int)want.size(); i++) {
    const Rec got{P.step[i].kernel, P.step[i].grid, P.step[i].block, P.step[i].lists};
    CHECK(got == want[i], "step %d: {%d, %d, %d, %d} != {%d, %d, %d, %d} (ngroups %d form %d sub %d hint %d)", i, got.kernel, got.grid,
          got.block, got.lists, want[i].kernel, want[i].grid, want[i].block, want[i].lists, in.ngroups, (int)in.form, (int)in.subsampled,
          in.se_dense_hint);
  }
  if (count_of(P, kK1LargeUnits, kK1NumKernels)) CHECK((P.large_fuse != 0) == (in.force_large_fused != 0), "fuse %d", P.large_fuse);
  // ---- invariants
  CHECK(P.n >= 1 && P.step[0].kernel < kK1ExpandEntries && count_of(P, 0, kK1ExpandEntries) == 1, "a scan is first, once");
  for (int i = 0; i < P.n; i++) {
    const int cap = cap_of(P.step[i].kernel, P.step[i].lists);
    if (cap) CHECK(P.step[i].grid >= 1 && P.step[i].grid <= cap && P.step[i].block >= 64 && P.step[i].block % 64 == 0,
                   "step %d kernel %d grid %d block %d", i, P.step[i].kernel, P.step[i].grid, P.step[i].block);
    else CHECK(P.step[i].grid == q.frame_groups && P.step[i].block == 0, "expansion over %d groups", P.step[i].grid);
  }
  if (in.strip && in.strip_all_closed) {
    CHECK(P.n == 1, "nothing follows the scan of an all-closed strip frame: %d", P.n);
    return;
  }
  const bool inline8 = in.force_inline >= 0 ? in.force_inline != 0 : in.se_dense_hint >= 2;
  const bool dense1632 = in.force_dense1632 >= 0 ? in.force_dense1632 != 0 : in.se_dense_hint >= 1;
  CHECK(count_of(P, kK1Dct1632Fallback, kK1Dct1632Fallback + 1) == (in.form == kFormDirect && !in.subsampled && !(inline8 && dense1632)),
        "the fallback launch");
  CHECK(count_of(P, kK1Class0, kK1ClassEnd, kK1DenseRouteLists) == (in.form >= kFormEntries && in.n_dense_route > 0), "dense-route steps");
  CHECK(count_of(P, 0, kK1NumKernels, kK1DenseRouteLists) == count_of(P, kK1Class0, kK1Special0, kK1DenseRouteLists), "only DCT classes are routed");
  CHECK(count_of(P, kK1SpecialLow, kK1SpecialAfv + 1) == (in.has_special ? 2 : 0), "special steps");
  CHECK(count_of(P, kK1LargeUnits, kK1NumKernels) == (in.has_large ? (in.force_large_fused == 0 ? 4 : 5) : 0), "large steps");
  CHECK(count_of(P, kK1ExpandEntries, kK1Class0) == (in.form != kFormDense && in.dense_slab && (in.has_special || in.has_large)),
        "the expansion step");
  CHECK(count_of(P, kK1Dct8Dense, kK1Dct1632Dense, kK1FrameLists) == 1, "one 8x8 launch on the frame's lists");
  CHECK(count_of(P, kK1Dct1632Dense, kK1Dct1632Fallback, kK1FrameLists) == (in.subsampled ? 0 : 1), "one 16..32 launch");
}

}  // namespace

int main() {
  // group counts: 1 .. beyond every cap (8x8: 256; 16..32: 256; fallback: 1024; routed: 512; special: ~410; large units:
  // 1024, LLF: ~43, large: ~22), the odd ones round grid_for up, and the largest frame jxlh_frame_begin admits
  const int kGroups[] = {1, 2, 3, 4, 5, 15, 16, 17, 21, 22, 42, 43, 63, 64, 65, 255, 256, 257, 409, 410, 511, 512, 513,
                         1023, 1024, 1025, 4096, 10922};
  for (int ngroups : kGroups)
    for (int form = 0; form < 4; form++)
      for (int sub = 0; sub < 2; sub++)
        for (int hint = 0; hint < 3; hint++)
          for (int ov = 0; ov < 27; ov++)
            for (int flags = 0; flags < 32; flags++)
              for (int strip = 0; strip < 3; strip++)
                for (int r = 0; r < 4; r++) {
                  K1Inputs in{};
                  in.ngroups = ngroups;
                  in.nblocks = (size_t)ngroups * 1024;
                  in.form = (K1Form)form;
                  in.subsampled = sub != 0;
                  in.se_dense_hint = hint;
                  in.force_inline = ov % 3 - 1;
                  in.force_dense1632 = ov / 3 % 3 - 1;
                  in.force_large_fused = ov / 9 - 1;
                  in.has_special = flags & 1;
                  in.has_large = (flags & 2) != 0;
                  in.dense_slab = (flags & 4) != 0;
                  in.group_route = (flags & 8) != 0;
                  const bool listed = (flags & 16) != 0;
                  in.strip = strip != 0;
                  in.strip_all_closed = strip == 2;
                  in.n_dense_route = r == 0 ? 0 : r == 1 ? 1 : r == 2 ? ngroups : ngroups + 5;
                  one(in, listed);
                }
  // the large transforms' unit lists: the plan's carve against the old offsets, and the lists fit the region
  for (size_t nb : {(size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)127, (size_t)128, (size_t)255, (size_t)256, (size_t)1089,
                    (size_t)65536, (size_t)10922 * 1024}) {
    size_t off[4], cap;
    old::large_lists(nb, off, &cap);
    const K1LargeCarve c = k1_large_carve(nb);
    CHECK(c.two_pass == off[0] && c.fused[0] == off[1] && c.fused[1] == off[2] && c.fused[2] == off[3] && c.capacity == cap,
          "carve of %zu blocks", nb);
    CHECK(c.fused[2] + (nb / 256 + 16) <= c.capacity, "the lists of %zu blocks fit their region", nb);
  }
  std::printf("%ld plans\n", g_plans);
  if (g_fail) {
    std::printf("k1 plans: %d failures\n", g_fail);
    return 1;
  }
  std::printf("k1 plans: ok\n");
  return 0;
}
