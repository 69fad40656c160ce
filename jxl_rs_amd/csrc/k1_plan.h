// The launches of one K1 call: which kernels launch_vardct_groups enqueues, in which order, with which grids and on
// which work lists -- decided here, issued by k1_launch.hip through one launcher per kernel-holding file.
// Plain C++, fixed-size arrays, no heap: host logic, tested without a device (tests/cpp/k1_plan.cc).
#pragma once
#include <stddef.h>

#ifndef JXLH_LLF_GRID
#define JXLH_LLF_GRID 1024  // four 32 KB workgroups of k1_large_llf fit a CU
#endif

namespace jxlh {

// ---- kernel geometry the grids depend on (the kernel files build on these or tie theirs to them)
constexpr int kWaves = 4;  // class kernels: wavefronts per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kScanGroups = 4;  // k1_scan: groups per workgroup, one 256-thread quarter each
constexpr int kScanThreads = kScanGroups * kThreads;
constexpr int kDct8Batch = 8;  // varblocks of a batch of the 8x8 class (S8x8::NB)
constexpr int kSpecWaves = 2;  // k1_special
constexpr int kSpecThreads = kSpecWaves * 64;
constexpr int kSpecChunk = 512;  // items of the special list a wave bins at a time
constexpr int kLargeWaves = 4;   // the 64..256 transforms: independent waves per workgroup
constexpr int kK1GroupBlocks = 32;  // 8x8 blocks per group side (kGroupBlocks)

// grid caps.  The class kernels' measured flat between 768 and 8192 workgroups at 8K (tools/bench_variants.sh)
constexpr int kCapDct8 = 4096, kCapDct16 = 2048, kCapDct32 = 2048, kCapDct1632 = 4096;
constexpr int kCapFallback = 512;
constexpr int kCapRouteDct8 = 4096, kCapRouteDct16 = 4096, kCapRouteAll = 8192;
constexpr int kCapSpecial = 2048;
constexpr int kCapLargeUnits = 64, kCapLargeLlf = JXLH_LLF_GRID;
constexpr int kCapLarge = 512;  // two 77 KiB workgroups fit a CU: 512 is the resident capacity

// The form K1 reads the frame's coefficients in (the class kernels' first template parameter)
enum K1Form : int {
  kFormDense = 0,    // dense slabs
  kFormSorted = 1,   // plain pairs, sorted by slot (FrameDev::sp_sorted)
  kFormEntries = 2,  // slot-bucketed entries (FrameDev::se_*) through the dense dequantisation pass
  kFormDirect = 3    // slot-bucketed entries, direct kernels: a zero coefficient provably reconstructs to +0.0f
};

// Every kernel instantiation K1 can launch.  [kK1Class0, kK1ClassEnd) take (FrameDev, WorkLists): k_vardct.hip and
// k_vardct_special.hip launch them from one table in this order.
enum K1Kernel : int {
  kK1ScanPlain, kK1ScanEntries, kK1ScanEntriesRoute, kK1ScanStrip,  // k1_scan<STRIP, ENT, ROUTE>
  kK1ExpandEntries, kK1ExpandSorted,  // k_coeffs.hip: dense slabs for the groups that hold special / large varblocks
  // k1_dct8<form, SUB, INLINE>
  kK1Dct8Dense, kK1Dct8Sorted, kK1Dct8Entries, kK1Dct8Direct, kK1Dct8DirectInline,
  kK1Dct8DenseSub, kK1Dct8SortedSub, kK1Dct8EntriesSub, kK1Dct8DirectSub,
  // k1_dct16_32<form, FB, ALL>
  kK1Dct1632Dense, kK1Dct1632Sorted, kK1Dct1632Entries, kK1Dct1632Direct, kK1Dct1632Fallback, kK1Dct1632DenseAll,
  kK1SpecialLow, kK1SpecialAfv,  // k1_special<0, 5>, <5, 9>
  kK1LargeUnits, kK1LargeLlf, kK1LargeFused, kK1LargePass1, kK1LargePass2,
  kK1NumKernels
};
constexpr int kK1Class0 = kK1Dct8Dense, kK1ClassEnd = kK1LargeUnits, kK1Special0 = kK1SpecialLow;

// which work lists a step runs: the frame's, or the lists of the groups routed to their dense slabs
// (WorkLists::ditems as items, the kCntDense0 counters, FrameDev::se_entries cleared)
enum K1Lists : int { kK1FrameLists, kK1DenseRouteLists };

struct K1Step {
  K1Kernel kernel;
  int grid, block;  // the expansion steps: grid = groups their launcher covers, block = 0 (k_coeffs.hip sizes them)
  K1Lists lists;
};
constexpr int kK1MaxSteps = 16;
struct K1Plan {
  int n;
  K1Step step[kK1MaxSteps];
  int large_fuse;  // k1_large_units' argument: != 0 sends the types below 256 pixels to the one-launch path
};

struct K1Inputs {
  int ngroups;       // groups of this launch (listed, or the row range): k1_ngroups
  int frame_groups;  // xgroups * ygroups
  size_t nblocks;    // 8x8 blocks of the frame
  K1Form form;
  bool subsampled;
  int se_dense_hint;  // entries form: 0 / 1 / 2 = the frame's density class (coeff_epoch.h)
  bool has_special, has_large;
  int n_dense_route;  // entries forms: groups read from their dense slabs
  bool dense_slab;    // a writable dense slab was passed (the expansion's target)
  bool group_route, strip, strip_all_closed;
  // JXLH_K1_INLINE, JXLH_K1_DENSE1632, JXLH_LARGE_FUSED as read by the caller; -1 = unset
  int force_inline, force_dense1632, force_large_fused;
};

inline int k1_ngroups(bool listed, int n_list, int group_row0, int group_row1, int xgroups) {
  return listed ? n_list : (group_row1 - group_row0) * xgroups;
}

// grids: enough waves to fill the chip; kernels stride over their lists (counts are device-side)
inline int k1_grid_for(long work_items, int items_per_wg, int cap) {
  long g = (work_items + items_per_wg - 1) / items_per_wg;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- the large transforms' unit lists behind each other in their region of the work-list memory, in u32: the two-pass
// units (nblocks / 32 + 16) and the three fused lists (/ 32, / 128, / 256, + 16 each); capacity = the region
struct K1LargeCarve { size_t two_pass, fused[3], capacity; };
inline K1LargeCarve k1_large_carve(size_t nblocks) {
  K1LargeCarve c{};
  c.two_pass = 0;
  c.fused[0] = c.two_pass + (nblocks / 32 + 16);
  c.fused[1] = c.fused[0] + (nblocks / 32 + 16);
  c.fused[2] = c.fused[1] + (nblocks / 128 + 16);
  c.capacity = nblocks / 8 + 64;
  return c;
}

// One stream: forking the class kernels onto side streams measured no gain on the d1 mix (event overhead ~ tail
// savings) and extra streams compete for the runtime's few hardware queues.  (The large transforms on a side stream
// next to the memory-bound DCT classes, one workgroup per CU: K1 of the 16K all-types frame 1.872 -> 1.847 ms, 1.937
// with their usual two per CU -- inside the noise, not kept.)
inline K1Plan plan_k1(const K1Inputs& in) {
  K1Plan P{};
  auto push = [&](K1Kernel k, int grid, int block, K1Lists lists = kK1FrameLists) { P.step[P.n++] = {k, grid, block, lists}; };
  const bool entries = in.form >= kFormEntries;
  push(in.strip ? kK1ScanStrip : entries && in.group_route ? kK1ScanEntriesRoute : entries ? kK1ScanEntries : kK1ScanPlain,
       (in.ngroups + kScanGroups - 1) / kScanGroups, kScanThreads);
  if (in.strip && in.strip_all_closed) return P;  // the host saw the whole map: no tile is left to the class kernels
  const int nblk = in.ngroups * kK1GroupBlocks * kK1GroupBlocks;
  // groups that hold special / large varblocks (flagged by k1_scan) still get a dense slab
  if (in.form != kFormDense && in.dense_slab && (in.has_special || in.has_large))
    push(entries ? kK1ExpandEntries : kK1ExpandSorted, in.frame_groups, 0);
  const int g8 = k1_grid_for(nblk, kWaves * kDct8Batch * 2, kCapDct8), g16 = k1_grid_for(nblk / 2, kWaves * 8 * 2, kCapDct16),
            g32 = k1_grid_for(nblk / 4, kWaves * 4 * 2, kCapDct32);
  bool inline8 = false, dense1632 = false;  // direct form: the dense-pass choices of a frame denser than d1 (se_dense_hint)
  if (in.subsampled) {
    // (the fallback launch has no sub-sampled form: such a frame always takes the inline fallback)
    // the other DCT classes are empty in a sub-sampled frame (k1_scan reports larger varblocks as an error)
    push((K1Kernel)(kK1Dct8DenseSub + in.form), g8, kThreads);
  } else {
    const int g1632 = g16 + g32 < kCapDct1632 ? g16 + g32 : kCapDct1632;
    if (in.form == kFormDirect) {
      // JXLH_K1_INLINE=0 / 1: A/B runs of the 8x8 class's two forms; JXLH_K1_DENSE1632: the same for the 16..32-point classes
      inline8 = in.force_inline >= 0 ? in.force_inline != 0 : in.se_dense_hint >= 2;
      dense1632 = in.force_dense1632 >= 0 ? in.force_dense1632 != 0 : in.se_dense_hint >= 1;
      push(inline8 ? kK1Dct8DirectInline : kK1Dct8Direct, g8, kThreads);
      push(dense1632 ? kK1Dct1632Entries : kK1Dct1632Direct, g1632, kThreads);
    } else {
      push((K1Kernel)(kK1Dct8Dense + in.form), g8, kThreads);
      push((K1Kernel)(kK1Dct1632Dense + in.form), g1632, kThreads);
    }
  }
  // what the direct form of k1_dct16_32 left (usually next to nothing: the workgroups read one counter and leave)
  // (a sparse frame leaves a handful of batches: the workgroups read one counter and go; a frame denser than d1 gets
  // the whole chip)
  // (the fallback as TWO launches -- the classes without a 32-point side apart: 32 KB of LDS, three waves per SIMD --
  // measured no better on the outlier frame and 4 % worse on dense ones: profiles/r06_c_density.txt)
  // (nothing can be left when both choices were made)
  if (in.form == kFormDirect && !in.subsampled && !(inline8 && dense1632)) {
    const int g = nblk / 2048 > 1 ? nblk / 2048 : 1;
    push(kK1Dct1632Fallback, g < kCapFallback ? g : kCapFallback, kThreads);
  }
  // entries form, groups routed to their dense slabs (FrameDev::group_route): the same class kernels in their dense
  // form on those groups' lists; the grids follow the routed share of the frame
  if (entries && in.n_dense_route > 0) {
    const long dblk = (long)(in.n_dense_route < in.ngroups ? in.n_dense_route : in.ngroups) * kK1GroupBlocks * kK1GroupBlocks;
    const int d8 = k1_grid_for(dblk, kWaves * kDct8Batch * 2, kCapRouteDct8);
    if (in.subsampled) {
      push(kK1Dct8DenseSub, d8, kThreads, kK1DenseRouteLists);
    } else {
      // (one launch for every DCT class of the routed groups)
      const unsigned g = (unsigned)d8 + (unsigned)k1_grid_for(dblk / 2, kWaves * 8 * 2, kCapRouteDct16);
      push(kK1Dct1632DenseAll, (int)(g < (unsigned)kCapRouteAll ? g : (unsigned)kCapRouteAll), kThreads, kK1DenseRouteLists);
    }
  }
  // an empty special list (the d1 mix) pays for every launched workgroup: the grid follows the list's worst case
  if (in.has_special) {
    push(kK1SpecialLow, k1_grid_for((long)(nblk / kSpecChunk + 1) * 5, kSpecWaves, kCapSpecial), kSpecThreads);
    push(kK1SpecialAfv, k1_grid_for((long)(nblk / kSpecChunk + 1) * 4, kSpecWaves, kCapSpecial), kSpecThreads);
  }
  // the large class: unit lists, LLF corners, the one-launch path, then one launch per separable pass of the 256-pixel
  // types.  All five exit at once when the class is empty
  if (in.has_large) {
    // development switch: JXLH_LARGE_FUSED=0 sends every large type through the two passes
    P.large_fuse = in.force_large_fused == -1 ? 1 : in.force_large_fused;
    push(kK1LargeUnits, k1_grid_for(nblk / 64 + 1, 256, kCapLargeUnits), 256);
    push(kK1LargeLlf, k1_grid_for(3L * (nblk / 32 + 1), kLargeWaves, kCapLargeLlf), kLargeWaves * 64);
    const int glarge = k1_grid_for(3L * (nblk / 32 + 1), kLargeWaves, kCapLarge);
    if (P.large_fuse) push(kK1LargeFused, glarge, kLargeWaves * 64);
    push(kK1LargePass1, glarge, kLargeWaves * 64);
    push(kK1LargePass2, glarge, kLargeWaves * 64);
  }
  return P;
}

}  // namespace jxlh
