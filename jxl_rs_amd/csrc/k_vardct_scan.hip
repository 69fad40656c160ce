// K1, the binning: varblock sizes and positions are data dependent, so the work of a K1 launch is first binned.
//
//   k1_scan   one 256-thread quarter of a workgroup per 256x256 group: loads the group's 32x32 transform map,
//             prefix-scans the varblock sizes in raster order -> coefficient offset of every varblock (the reference lays
//             varblocks back to back in decode order, group.rs:440, :612) and appends one 16-byte work item per varblock
//             to a frame-wide list per transform class (k_vardct_common.h: WorkItem, WorkLists).
//
// Behind the kernel: the layout of the work-list memory the lists live in, and its counters.
#include "k_vardct_common.h"

namespace jxlh {
namespace {

// ------------------------------------------------------------------------------------------
// One workgroup scans kScanGroups groups (one 256-thread quarter each).  Its duration is the serial head of K1 and is
// one latency chain -- map bytes -> two block scans -> a returning global atomic per class -> item stores -- so (round 3)
// every global input is requested up front, the type tables are register immediates, two classes share a 32-bit scan
// word, and the quarters pool their counts: 256 workgroups' atomics meet on a class counter instead of 1024 (same-
// address atomics serialise at ~12 ns each: 13 of the former 36 us).
// STRIP (the frame runs through k123_strip, k_strip.hip): the scan also decides per 64x64 tile who reconstructs it -- the
// strip kernel, iff every varblock touching the tile lies inside one 32x32 quadrant of it and is a DCT with sides <= 32
// (what aligning every varblock to its own size gives) -- writes a descriptor
// per block of those tiles ({type | dx << 5 | dy << 7 | off64 << 9 | 1 << 31, raw_quant of the varblock}: everything the
// strip kernel needs to find a block's varblock and its coefficients) and appends work items for the OTHER tiles only.
// ENT (the frame is read in the slot-bucketed form, FrameDev::se_*): the scan also turns the group's slot counts into
// the entry range of every varblock -- an exclusive prefix sum over the 1024 slots of each channel (a thread loads the
// counts of four slots as one word, the three channels ride one 64-bit block scan, 17 bits each), kept in LDS and read
// at the varblock's first slot -- and writes it beside the work item: the class kernels then go from the item straight
// to the entries.  This replaces the unpack pass of round 4 (pair words + 4-byte slot tables: 69 + 12.6 MB written and
// read again per 8K frame).
// ROUTE (ENT only): some groups of the frame are read from their dense slabs (FrameDev::group_route): their DCT-class
// varblocks go to WorkLists::ditems.  A frame without routed groups runs the instantiation without any of it.
template <bool STRIP, bool ENT = false, bool ROUTE = false>
__global__ __launch_bounds__(kScanThreads) void k1_scan(const FrameDev f, const WorkLists wl, const int group_row0,
                                                         int* __restrict__ error_flag,
                                                         const int* __restrict__ group_list, const int ngroups,
                                                         int* __restrict__ next_counts) {
  constexpr int kPairs = (kNumClasses + 1) / 2;
  __shared__ int s_wave_sum[kScanGroups][kWaves];
  __shared__ uint32_t s_wcls[kScanGroups][kWaves][kPairs];
  __shared__ int s_count[kScanGroups][kNumClasses], s_base[kScanGroups][kNumClasses];
  __shared__ int s_route[ROUTE ? kScanGroups : 1];  // != 0 = the quarter's group is read from its dense slab (FrameDev::group_route)
  __shared__ int s_tmode[kScanGroups][16];  // STRIP: != 0 = a tile of the group (4 x 4 of them) the class kernels keep
  // ENT: exclusive prefix of the slot counts, three channels packed (17 bits each; a run holds at most 65536 entries)
  __shared__ uint64_t s_pref[ENT ? kScanGroups : 1][ENT ? kSlotsPerRun + 1 : 1];
  __shared__ uint64_t s_wpref[ENT ? kScanGroups : 1][kWaves];
  if constexpr (STRIP) {
    if (threadIdx.x < kScanGroups * 16) s_tmode[threadIdx.x / 16][threadIdx.x % 16] = 0;
    // progress flags + ticket counter of the strip kernel that follows
    if (blockIdx.x == 0)
      for (int i = threadIdx.x; i < f.strip_nflags; i += kScanThreads) f.strip_flags[i] = 0;
    __syncthreads();
  }
  // the counters of the NEXT launch (the other set: its last readers finished before this kernel started)
  if (blockIdx.x == 0 && threadIdx.x < kCountLines) next_counts[threadIdx.x * kCountPitch] = 0;
  const int sub = threadIdx.x / kThreads, tid = threadIdx.x % kThreads, lane = tid & 63, wave = tid >> 6;
  const int gi = blockIdx.x * kScanGroups + sub;
  const bool live = gi < ngroups;  // a dead quarter walks through the barriers with an empty group
  const int group = !live ? 0 : group_list ? group_list[gi] : group_row0 * f.xgroups + gi;
  const int bx0 = (group % f.xgroups) * kGroupBlocks, by0 = (group / f.xgroups) * kGroupBlocks;
  const int bw = live ? min(kGroupBlocks, f.xblocks - bx0) : 0, bh = live ? min(kGroupBlocks, f.yblocks - by0) : 0;
  // 4 consecutive blocks of the 32x32 raster per thread
  int sizes[4], types[4], rq4[4], local = 0;
  const int by = tid >> 3, bx4 = (tid & 7) * 4;
  const int gby = min(by0 + by, f.yblocks - 1);
  uint8_t raw4[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const size_t at = (size_t)gby * f.xblocks + min(bx0 + bx4 + i, f.xblocks - 1);
    raw4[i] = f.transform_map[at];
    rq4[i] = f.raw_quant[at];
  }
  // the four blocks of a thread share one colour tile (8 blocks wide, bx4 % 4 == 0)
  const int ci = (gby / kColorTileBlocks) * f.cmap_stride + min(bx0 + bx4, f.xblocks - 1) / kColorTileBlocks;
  const uint32_t cc = (uint32_t)(uint8_t)f.ytox[ci] | (uint32_t)(uint8_t)f.ytob[ci] << 8;
  // ENT: counts of slots 4 tid .. 4 tid + 3 of the three channels, {first entry, entries} of the three runs
  uint32_t cw[3] = {0u, 0u, 0u};
  uint2 run[3] = {make_uint2(0u, 0u), make_uint2(0u, 0u), make_uint2(0u, 0u)};
  bool dense_route = false;
  if constexpr (ENT) {
    if constexpr (ROUTE) {
      dense_route = live && f.group_route[group] != 0;
      if (tid == 0) s_route[sub] = dense_route ? 1 : 0;  // (published by the barriers below)
    }
    if (live && !dense_route) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        cw[c] = *reinterpret_cast<const uint32_t*>(f.se_counts + ((size_t)group * 3 + c) * kSlotsPerRun + 4 * tid);
        run[c] = f.se_runs[group * 3 + c];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int bx = bx4 + i;
    const uint8_t raw = (bx < bw && by < bh) ? raw4[i] : 0;
    const int type = raw & 127;
    int sz = 0;
    if (raw >= 128) {  // first (top-left) block of a varblock, group.rs:468-473
      if (type < JXLH_NUM_TRANSFORMS) {
        const int cx = 1 << log2_covered_x_reg(type), cy = 1 << log2_covered_y_reg(type);
        sz = cx * cy;
        // Error::InvalidBlockSizeForChromaSubsampling (frame/modular/mod.rs:1058-1060)
        if (f.subsampled && sz > 1) atomicExch(error_flag, JXLH_ERR_INVALID_BLOCK_SIZE);
        // Error::HFBlockOutOfBounds (frame/modular/mod.rs:1061-1064): the varblock must end inside its group
        // and inside the frame.  Such an item is dropped: its pixel stores would leave the plane.
        if (bx + cx > bw || by + cy > bh) {
          atomicExch(error_flag, JXLH_ERR_BLOCK_OUT_OF_BOUNDS);
          sz = 0;
        }
        if constexpr (STRIP) {
          // tiles this varblock keeps away from the strip kernel: all it touches if it is not a small DCT or leaves
          // its tile; every tile of the group if the map is broken
          const bool closed = (bx & 3) + cx <= 4 && (by & 3) + cy <= 4 && class_of_type_reg(type) < kClsSpecial;
          if (sz == 0 || f.subsampled) {
            for (int k = 0; k < 16; k++) atomicOr(&s_tmode[sub][k], 1);
          } else if (!closed) {
            for (int ty = by >> 3; ty <= (by + cy - 1) >> 3; ty++)
              for (int tx = bx >> 3; tx <= (bx + cx - 1) >> 3; tx++) atomicOr(&s_tmode[sub][ty * 4 + tx], 1);
          }
        }
      } else {
        atomicExch(error_flag, JXLH_ERR_INVALID_TRANSFORM);  // Error::InvalidVarDCTTransform
        if constexpr (STRIP)
          for (int k = 0; k < 16; k++) atomicOr(&s_tmode[sub][k], 1);
      }
    }
    sizes[i] = sz;
    types[i] = type;
    local += sz;
  }
  // coefficient offsets (in 64-coefficient slots): prefix sum of the covered areas in raster order (group.rs:612)
  int incl = local;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int n = __shfl_up(incl, d, 64);
    if (lane >= d) incl += n;
  }
  if (lane == 63) s_wave_sum[sub][wave] = incl;
  uint64_t pmine = 0, pincl = 0;
  if constexpr (ENT) {
    auto bytes = [](uint32_t w) { return (uint64_t)((w & 0xffu) + ((w >> 8) & 0xffu) + ((w >> 16) & 0xffu) + (w >> 24)); };
    pmine = bytes(cw[0]) | bytes(cw[1]) << 17 | bytes(cw[2]) << 34;
    pincl = pmine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)pincl, d, 64), hi = (uint32_t)__shfl_up((int)(uint32_t)(pincl >> 32), d, 64);
      if (lane >= d) pincl += (uint64_t)lo | (uint64_t)hi << 32;
    }
    if (lane == 63) s_wpref[sub][wave] = pincl;
  }
  // per-class rank of every varblock in raster order (stable: neighbouring blocks stay neighbours in the lists ->
  // contiguous coefficient reads, full-line pixel writes).  Two classes share a 32-bit word, 16 bits each (a group
  // holds at most 1024 varblocks).
  int slot[4], cls4[4];
  bool strip_tile = false;  // the thread's four blocks share a tile
  if constexpr (STRIP) {
    __syncthreads();
    strip_tile = s_tmode[sub][(by >> 3) * 4 + (bx4 >> 3)] == 0;
  }
  uint32_t mine[kPairs], excl[kPairs];
#pragma unroll
  for (int w = 0; w < kPairs; w++) mine[w] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int cls = sizes[i] > 0 && !strip_tile ? class_of_type_reg(types[i]) : -1;
    cls4[i] = cls;
    slot[i] = 0;
    const int sh = (cls & 1) * 16;
#pragma unroll
    for (int w = 0; w < kPairs; w++) {
      if ((cls >> 1) == w) {  // cls = -1 matches no pair
        slot[i] = (int)((mine[w] >> sh) & 0xffffu);
        mine[w] += 1u << sh;
      }
    }
  }
#pragma unroll
  for (int w = 0; w < kPairs; w++) {
    uint32_t inc = mine[w];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t n = (uint32_t)__shfl_up((int)inc, d, 64);
      if (lane >= d) inc += n;
    }
    excl[w] = inc - mine[w];
    if (lane == 63) s_wcls[sub][wave][w] = inc;
  }
  __syncthreads();
  if constexpr (ENT) {
    uint64_t base = pincl - pmine;
#pragma unroll
    for (int v = 0; v < kWaves; v++)
      if (v < wave) base += s_wpref[sub][v];
    uint64_t* P = s_pref[sub] + 4 * tid;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      P[k] = base;
      base += (uint64_t)((cw[0] >> (8 * k)) & 0xffu) | (uint64_t)((cw[1] >> (8 * k)) & 0xffu) << 17 |
              (uint64_t)((cw[2] >> (8 * k)) & 0xffu) << 34;
    }
    if (tid == kThreads - 1) P[4] = base;  // the run's total (entry kSlotsPerRun)
  }
  int off64 = incl - local;
  int group_total = 0;
#pragma unroll
  for (int v = 0; v < kWaves; v++) {
    if (v < wave) off64 += s_wave_sum[sub][v];
    group_total += s_wave_sum[sub][v];
  }
  // first-block flags that claim more blocks than the group holds (overlapping varblocks; the reference cannot
  // produce such a map, a caller-built one can): the 10-bit coefficient offset of the work items would overflow,
  // K1 would read past the group's slab and the class lists (sized by area) could overflow.  Nothing of such a
  // group is reconstructed.
  const bool bad_group = group_total > bw * bh;
  if (bad_group && tid == 0) atomicExch(error_flag, JXLH_ERR_BLOCK_OUT_OF_BOUNDS);
#pragma unroll
  for (int w = 0; w < kPairs; w++) {
    uint32_t woff = 0, total = 0;
#pragma unroll
    for (int v = 0; v < kWaves; v++) {
      if (v < wave) woff += s_wcls[sub][v][w];
      total += s_wcls[sub][v][w];
    }
    excl[w] += woff;
    if ((tid >> 1) == w && tid < kNumClasses)
      s_count[sub][tid] = bad_group ? 0 : (int)((total >> ((tid & 1) * 16)) & 0xffffu);
  }
  __syncthreads();
  // one atomic per class for the whole workgroup; the quarters take consecutive ranges in group order.  ENT: the DCT
  // classes of a dense-route quarter count into the dense lists (threads 32 .. 32 + kClsSpecial) instead
  if (threadIdx.x < kNumClasses || (ROUTE && threadIdx.x >= 32 && threadIdx.x < 32 + kClsSpecial)) {
    const bool dlist = ROUTE && threadIdx.x >= 32;
    const int c = dlist ? threadIdx.x - 32 : threadIdx.x;
    auto mine_q = [&](int q) {
      if constexpr (ROUTE) return c >= kClsSpecial || (s_route[q] != 0) == dlist;
      else return true;
    };
    int total = 0;
#pragma unroll
    for (int q = 0; q < kScanGroups; q++) total += mine_q(q) ? s_count[q][c] : 0;
    int base = total > 0 ? atomicAdd(&wl.counts[(dlist ? kCntDense0 + c : c) * kCountPitch], total) : 0;
#pragma unroll
    for (int q = 0; q < kScanGroups; q++) {
      if (mine_q(q)) {
        s_base[q][c] = base;
        base += s_count[q][c];
      }
    }
  }
  // (a dense-route group's slab is already there: nothing to expand for its special / large varblocks)
  if (live && tid == 0 && f.group_dense)
    f.group_dense[group] = !dense_route && (s_count[sub][kClsSpecial] | s_count[sub][kClsLarge]) != 0;
  if constexpr (STRIP) {
    if (live && tid < 16) {
      const int gtx = (group % f.xgroups) * 4 + (tid & 3), gty = (group / f.xgroups) * 4 + (tid >> 2);
      if (gtx < f.strips && gty < f.tile_rows) f.strip_mode[gty * f.strips + gtx] = (bad_group || s_tmode[sub][tid]) ? 1 : 0;
    }
  }
  __syncthreads();
  if (bad_group) return;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (sizes[i] > 0) {
      WorkItem it;
      it.packed = (uint32_t)(bx4 + i) | ((uint32_t)by << 5) | ((uint32_t)off64 << 10) | ((uint32_t)types[i] << 20);
      it.group = (uint32_t)group;
      it.raw_quant = rq4[i];
      it.cc = cc;
      const int cls = cls4[i];
      if (cls >= 0) {
        const int sh = (cls & 1) * 16;
        int rank = slot[i];
#pragma unroll
        for (int w = 0; w < kPairs; w++)
          if ((cls >> 1) == w) rank += (int)((excl[w] >> sh) & 0xffffu);
        bool to_dense = false;
        if constexpr (ENT) {
          if (cls < kClsSpecial) {
            if (dense_route) {
              to_dense = true;
              wl.ditems[cls][s_base[sub][cls] + rank] = it;
            } else {
              // (the prefixes were published by the barriers above.)  A count table that claims more than its run holds
              // is cut at the run's end: no entry outside the run is ever read.  A DCT-class varblock has at most 16
              // slots of at most 255 entries: the counts fit their 16 bits
              const uint64_t p0 = s_pref[sub][off64], p1 = s_pref[sub][min(off64 + sizes[i], kSlotsPerRun)];
              EntryItem ei;
              uint32_t n[3];
#pragma unroll
              for (int c = 0; c < 3; c++) {
                const uint32_t a0 = min((uint32_t)(p0 >> (17 * c)) & 0x1ffffu, run[c].y);
                const uint32_t a1 = min((uint32_t)(p1 >> (17 * c)) & 0x1ffffu, run[c].y);
                ei.e0[c] = run[c].x + a0;
                n[c] = min(a1 - a0, 0xffffu);
              }
              ei.nxy = n[0] | n[1] << 16;
              it.group |= n[2] << 16;
              wl.eitems[cls][s_base[sub][cls] + rank] = ei;
            }
          }
        }
        if (!to_dense) wl.items[cls][s_base[sub][cls] + rank] = it;
      }
      if constexpr (STRIP) {
        if (strip_tile) {
          const int cx = 1 << log2_covered_x_reg(types[i]), cy = 1 << log2_covered_y_reg(types[i]);
          const uint32_t d0 = (uint32_t)types[i] | ((uint32_t)off64 << 9) | (1u << 31);
          for (int dy = 0; dy < cy; dy++)
            for (int dx = 0; dx < cx; dx++)
              f.strip_desc[(size_t)(by0 + by + dy) * f.xblocks + bx0 + bx4 + i + dx] =
                  make_uint2(d0 | ((uint32_t)dx << 5) | ((uint32_t)dy << 7), (uint32_t)rq4[i]);
        }
      }
    }
    off64 += sizes[i];
  }
}

}  // namespace

void launch_k1_scan(hipStream_t s, const K1Step& step, const FrameDev& f, const WorkLists& wl, int group_row0,
                    int* error_flag, const int* group_list, int ngroups, int* next_counts) {
  const dim3 grid(step.grid), block(step.block);
  switch (step.kernel) {
    case kK1ScanStrip:
      hipLaunchKernelGGL(k1_scan<true>, grid, block, 0, s, f, wl, group_row0, error_flag, group_list, ngroups, next_counts);
      break;
    case kK1ScanEntriesRoute:
      hipLaunchKernelGGL((k1_scan<false, true, true>), grid, block, 0, s, f, wl, group_row0, error_flag, group_list, ngroups,
                         next_counts);
      break;
    case kK1ScanEntries:
      hipLaunchKernelGGL((k1_scan<false, true>), grid, block, 0, s, f, wl, group_row0, error_flag, group_list, ngroups,
                         next_counts);
      break;
    default:
      hipLaunchKernelGGL(k1_scan<false>, grid, block, 0, s, f, wl, group_row0, error_flag, group_list, ngroups, next_counts);
      break;
  }
}

// ---- the work-list memory ------------------------------------------------------------------
static_assert(kWlEItems0 - kWlItems0 == kNumClasses && kWlDItems0 - kWlEItems0 == kClsSpecial &&
              kWlFallback0 - kWlDItems0 == kClsSpecial && kWlFbAny - kWlFallback0 == kClsSpecial, "work-list regions");

WorklistLayout vardct_worklist_layout(size_t nblocks) {
  WorklistLayout L{};
  size_t p = 0;
  auto put = [&](int r, size_t len) {
    L.off[r] = p;
    L.len[r] = len;
    p += len;
  };
  put(kWlCounts, 2 * kCountBytes);  // two sets of counters, one 128-byte line each
  for (int c = 0; c < kNumClasses; c++) put(kWlItems0 + c, (nblocks / class_min_area(c) + 1) * sizeof(WorkItem));
  // entry side items of the DCT classes + their dense-route lists
  for (int c = 0; c < kClsSpecial; c++) put(kWlEItems0 + c, (nblocks / class_min_area(c) + 1) * sizeof(EntryItem));
  for (int c = 0; c < kClsSpecial; c++) put(kWlDItems0 + c, (nblocks / class_min_area(c) + 1) * sizeof(WorkItem));
  // the fallback flags: one word per batch of the class (at least 2 varblocks per batch)
  for (int c = 0; c < kClsSpecial; c++) put(kWlFallback0 + c, (nblocks / (2 * class_min_area(c)) + 16) * sizeof(uint32_t));
  put(kWlFbAny, (size_t)kFbAny * kFbAnyPitch * sizeof(uint32_t));  // the fallback launch's summary words
  // the unit lists of the large transforms: one u32 per 4096 samples of a 256-pixel varblock (two-pass units) and one
  // per varblock of the smaller types (three lists by slabs per channel; worst case one entry per 32 blocks)
  put(kWlLargeUnits, k1_large_carve(nblocks).capacity * sizeof(uint32_t));
  // the LLF planes of the large transforms (3 x nblocks floats, k1_large_llf): launch_k1_large aligns their pointer
  // to 64 bytes, which is this offset on a hipMalloc'ed (256-byte aligned) base
  p = (p + 63) & ~(size_t)63;
  put(kWlLlf, 3 * nblocks * sizeof(float));
  L.bytes = p;
  return L;
}

size_t vardct_worklist_bytes(const FrameDev& f) {
  return vardct_worklist_layout((size_t)f.xblocks * f.yblocks).bytes;
}

void vardct_worklist_clear_flags(hipStream_t s, void* worklist_mem, size_t nblocks) {
  const WorklistLayout L = vardct_worklist_layout(nblocks);
  (void)hipMemsetAsync(reinterpret_cast<char*>(worklist_mem) + L.off[kWlFallback0], 0,
                       L.off[kWlFbAny] + L.len[kWlFbAny] - L.off[kWlFallback0], s);
}

void vardct_worklist_reset(hipStream_t s, void* worklist_mem, uint32_t* launch_parity) {
  (void)hipMemsetAsync(worklist_mem, 0, 2 * kCountBytes, s);
  *launch_parity = 0;
}

const void* vardct_worklist_counters(const void* worklist_mem, uint32_t launch, size_t* bytes, int* lines) {
  static_assert(kCntFallback0 == kNumClasses + 4 && kCntDense0 == kCntFallback0 + kClsSpecial && kNumClasses == 11,
                "jxlh_frame_k1_counters maps the lines by position");
  *bytes = kCountBytes;
  *lines = kCountLines;
  return reinterpret_cast<const char*>(worklist_mem) + (launch & 1u) * kCountBytes;
}

}  // namespace jxlh
