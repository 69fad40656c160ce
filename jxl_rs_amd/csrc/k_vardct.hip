// K1 -- dequantisation + chroma-from-luma + LLF-from-LF + variable-size IDCT for a frame.
//
// Replaces the `if let Some(pixels)` branch of decode_vardct_group
// (jxl/src/frame/group.rs:579-611): dequant_block (:137-177), dequant_lane (:100-133),
// adjust_quant_bias (:85-96), the LF patch copy (:227-235), transform_to_pixels and
// the copy into the group planes (:237-250).
//
// Varblock sizes and positions are data dependent, so the work is first *binned* (k1_scan, k_vardct_scan.hip: one
// frame-wide list of 16-byte work items per transform class).  This file holds the DCT classes with sides of 8..32:
//
//   k1_dct*   one kernel per class family, sized for that family's registers/LDS: wavefronts
//             stride over batches of same-shape varblocks; a batch's dequantised coefficients
//             are staged channel by channel in the wave's private LDS tile with 16-byte
//             coalesced loads and run through the wave-level cores of varblock_core.h.  For
//             the small shapes all three channels' loads are issued up front and the dequant
//             weights stay in registers across batches; on dense slabs every shape's batch is
//             sized to 16 coefficients per lane and channel or fewer, and all of them issue
//             the three channels' loads up front.
//
// The 8x8 special transforms are k_vardct_special.hip, the 64..256 transforms k_vardct_large.hip; which of all these
// kernels a launch enqueues is k1_plan.h, issued by k1_launch.hip.
//
// HBM traffic is the compulsory 12 B/px in + 12 B/px out (+ maps, + 32 B per varblock of
// work items); arithmetic is f32 in the reference's operation order (bit-exact vs the FMA
// build of the oracle).  Output is independent of the order in which work items land in
// the lists (each varblock is independent).
#include <type_traits>

#include "k_vardct_common.h"

// (the policy of K1's two streams: JXLH_NT_COEF, k_vardct_common.h)
#ifndef JXLH_NT_K1_STORE
#define JXLH_NT_K1_STORE true
#endif
namespace jxlh {
namespace {
template <class S>
__device__ __forceinline__ void stage4(float* __restrict__ buf, int b, int k, float4 v) {
  if constexpr (S::kWide) {
    buf[m_addr<S>(b, k)] = v.x;
    buf[m_addr<S>(b, k + 1)] = v.y;
    buf[m_addr<S>(b, k + 2)] = v.z;
    buf[m_addr<S>(b, k + 3)] = v.w;
  } else {
    *reinterpret_cast<float4*>(buf + m_addr<S>(b, k)) = v;
  }
}

// All batches of one DCT shape assigned to this wave.  PREFETCH: the dequant weights a lane needs stay in registers
// across batches, and the coefficient loads of all three channels are issued before any is touched (small shapes;
// 3*E/4 int4 in flight per lane).  Dense slabs issue the three channels' loads together without PREFETCH too, whenever
// a lane holds at most 16 coefficients per channel (generic_batch: kQPF).
// Sparse input: builds the integer coefficients of one channel of the batch in the wave's tile
// (zero, then ds_add of the varblocks' pairs: duplicates from several passes add up before
// dequantisation, like `coeffs[i] += v` in the dense slab).  64 / NB lanes per varblock walk its
// pair range; the layout is the M layout, so the dequantisation pass converts in place.
// The pair ranges of all three channels (sparse_ranges) and the first kSparsePrefetch pairs of each
// (sparse_first) are fetched when the batch starts, so the per-channel step only waits on LDS.
// (Software-pipelining this across batches -- next batch's items / ranges / pairs requested while
// the current one is transformed -- was measured slower: 216 vs 190 us for the 8x8 class at 8K.)
constexpr int kSparsePrefetch = 2;
struct SparseLane {
  uint32_t i0[3], i1[3];
  uint32_t first[3][kSparsePrefetch];
  int first_pos;
};

template <class S>
__device__ __forceinline__ void sparse_ranges(const FrameDev& f, const BlockInfo* __restrict__ binfo, int nb, int lane,
                                              SparseLane& sl) {
  constexpr int LPB = 64 / S::NB;
  const int b = lane / LPB, j = lane % LPB;
  const bool on = b < nb;
  const int base = on ? binfo[b].slot_base : 0;
  sl.first_pos = on ? binfo[b].first_pos : 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    sl.i0[c] = on ? f.sp_slot_start[base + c * kSlotTable] + j : 0u;
    sl.i1[c] = on ? f.sp_slot_start[base + c * kSlotTable + S::N / 64] : 0u;
  }
}
template <class S>
__device__ __forceinline__ void sparse_first(const FrameDev& f, SparseLane& sl) {
  constexpr int LPB = 64 / S::NB;
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int k = 0; k < kSparsePrefetch; k++) {
      const uint32_t i = sl.i0[c] + k * LPB;
      sl.first[c][k] = i < sl.i1[c] ? f.sp_sorted[i] : 0u;  // pos 0 + value 0 adds nothing
    }
}

template <class S>
__device__ __forceinline__ void sparse_stage_channel(const FrameDev& f, int ch, float* __restrict__ buf, int lane,
                                                     const SparseLane& sl) {
  int* ibuf = reinterpret_cast<int*>(buf);
  constexpr int kWords = S::NB * S::SM;
  if constexpr (kWords % 4 == 0) {
    for (int i = lane * 4; i < kWords; i += 256) *reinterpret_cast<int4*>(ibuf + i) = make_int4(0, 0, 0, 0);
  } else {
    for (int i = lane; i < kWords; i += 64) ibuf[i] = 0;
  }
  wave_sync();
  constexpr int LPB = 64 / S::NB;
  const int b = lane / LPB;
  auto add = [&](uint32_t p) {
    atomicAdd(&ibuf[m_addr<S>(b, (int)(p & 0xffffu) - sl.first_pos)], (int)(int16_t)(p >> 16));
  };
#pragma unroll
  for (int k = 0; k < kSparsePrefetch; k++)
    if (sl.i0[ch] + k * LPB < sl.i1[ch]) add(sl.first[ch][k]);
  for (uint32_t i = sl.i0[ch] + kSparsePrefetch * LPB; i < sl.i1[ch]; i += LPB) add(f.sp_sorted[i]);
  wave_sync();
}

// ---- the slot-bucketed entries read in place (SPARSE == 2).  The varblock's entry range per channel comes with the
// work item (k1_scan<ENT>), so the first entries of all three channels are requested one memory round trip after the
// item -- the pair form needs two (slot table, then pairs).  The LPB lanes of a varblock share its range evenly
// (entry r of the range goes to lane r % LPB); an entry carries only its position inside its 64-coefficient slot, so
// for varblocks of more than one slot the lane finds the slot of entry r in the exclusive prefix of the varblock's
// slot counts (one byte load per slot and channel, a segmented shuffle scan, 10 bits per channel in one LDS word per
// slot): log2(slots) LDS reads per entry.
// entries a lane holds per channel before it has to go back to memory: a varblock with at most D * LPB entries per
// channel is staged without a second round trip (and may take the direct path below)
// (a d1-like varblock has an entry at ~11 % of its Y positions, half / two thirds of that in X / B:
// profiles/r05_c_entry_counts.txt)
template <class S>
constexpr int ent_depth() {
  constexpr int per_lane = S::E;                    // coefficients per lane and channel: 8, 16 or 32
  constexpr int lpb = 64 / S::NB;
  return per_lane <= 8 ? 3 : per_lane <= 16 ? (lpb <= 8 ? 4 : 3) : (lpb <= 8 ? 6 : lpb <= 16 ? 5 : 4);
}
template <int D>
struct EntLane {
  uint32_t i0[3], i1[3];  // this lane's first entry / the end of the varblock's range, per channel (frame-wide indices)
  uint32_t e[3][D];       // the lane's first D entries of each channel
};
// EX: the word an exclusive slot-count prefix of the three channels is packed in.  uint32_t, 10 bits per channel: enough
// for the varblocks the direct path takes (at most D entries per lane); uint64_t, 21 bits per channel: any count a
// varblock can legally have (16 slots x 255 entries -- repeated positions of several passes, wide values split into
// in-range entries), what the dense dequantisation pass (mode 2, the fallback of the direct kernels) is built with.
template <class EX>
constexpr int excl_bits() { return sizeof(EX) == 8 ? 21 : 10; }
template <class S, int D, class EX>
__device__ __forceinline__ void entries_begin(const FrameDev& f, const BlockInfo* __restrict__ binfo, EX* __restrict__ s_excl,
                                              int nb, int lane, EntLane<D>& sl) {
  constexpr int LPB = 64 / S::NB, NS = S::N / 64;
  static_assert(LPB >= NS, "one lane per slot for the count scan");
  const int b = lane / LPB, j = lane % LPB;
  const bool on = b < nb;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    sl.i0[c] = on ? binfo[b].e0[c] + j : 0u;
    sl.i1[c] = on ? binfo[b].e0[c] + binfo[b].en[c] : 0u;
  }
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int k = 0; k < D; k++) {
      const uint32_t i = sl.i0[c] + k * LPB;
      sl.e[c][k] = i < sl.i1[c] ? (uint32_t)f.se_entries[i] : 0u;
    }
  if constexpr (NS > 1) {
    constexpr int B = excl_bits<EX>();
    EX packed = 0;
    if (on && j < NS) {
      const uint8_t* cp = f.se_counts + binfo[b].cnt_base + j;
      packed = (EX)cp[0] | (EX)cp[kSlotsPerRun] << B | (EX)cp[2 * kSlotsPerRun] << (2 * B);
    }
    auto shfl_up = [](EX v, int d) {
      if constexpr (sizeof(EX) == 8) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, LPB), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, LPB);
        return (EX)((uint64_t)lo | (uint64_t)hi << 32);
      } else {
        return (EX)__shfl_up((int)v, d, LPB);
      }
    };
    // exclusive scan over the block's lanes (segments of LPB lanes): shift by one slot, then an inclusive scan
    EX x = shfl_up(packed, 1);
    if (j == 0) x = 0;
#pragma unroll
    for (int d = 1; d < NS; d <<= 1) {
      const EX y = shfl_up(x, d);
      if (j >= d) x += y;
    }
    if (j < NS) s_excl[b * NS + j] = x;  // b < NB always: the tile holds NB * NS words
  }
}
// position (in the varblock's stored order) of entry e, the r-th of the varblock's range of channel ch
template <class S, class EX>
__device__ __forceinline__ int entry_pos(const EX* __restrict__ s_excl, int b, int ch, uint32_t e, uint32_t r) {
  constexpr int NS = S::N / 64, B = excl_bits<EX>();
  int sidx = 0;
  if constexpr (NS > 1) {
#pragma unroll
    for (int step = NS / 2; step >= 1; step >>= 1) {
      const uint32_t v = (uint32_t)(s_excl[b * NS + sidx + step] >> (B * ch)) & ((1u << B) - 1u);
      if (r >= v) sidx += step;
    }
  }
  return sidx * 64 + (int)(e & 63u);
}
template <class S>
__device__ __forceinline__ void zero_tile(int* __restrict__ ibuf, int lane) {
  constexpr int kWords = S::NB * S::SM;
  if constexpr (kWords % 4 == 0) {
    for (int i = lane * 4; i < kWords; i += 256) *reinterpret_cast<int4*>(ibuf + i) = make_int4(0, 0, 0, 0);
  } else {
    for (int i = lane; i < kWords; i += 64) ibuf[i] = 0;
  }
}

// HELD = false (the inline fallback of the direct 8x8 kernel): the lane's first D entries are NOT taken from sl -- every
// entry is requested again (L2 hits), the range comes from the batch's BlockInfo -- so that nothing of sl stays alive
// through the transforms: with it the inline body raised the direct kernel from 76 to 98 VGPRs (6 -> 4 waves per SIMD).
template <class S, int D, class EX, bool HELD = true>
__device__ __forceinline__ void entries_stage_channel(const FrameDev& f, int ch, float* __restrict__ buf,
                                                      const EX* __restrict__ s_excl, int lane, const EntLane<D>& sl,
                                                      const BlockInfo* __restrict__ binfo = nullptr, int nb = 0) {
  int* ibuf = reinterpret_cast<int*>(buf);
  zero_tile<S>(ibuf, lane);
  wave_sync();
  constexpr int LPB = 64 / S::NB;
  const int b = lane / LPB, j = lane % LPB;
  auto add = [&](uint32_t e, uint32_t r) {  // r: index of the entry inside the varblock's range
    atomicAdd(&ibuf[m_addr<S>(b, entry_pos<S, EX>(s_excl, b, ch, e, r))], (int)(e << 16) >> 22);
  };
  constexpr int DH = HELD ? D : 0;
  uint32_t i0 = 0, i1 = 0;
  if constexpr (HELD) {
    i0 = sl.i0[ch];
    i1 = sl.i1[ch];
  } else if (b < nb) {
    i0 = binfo[b].e0[ch] + j;
    i1 = binfo[b].e0[ch] + binfo[b].en[ch];
  }
#pragma unroll
  for (int k = 0; k < DH; k++)
    if (i0 + k * LPB < i1) add(sl.e[ch][k], (uint32_t)(j + k * LPB));
  // what lies beyond the D entries a lane holds (content denser than d1, split wide values): four requests in flight per
  // lane and round -- one dependent load per entry made the dense pass 3x the time of the dense-slab kernels at four
  // times d1's density (round 6, profiles/r06_c_density.txt)
  constexpr int U = 4;
  uint32_t r = (uint32_t)(j + DH * LPB), i = i0 + DH * LPB;
  while (__any(i < i1)) {
    uint32_t ev[U];
#pragma unroll
    for (int u = 0; u < U; u++) ev[u] = i + u * LPB < i1 ? (uint32_t)f.se_entries[i + u * LPB] : 0u;
#pragma unroll
    for (int u = 0; u < U; u++)
      if (i + u * LPB < i1) add(ev[u], r + u * LPB);
    i += U * LPB;
    r += U * LPB;
  }
  wave_sync();
}

// ---- the direct path of the entries form: only the coefficients that HAVE an entry are dequantised; every other
// position of the tile is +0.0f, which is what the reference computes for a zero coefficient under the conditions
// FrameDev::se_direct_ok / tables_ok / AdjTable::nofast establish (group.rs:85-133: (0.0 * bias_c) * mul = +0.0,
// fma(cc, +0.0, +0.0) = +0.0; a non-zero coefficient never dequantises to a zero).  At d1 about one coefficient in ten
// has an entry: the dense pass (tile read, ~10 vector instructions and an LDS table lookup per POSITION, tile write)
// becomes ~15 instructions per ENTRY.  Duplicate positions (several passes' updates in one list) still add up as
// integers first:
//   a  ds_add of the entry's value into the zeroed tile              (integer sums, like `coeffs[i] += v`)
//   b  ds exchange of the word with a sentinel: the first lane to arrive gets the sum and owns the position
//   c  the owner writes the dequantised float over the sentinel
// (LDS operations of a wavefront execute in program order: every lane's step a is done before any step b, every b
// before any c.)  The sentinel INT32_MIN cannot be a sum: a run holds at most 65536 entries of 10 bits.  X and B then
// add the chroma-from-luma term at the positions Y owns, fma(cc, dy, v) in the reference's form; where Y has no entry
// the reference's fma(cc, +0.0, v) returns v itself (v is never -0.0).
template <int D>
struct EntDirect {
  uint32_t ad[3][D];  // position of the entry's coefficient in the varblock | value << 16; kNoEntry = no k-th entry
};
constexpr uint32_t kNoEntry = 0xffffffffu;
constexpr int kClaimed = (int)0x80000000;

template <class S, int CH, int D>
__device__ __forceinline__ void direct_stage_channel(const FrameDev& f, float* __restrict__ buf, int lane,
                                                     const EntDirect<D>& ed, const float* __restrict__ table, int tsize,
                                                     float sdy, float cc, const AdjTable* __restrict__ adj,
                                                     float (&dyw)[D], uint32_t& ywin) {
  int* ibuf = reinterpret_cast<int*>(buf);
  constexpr int LPB = 64 / S::NB;
  const int b = lane / LPB;
  // the dequant weights of this channel's entries: requested first, needed in step c
  float w[D];
#pragma unroll
  for (int k = 0; k < D; k++) w[k] = ed.ad[CH][k] != kNoEntry ? table[CH * tsize + (int)(ed.ad[CH][k] & 0xffffu)] : 0.0f;
  zero_tile<S>(ibuf, lane);
  wave_sync();
  int at[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    at[k] = m_addr<S>(b, (int)(ed.ad[CH][k] & 0x3ffu));
    if (ed.ad[CH][k] != kNoEntry) atomicAdd(&ibuf[at[k]], (int)ed.ad[CH][k] >> 16);
  }
  wave_sync();
  int sum[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    sum[k] = kClaimed;
    if (ed.ad[CH][k] != kNoEntry) sum[k] = atomicExch(&ibuf[at[k]], kClaimed);
  }
  wave_sync();
  float sd = sdy;
  if constexpr (CH == 0) sd = sdy * f.x_dm;
  if constexpr (CH == 2) sd = sdy * f.b_dm;
#pragma unroll
  for (int k = 0; k < D; k++) {
    if (sum[k] != kClaimed) {
      // dequant_lane (group.rs:100-133) for one coefficient, the operations of dequant4t
      const int q = sum[k];
      const uint32_t aq = wrapping_abs(q);
      float am = adj->v[CH][min(aq, (uint32_t)kAdjN - 1u)];
      if (aq >= (uint32_t)kAdjN)
        am = __uint_as_float(__float_as_uint(adjust_quant_bias(q, f.quant_biases[CH], f.quant_biases[3])) ^ ((uint32_t)q & 0x80000000u));
      const float a = __uint_as_float(__float_as_uint(am) ^ ((uint32_t)q & 0x80000000u));
      const float mul = w[k] * sd;
      const float v = a * mul;
      if constexpr (CH == 1) {
        dyw[k] = v;
        ywin |= 1u << k;
      }
      buf[at[k]] = v;
    }
  }
  if constexpr (CH != 1) {
    wave_sync();
#pragma unroll
    for (int k = 0; k < D; k++)
      if ((ywin >> k) & 1u) {
        float* t = buf + m_addr<S>(b, (int)(ed.ad[1][k] & 0x3ffu));
        *t = __builtin_fmaf(cc, dyw[k], *t);
      }
  }
  wave_sync();
}

template <class S>
__device__ __forceinline__ int4 tile_q4(const float* __restrict__ buf, int b, int k) {
  const int* ibuf = reinterpret_cast<const int*>(buf);
  if constexpr (S::kWide) {
    return make_int4(ibuf[m_addr<S>(b, k)], ibuf[m_addr<S>(b, k + 1)], ibuf[m_addr<S>(b, k + 2)],
                     ibuf[m_addr<S>(b, k + 3)]);
  } else {
    return *reinterpret_cast<const int4*>(ibuf + m_addr<S>(b, k));
  }
}

// gwave: this wave's index among the nwaves of the grid, rotated by the caller so that the classes one
// kernel handles start on different waves (batch b of a class goes to wave (rotation + b) % nwaves);
// without it every class would pile its batches on the low-numbered waves.  Returns the number of
// batches of the class (the next class's rotation).
// SUB (chroma-subsampled frames, S8x8 only): a channel holds a block only if the block is aligned to the channel's
// sampling (decode_item marks the others with px_off == scrap_off); their coefficients are never decoded (zeros
// in the reference's slab, frame/group.rs:521-524), so the loads are skipped and read as zero, and nothing is stored.
// SPARSE: 0 = dense slabs, 1 = bucketed pair words + slot tables (sp_sorted), 2 = slot-bucketed entries in place (se_*)
// with the dense dequantisation pass, 3 = the same input, direct path only: batches it cannot take are flagged in
// WorkLists::fallback[class] (one word per batch, written with the launch's epoch: no atomics, no clear per launch) and the
// fallback launch (LISTED) runs the flagged ones through mode 2.  CLS: the class id.
// INLINE_FB (mode 3): a batch the direct path cannot take runs through the dense dequantisation pass right here instead
// of going to the fallback list -- for the 8x8 class, whose generic body costs a handful of registers: a frame denser
// than d1 content then degrades batch by batch inside one launch (round 6).
// s_dy (mode 2, shapes with 32 coefficients per lane; nullable): the dequantised Y of the batch waits in LDS for the X / B
// channels' chroma-from-luma instead of in 32 registers through two 32-point IDCTs -- the kernels that take it run two
// workgroups per CU and have the room (S::E * 64 floats per wavefront).
template <class S, bool PREFETCH, int SPARSE, bool SUB = false, int CLS = 0, bool INLINE_FB = false, bool LISTED = false,
          class EX = uint32_t>
__device__ __forceinline__ int run_dct_class(const FrameDev& f, const WorkItem* __restrict__ items,
                                             const EntryItem* __restrict__ eitems, int count, int type,
                                             float* __restrict__ buf, BlockInfo* __restrict__ binfo_base,
                                             EX* __restrict__ s_excl, float* __restrict__ s_lf, int gwave,
                                             int nwaves, int lane, const AdjTable* __restrict__ adj,
                                             uint32_t* __restrict__ wl_fallback = nullptr,
                                             int* __restrict__ fallback_count = nullptr, float* __restrict__ s_dy = nullptr,
                                             uint32_t fb_first_flag = 0, uint32_t* __restrict__ wl_fb_any = nullptr,
                                             int* fb_rank = nullptr) {
  constexpr int NCH = S::E / 4;  // 16-byte chunks per lane per channel
  const int q = quant_table_for_type(type);
  const float* __restrict__ table = f.tables + f.table_offset[q];
  const int tsize = quant_table_size(q);
  const int nbatches = (count + S::NB - 1) / S::NB;
  // The batches this wave runs.  Plain: gwave, gwave + nwaves, ...  LISTED (the fallback launch): the batches whose word
  // in wl_fallback holds this launch's epoch -- a workgroup takes chunks of kFbChunk consecutive batches (one flag per
  // lane, a ballot), its kWaves waves share a chunk's flagged batches round robin; the caller rotates the chunk -> workgroup
  // map from class to class (gwave), so the classes' chunks spread over the whole grid, and hands over the flag word of
  // the workgroup's first FOUR chunks (fb_first_flag: the kernel requests those of all classes at once when it starts, so a
  // workgroup with nothing to do leaves after one memory round trip and one with work does not pay a round trip per
  // class).  (Round 6's first form appended batch ids to a list: one returning atomic per wave and class on one counter,
  // 131 000 of them on a frame that leaves every batch -- 0.27 ms for a launch with nothing else to do.)
  constexpr int kFbChunk = 16;  // (64-batch chunks leave most of the grid idle on dense frames: K1 0.42 -> 0.57 ms at x2)
  struct BatchIter {
    int bi;                    // plain: the batch; listed: the chunk
    unsigned long long mask;   // listed: flagged batches of the chunk not yet handed out
    bool pre;                  // listed: mask = the kernel's prefetch: the workgroup's first FOUR chunks, 16 bits each
  };
  const int it_wave = gwave % kWaves, it_wg = gwave / kWaves, it_nwg = nwaves / kWaves;  // (LISTED: gwave is not rotated)
  auto iter_next = [&](BatchIter& st) -> int {  // the next batch of this wave, -1 when done
    if constexpr (!LISTED) {
      const int b = st.bi;
      st.bi += nwaves;
      return b < nbatches ? b : -1;
    } else {
      for (;;) {
        while (st.mask) {
          const int bit = __builtin_ctzll(st.mask);
          st.mask &= st.mask - 1;
          const int chunk = st.pre ? st.bi + (bit >> 4) * it_nwg : st.bi;
          // (*fb_rank: flagged batches the WORKGROUP has met so far in this launch, over all classes -- its waves see
          // the same flags and count alike -- so the few batches a sparse frame leaves never queue up behind each other
          // on one wave while the other three idle: the launch then lasts one batch's latency, not two)
          if ((*fb_rank)++ % kWaves == it_wave) return chunk * kFbChunk + (bit & 15);
        }
        st.bi += st.pre ? 4 * it_nwg : it_nwg;
        st.pre = false;
        if (st.bi * kFbChunk >= nbatches) return -1;
        const int idx = st.bi * kFbChunk + lane;
        st.mask = __ballot(lane < kFbChunk && idx < nbatches && wl_fallback[idx] == (uint32_t)f.fb_epoch);
      }
    }
  };
  static_assert(kFbChunk == 16, "the prefetched mask holds four 16-batch chunks");
  BatchIter iter = {LISTED ? it_wg : gwave, LISTED ? __ballot(fb_first_flag == (uint32_t)f.fb_epoch && fb_first_flag != 0) : 0ull, LISTED};
  // the weights a lane needs do not depend on the batch
  constexpr bool kPF = PREFETCH && SPARSE != 3;  // (the inline fallback of mode 3 reads its weights per batch)
  float4 tw[kPF ? 3 : 1][NCH];
  if constexpr (kPF) {
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int j = 0; j < NCH; j++)
        tw[c][j] = *reinterpret_cast<const float4*>(table + c * tsize + ((j * 64 + lane) * 4) % S::N);
  }
  // The entries form is bound by the chain of dependent memory round trips of a batch (item -> entries, then the LF
  // samples of each channel right before its transform: five per batch, 72 % of a wavefront's life parked on them,
  // profiles/r05_b_sparse_pairs_pmc.txt), not by bytes.  kChain: the NEXT batch's items are requested while this one is
  // transformed, and the LF samples of all three channels are requested together with the entries (spread over the
  // lanes, handed over through LDS): one exposed round trip per batch.
  constexpr bool kChain = SPARSE >= 2;
#ifndef JXLH_ITEM_PREFETCH
#define JXLH_ITEM_PREFETCH 1  // 0 none, 1 the 8..16-point classes (register-light bodies), 2 every class
#endif
  constexpr bool kNextItem = kChain && !LISTED && (JXLH_ITEM_PREFETCH == 2 || (JXLH_ITEM_PREFETCH == 1 && PREFETCH));
  constexpr int kLfPerBlock = 3 * (S::R / 8) * (S::C / 8), kLfIters = (S::NB * kLfPerBlock + 63) / 64;
  // Dense slabs, the 16..32-point classes (16 coefficients per lane and channel): the three channels are dequantised in
  // one go, see generic_batch.  (Requesting the next batch's work items while this one is transformed, and the LF samples
  // together with the coefficients, as the entries form does, measured no better on dense slabs -- K1's 16..32-point
  // kernel 169.4 against 169.0 us, and 175.7 us with the LF samples ahead: profiles/r07_a_dense_k1_batches.txt.)
  constexpr bool kEarly = SPARSE == 0 && S::E == 16;
  WorkItem it_next = {};
  EntryItem ei_next = {};
  if constexpr (kNextItem) {
    if (gwave < nbatches && lane < min(S::NB, count - gwave * S::NB)) {
      it_next = items[gwave * S::NB + lane];
      ei_next = eitems[gwave * S::NB + lane];
    }
  }
  int n_dense_pass = 0;  // (wave-uniform) batches this wave ran through the dense pass: inline (mode 3) or listed
  bool flagged_any = false;
  for (int batch = iter_next(iter); batch >= 0; batch = iter_next(iter)) {
    const int nb = min(S::NB, count - batch * S::NB);
    if constexpr (LISTED) n_dense_pass++;
    BlockInfo* __restrict__ binfo = binfo_base;
    bool direct_ok = true;  // (wave-uniform)
    if constexpr (kChain) {
      WorkItem it = it_next;
      EntryItem ei = ei_next;
      if constexpr (kNextItem) {
        const int nxt = batch + nwaves;
        if (nxt < nbatches && lane < min(S::NB, count - nxt * S::NB)) {
          it_next = items[nxt * S::NB + lane];
          ei_next = eitems[nxt * S::NB + lane];
        }
      } else if (lane < nb) {
        it = items[batch * S::NB + lane];
        ei = eitems[batch * S::NB + lane];
      }
      bool item_ok = true;
      if (lane < nb) {
        decode_item(f, it, &binfo[lane]);
#pragma unroll
        for (int c = 0; c < 3; c++) binfo[lane].e0[c] = ei.e0[c];
        binfo[lane].en[0] = ei.nxy & 0xffffu;
        binfo[lane].en[1] = ei.nxy >> 16;
        binfo[lane].en[2] = it.group >> 16;
        if constexpr (SPARSE == 3) {
          // the direct path takes a varblock whose raw_quant the division survives and that has no more entries per
          // channel than its lanes hold
          const float sdy = binfo[lane].sdy;
          item_ok = sdy > 0.0f && sdy < __builtin_inff() &&
                    max(max(ei.nxy & 0xffffu, ei.nxy >> 16), it.group >> 16) <= (uint32_t)(ent_depth<S>() * (64 / S::NB));
        }
      }
      if constexpr (SPARSE == 3 && !INLINE_FB) {
        // left to the fallback launch BEFORE anything of the batch is requested: its word gets the launch's epoch
        if (!__all(item_ok)) {
          if (lane == 0) {
            wl_fallback[batch] = (uint32_t)f.fb_epoch;
            // ... and one of the launch's kFbAny summary words (own cache lines, picked by the wave): plain stores of
            // the same value, a wave's first reject only
            if (!flagged_any) wl_fb_any[(gwave % kFbAny) * kFbAnyPitch] = (uint32_t)f.fb_epoch;
          }
          flagged_any = true;
          continue;
        }
      } else {
        direct_ok = __all(item_ok);
      }
    } else if (lane < nb) {
      const WorkItem it = items[batch * S::NB + lane];
      decode_item(f, it, &binfo[lane]);
    }
    wave_sync();
    SparseLane sl;
    constexpr int D = ent_depth<S>();
    EntLane<D> el;
    if constexpr (SPARSE == 1) {
      sparse_ranges<S>(f, binfo, nb, lane, sl);
      sparse_first<S>(f, sl);
    } else if constexpr (SPARSE >= 2) {
      entries_begin<S, D, EX>(f, binfo, s_excl, nb, lane, el);
    }
    if constexpr (kChain) {
      // LF sample idx = (block, channel, y, x) of the batch: requested now, in LDS before the first transform
      float lfv[kLfIters];
#pragma unroll
      for (int i = 0; i < kLfIters; i++) {
        const int idx = i * 64 + lane, b = idx / kLfPerBlock, rem = idx % kLfPerBlock;
        const int c = rem / ((S::R / 8) * (S::C / 8)), yx = rem % ((S::R / 8) * (S::C / 8));
        const int y = yx / (S::C / 8), x = yx % (S::C / 8);
        lfv[i] = 0.0f;
        if (b < nb) {
          const float* __restrict__ lp = c == 0 ? f.lf[0] : c == 1 ? f.lf[1] : f.lf[2];
          lfv[i] = lp[binfo[b].lf_off[c] + y * f.xblocks + x];
        }
      }
#pragma unroll
      for (int i = 0; i < kLfIters; i++)
        if (i * 64 + lane < S::NB * kLfPerBlock) s_lf[i * 64 + lane] = lfv[i];
      // (published by the wave_sync that follows the tile's zero fill in entries_stage_channel)
    }
    auto transform_channel = [&](auto ch_tag) {
      constexpr int CH = decltype(ch_tag)::value;
      const float* __restrict__ lfp = f.lf[CH];
      float* __restrict__ plane = f.planes[CH];
      const PixLayout lay = pix_layout(f);
      const int xblocks = f.xblocks;
      idct_batch<S>(
          buf, nb, lane,
          [&](int b, int y, int x) {
            if constexpr (kChain) return s_lf[b * kLfPerBlock + (CH * (S::R / 8) + y) * (S::C / 8) + x];
            else return lfp[binfo[b].lf_off[CH] + y * xblocks + x];
          },
          [&](int b, int x, int yb, const float(&v)[8]) {
            if (SUB && binfo[b].px_off[CH] == f.scrap_off) return;
            float* dst = plane + binfo[b].px_off[CH] + lay.xoff(x) + yb * lay.ystep_blk;
            if (lay.tiled) {  // rows 0-3 and rows 4-7 of the lane's column: two 16-byte stores, 128 bytes apart
              gstore_f4<JXLH_NT_K1_STORE>(dst, make_float4(v[0], v[1], v[2], v[3]));
              gstore_f4<JXLH_NT_K1_STORE>(dst + 32, make_float4(v[4], v[5], v[6], v[7]));
            } else {
#pragma unroll
              for (int i = 0; i < 8; i++) dst[i * lay.ystep8] = v[i];
            }
          });
    };
    using TagX = std::integral_constant<int, 0>;
    using TagY = std::integral_constant<int, 1>;
    using TagB = std::integral_constant<int, 2>;
    // the dense dequantisation pass: every coefficient position of the batch (GM: 0 dense slabs, 1 pair words, 2 entries)
    auto generic_batch = [&](auto mode_tag) {
      constexpr int GM = decltype(mode_tag)::value;
      // dense slabs: all three channels' coefficients are requested together whenever a lane holds at most 16 per channel
      // (48 registers) -- with or without the weights resident (kPF): the two are separate switches
      constexpr bool kQPF = !GM && (kPF || S::E <= 16);
      int4 qv[kQPF ? 3 : 1][NCH];
      if constexpr (kQPF) {
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int j = 0; j < NCH; j++) {
            const int fl = (j * 64 + lane) * 4;
            const int b = fl / S::N, k = fl % S::N;
            qv[c][j] = make_int4(0, 0, 0, 0);
            if (b < nb && (!SUB || binfo[b].px_off[c] != f.scrap_off))
              qv[c][j] = gload_i4<JXLH_NT_COEF>(f.coeffs + binfo[b].coef_off + c * kGroupArea + k);
          }
      }
      // The dequantised Y the X / B channels' chroma-from-luma needs is kept in registers across the channels.  (Dense
      // slabs once ran the shapes with a 32-point side at 32 coefficients per lane, where 32 values of Y would have sat
      // through two 32-point IDCTs: X and B loaded and dequantised their Y again.  Those shapes now run at half the batch.)
      static_assert(GM != 0 || S::E <= 16, "dense slabs: at most 16 coefficients per lane and channel");
      constexpr bool kDyLds = GM == 2 && SPARSE == 2 && S::E > 16;  // (callers of mode 2 pass s_dy)
      float dy[kDyLds ? 4 : S::E];
      auto stage_channel = [&](auto ch_tag) {
        constexpr int CH = decltype(ch_tag)::value;
        if constexpr (GM == 1) sparse_stage_channel<S>(f, CH, buf, lane, sl);
        if constexpr (GM == 2) entries_stage_channel<S, D, EX, SPARSE == 2>(f, CH, buf, s_excl, lane, el, binfo, nb);
#pragma unroll
        for (int j = 0; j < NCH; j++) {
          const int fl = (j * 64 + lane) * 4;
          const int b = fl / S::N, k = fl % S::N;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          float d4[4];
          if constexpr (kDyLds) {
            d4[0] = d4[1] = d4[2] = d4[3] = 0.0f;
            if constexpr (CH != 1) {
              const float4 t = *reinterpret_cast<const float4*>(s_dy + (j * 64 + lane) * 4);
              d4[0] = t.x;
              d4[1] = t.y;
              d4[2] = t.z;
              d4[3] = t.w;
            }
          } else {
            d4[0] = dy[j * 4];
            d4[1] = dy[j * 4 + 1];
            d4[2] = dy[j * 4 + 2];
            d4[3] = dy[j * 4 + 3];
          }
          if (b < nb) {
            const BlockInfo bi = binfo[b];
            int4 qq;
            float4 tt;
            if constexpr (GM != 0) {
              qq = tile_q4<S>(buf, b, k);  // converted in place: this lane alone touches (b, k..k+3)
              if constexpr (kPF) tt = tw[CH][j];
              else tt = *reinterpret_cast<const float4*>(table + CH * tsize + k);
            } else {
              if constexpr (kQPF) qq = qv[CH][j];
              else qq = gload_i4<JXLH_NT_COEF>(f.coeffs + bi.coef_off + CH * kGroupArea + k);
              if constexpr (kPF) tt = tw[CH][j];
              else tt = *reinterpret_cast<const float4*>(table + CH * tsize + k);
            }
            v = dequant4t<CH>(f, qq, tt, bi, adj, d4);
          }
          if constexpr (CH == 1 && kDyLds) {
            *reinterpret_cast<float4*>(s_dy + (j * 64 + lane) * 4) = make_float4(d4[0], d4[1], d4[2], d4[3]);
          } else if constexpr (CH == 1) {
            dy[j * 4] = d4[0];
            dy[j * 4 + 1] = d4[1];
            dy[j * 4 + 2] = d4[2];
            dy[j * 4 + 3] = d4[3];
          }
          stage4<S>(buf, b, k, v);
        }
        wave_sync();
      };
      if constexpr (kEarly && !GM) {
        // 16 coefficients per lane and channel, all requested above: X and B are dequantised right behind Y, chunk by
        // chunk (dequant4t in the reference's order Y, X, B; the Y a chunk's chroma-from-luma takes is four registers
        // old), so what waits through the first two transforms is 32 finished values -- not 32 integers and 16 Y values
        float4 vx[NCH];
#pragma unroll
        for (int j = 0; j < NCH; j++) {
          const int fl = (j * 64 + lane) * 4;
          const int b = fl / S::N, k = fl % S::N;
          float4 vy = make_float4(0.f, 0.f, 0.f, 0.f);
          float4 vb = vy;
          vx[j] = vy;
          if (b < nb) {
            const BlockInfo bi = binfo[b];
            float d4[4];
            float4 ty, tx, tb;
            if constexpr (kPF) {
              ty = tw[1][j];
              tx = tw[0][j];
              tb = tw[2][j];
            } else {
              ty = *reinterpret_cast<const float4*>(table + tsize + k);
              tx = *reinterpret_cast<const float4*>(table + k);
              tb = *reinterpret_cast<const float4*>(table + 2 * tsize + k);
            }
            vy = dequant4t<1>(f, qv[1][j], ty, bi, adj, d4);
            vx[j] = dequant4t<0>(f, qv[0][j], tx, bi, adj, d4);
            vb = dequant4t<2>(f, qv[2][j], tb, bi, adj, d4);
          }
          stage4<S>(buf, b, k, vy);
          *reinterpret_cast<float4*>(s_dy + (j * 64 + lane) * 4) = vb;  // (read back by this lane alone)
        }
        wave_sync();
        transform_channel(TagY{});
#pragma unroll
        for (int j = 0; j < NCH; j++) stage4<S>(buf, ((j * 64 + lane) * 4) / S::N, ((j * 64 + lane) * 4) % S::N, vx[j]);
        wave_sync();
        transform_channel(TagX{});
#pragma unroll
        for (int j = 0; j < NCH; j++)
          stage4<S>(buf, ((j * 64 + lane) * 4) / S::N, ((j * 64 + lane) * 4) % S::N,
                    *reinterpret_cast<const float4*>(s_dy + (j * 64 + lane) * 4));
        wave_sync();
        transform_channel(TagB{});
        return;
      }
      // channel order of the reference: Y, X, B (group.rs:223)
      stage_channel(TagY{});
      transform_channel(TagY{});
      stage_channel(TagX{});
      transform_channel(TagX{});
      stage_channel(TagB{});
      transform_channel(TagB{});
    };
    if constexpr (SPARSE == 3) {
      // direct path: every varblock of the batch has a raw_quant the division survives and no more entries per channel
      // than its lanes hold -- otherwise the batch is left to the dense pass (k1_entries_fallback)
      constexpr int LPB = 64 / S::NB;
      const int b = lane / LPB, j = lane % LPB;
      float sdy = 0.0f, xcc = 0.0f, bcc = 0.0f;
      if (b < nb) {
        sdy = binfo[b].sdy;
        xcc = binfo[b].x_cc;
        bcc = binfo[b].b_cc;
      }
      if constexpr (INLINE_FB) {
        if (!direct_ok) {
          static_assert(S::N == 64, "the inline fallback has no slot prefixes: one-slot varblocks only");
          generic_batch(std::integral_constant<int, 2>{});
          n_dense_pass++;
          wave_sync();  // binfo / s_lf are rewritten by the next batch
          continue;
        }
      }
      wave_sync();  // the slot prefixes (entries_begin) are in LDS
      EntDirect<D> ed;
#pragma unroll
      for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < D; k++) {
          ed.ad[c][k] = kNoEntry;
          if (el.i0[c] + k * LPB < el.i1[c]) {
            const uint32_t e = el.e[c][k];
            ed.ad[c][k] = (uint32_t)entry_pos<S, EX>(s_excl, b, c, e, (uint32_t)(j + k * LPB)) | (uint32_t)((int)(e << 16) >> 22) << 16;
          }
        }
      float dyw[D];
      uint32_t ywin = 0;
#pragma unroll
      for (int k = 0; k < D; k++) dyw[k] = 0.0f;
      direct_stage_channel<S, 1, D>(f, buf, lane, ed, table, tsize, sdy, 0.0f, adj, dyw, ywin);
      transform_channel(TagY{});
      direct_stage_channel<S, 0, D>(f, buf, lane, ed, table, tsize, sdy, xcc, adj, dyw, ywin);
      transform_channel(TagX{});
      direct_stage_channel<S, 2, D>(f, buf, lane, ed, table, tsize, sdy, bcc, adj, dyw, ywin);
      transform_channel(TagB{});
    } else {
      generic_batch(std::integral_constant<int, SPARSE>{});
    }
  }
  // statistics (jxlh_frame_k1_counters; only while kernel timing is on: 16 000 waves' atomics on one counter cost 0.2 ms)
  if (f.k1_stats && (LISTED || INLINE_FB) && n_dense_pass && lane == 0) atomicAdd(fallback_count, n_dense_pass);
  return nbatches;
}

// wave index rotated by the batches the previous classes of the kernel occupy
__device__ __forceinline__ int rotate_wave(int gw, int used, int nw) {
  const int r = (gw - used % nw) % nw;
  return r < 0 ? r + nw : r;
}

template <class S>
struct ShapeTag {
  using type = S;
};
using S8x8 = Shape<8, 8>;
using S16x16 = Shape<16, 16>;
using S32x32 = Shape<32, 32>;
using S16x8 = Shape<16, 8>;
using S8x16 = Shape<8, 16>;
using S32x8 = Shape<32, 8, 4>;  // tall 32x8 at NB = 8 would need a 3136-word tile
using S8x32 = Shape<8, 32>;
using S32x16 = Shape<32, 16>;
using S16x32 = Shape<16, 32>;

// Dense slabs: the classes with a 32-point side at HALF the varblocks per batch -- 16 coefficients per lane and channel,
// like 16x16 and 32x8 -- so that their body is the one the small shapes run: the three channels' coefficients requested
// together (48 registers), the dequantised Y kept in 16.  (At 32 per lane that form does not fit: the channels went to
// memory one after the other and X / B loaded and dequantised their Y again.)
using D32x32 = Shape<32, 32, 1>;
using D32x16 = Shape<32, 16, 2>;
using D16x32 = Shape<16, 32, 2>;
using D8x32 = Shape<8, 32, 4>;
constexpr int kTileD = cmax(cmax(cmax(cmax(S32x8::kTile, D8x32::kTile), cmax(D32x16::kTile, D16x32::kTile)), D32x32::kTile),
                            cmax(cmax(S16x16::kTile, S16x8::kTile), cmax(S8x16::kTile, S8x8::kTile)));  // 1600 words
constexpr int kTileA = S8x8::kTile;                                               // 832 words
constexpr int kTileC = cmax(cmax(cmax(S32x8::kTile, S8x32::kTile), cmax(S32x16::kTile, S16x32::kTile)),
                            S32x32::kTile);                                       // 2624

// family A: DCT 8x8 -- the dominant transform
// INLINE (mode 3): batches beyond the direct path's depth take the dense dequantisation pass inside this launch (one-slot
// varblocks need no slot prefixes) instead of going to the fallback launch.  The host picks the form per frame from the
// density of its entries (FrameDev::se_dense_hint): the inline body costs registers (79 -> 98 VGPRs, 6 -> 4 waves per
// SIMD: +12 us on a d1 frame), the fallback launch a second pass over the work items (0.84 against 0.68 ms for K1 at
// four times d1's density; profiles/r06_c_density.txt).
// (the direct form without the inline body sits one register above six waves per SIMD: the bound makes the compiler fit)
template <int SPARSE, bool SUB = false, bool INLINE = false>
#ifndef JXLH_K1_INLINE_WPE
#define JXLH_K1_INLINE_WPE 1  // waves per SIMD the inline form is compiled for (1 = whatever its 96 VGPRs allow: 5)
#endif
__global__ __launch_bounds__(kThreads, SPARSE == 3 ? (INLINE ? JXLH_K1_INLINE_WPE : 6) : 1) void k1_dct8(const FrameDev f, const WorkLists wl) {
  __shared__ __attribute__((aligned(16))) float s_buf[kWaves * kTileA];
  __shared__ BlockInfo s_binfo[kWaves][S8x8::NB];
  __shared__ AdjTable s_adj;
  build_adj_table(f, &s_adj, threadIdx.x, kThreads);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ float s_lf[SPARSE >= 2 ? kWaves : 1][S8x8::NB * 3];
  // (mode 3: batches beyond the direct path's depth take the dense dequantisation pass inline -- one-slot varblocks need
  // no slot prefixes, and the generic body fits the kernel's registers)
  static_assert(!INLINE || SPARSE == 3, "the inline fallback belongs to the direct form");
  run_dct_class<S8x8, true, SPARSE, SUB, kClsDct8, INLINE>(f, wl.items[kClsDct8], wl.eitems[kClsDct8], wl.counts[(kClsDct8) * kCountPitch], 0,
                                                   s_buf + wave * kTileA, s_binfo[wave], (uint32_t*)nullptr, s_lf[SPARSE >= 2 ? wave : 0],
                                                   blockIdx.x * kWaves + wave, gridDim.x * kWaves, lane, &s_adj,
                                                   wl.fallback[kClsDct8], wl.counts + (kCntFallback0 + kClsDct8) * kCountPitch, nullptr, 0u,
                                                   wl.fb_any);
}

// families B (16x8, 8x16, 16x16) + C (everything with a 32-point side) in ONE launch (round 3): as two kernels both
// ran at three waves per SIMD (145 / 168 VGPRs), so merging them costs no occupancy and removes a kernel boundary -- one
// fill / drain less in K1's serial sequence -- while the eight class lists spread over one grid (rotated start waves).
// Occupancy is not what limits these classes' batches anyway: at two waves per SIMD the 32-point family runs 24 %
// slower, the 16-point one 8 %, and DCT8 is flat between 3 and 5 (profiles/r03_n_k1.txt); requesting the LF samples
// of a batch ahead of the coefficients (through an LDS scratch) measured flat as well
// exclusive slot-count prefixes of a batch's varblocks (entries form): NB * (N / 64) words, at most 40 (8 x 32)
constexpr int kExclWords = 40;
#ifndef JXLH_K1_DIRECT_WPE
#define JXLH_K1_DIRECT_WPE 3  // waves per SIMD the direct form of k1_dct16_32 is compiled for
#endif
// mode 2 (the dense dequantisation pass of the entries form: frames whose parameters rule the direct path out) is
// compiled for two workgroups per CU: its 32-point bodies then hold everything in registers + the LDS stash of the
// dequantised Y (at three they spilled 250-330 bytes per lane)
constexpr int kDyWords = 32 * 64;  // S::E * 64 for the shapes with a 32-point side
// FB (mode 2 only): the fallback launch of the direct form -- per class, the batches flagged in WorkLists::fallback[class]
// (what the direct kernels could not take: more entries than their lanes hold, raw_quant == 0) instead of the class's
// whole list.  Usually a handful of batches (a workgroup reads a few words of flags per class and leaves); on content
// denser than d1 it is the main route of the 16..32-point classes.  (Round 5's fallback kernel dispatched one mixed list through a switch over the nine
// bodies: 203 spilled VGPRs, 792 bytes of scratch per lane.)
template <int SPARSE, bool FB = false, bool ALL = false>
__global__ __launch_bounds__(kThreads, SPARSE == 3 ? JXLH_K1_DIRECT_WPE : SPARSE == 2 ? 2 : 3) void k1_dct16_32(const FrameDev f, const WorkLists wl) {
  static_assert(!FB || SPARSE == 2, "the fallback launch runs the dense dequantisation pass of the entries form");
  static_assert(!ALL || SPARSE == 0, "one launch for every DCT class: dense slabs only");
  // FB: the flag word of this lane in the workgroup's first four chunks of every class, requested together before anything
  // else of the workgroup is set up (order = the order the classes run in below; a class's chunk c belongs to workgroup
  // (c + chunks of the classes before it) % grid).  Nothing flagged there and no later chunk: the workgroup leaves.
  uint32_t fb_pre[kClsSpecial] = {};
  uint32_t fb_live = 0;  // FB: classes (bit = position in the FB order) with a flagged batch or chunks beyond the prefetch
  if constexpr (FB) {
    // first level: the launch's summary words (one hot load; the direct kernels set one on a wave's first reject).  A
    // frame that left nothing -- the usual one -- costs this launch ~4 us instead of the ~25 us of the flag prefetch.
    // (the class counters are requested in the same round trip)
    const uint32_t summary = wl.fb_any[(threadIdx.x & (kFbAny - 1)) * kFbAnyPitch];
    constexpr int kOrder[kClsSpecial] = {kClsDct32x32, kClsDct32x16, kClsDct16x32, kClsDct32x8, kClsDct8x32,
                                         kClsDct16x16, kClsDct16x8,  kClsDct8x16,  kClsDct8};
    constexpr int kNb[kClsSpecial] = {S32x32::NB, S32x16::NB, S16x32::NB, S32x8::NB, S8x32::NB, S16x16::NB, S16x8::NB, S8x16::NB, S8x8::NB};
    const int grid = (int)gridDim.x, l = threadIdx.x & 63;
    int nbat[kClsSpecial];
#pragma unroll
    for (int k = 0; k < kClsSpecial; k++) nbat[k] = (wl.counts[kOrder[k] * kCountPitch] + kNb[k] - 1) / kNb[k];
    if (!__any(summary == (uint32_t)f.fb_epoch)) return;
    int used = 0;
#pragma unroll
    for (int k = 0; k < kClsSpecial; k++) {
      // (chunks of 16 batches: lanes 16 r .. 16 r + 15 take the workgroup's chunk of round r, fc + r * grid)
      const int nch = (nbat[k] + 15) / 16, fc = rotate_wave((int)blockIdx.x, used, grid), idx = (fc + (l >> 4) * grid) * 16 + (l & 15);
      fb_pre[k] = idx < nbat[k] ? wl.fallback[kOrder[k]][idx] : 0u;
      if (fc + 4 * grid < nch) fb_live |= 1u << k;
      used += nch;
    }
#pragma unroll
    for (int k = 0; k < kClsSpecial; k++)
      if (__any(fb_pre[k] == (uint32_t)f.fb_epoch)) fb_live |= 1u << k;
    if (!fb_live) return;  // (every wave of the workgroup reads the same words: uniform)
  }
  constexpr bool kDense = SPARSE == 0;
  constexpr int kTileK = kDense ? kTileD : kTileC;
  __shared__ __attribute__((aligned(16))) float s_buf[kWaves * kTileK];
  __shared__ BlockInfo s_binfo[kWaves][8];
  using EX = std::conditional_t<SPARSE == 2, uint64_t, uint32_t>;  // mode 2 takes any entry count (excl_bits)
  __shared__ EX s_excl[SPARSE >= 2 ? kWaves : 1][kExclWords];
  __shared__ AdjTable s_adj;
  build_adj_table(f, &s_adj, threadIdx.x, kThreads);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* buf = s_buf + wave * kTileK;
  EX* ex = s_excl[SPARSE >= 2 ? wave : 0];
  __shared__ float s_lfs[SPARSE >= 2 ? kWaves : 1][96];  // LF samples of a batch: NB * 3 * (R / 8) * (C / 8) <= 96
  float* lfs = s_lfs[SPARSE >= 2 ? wave : 0];
  // (dense slabs: the finished B values of a batch wait here through the Y and X transforms, 16 per lane)
  constexpr int kParkWords = 16 * 64;
  __shared__ __attribute__((aligned(16))) float s_dyb[SPARSE == 2 ? kWaves * kDyWords : kDense ? kWaves * kParkWords : 4];
  float* sdy = SPARSE == 2 ? s_dyb + wave * kDyWords : kDense ? s_dyb + wave * kParkWords : nullptr;
  const int gw = blockIdx.x * kWaves + wave, nw = gridDim.x * kWaves;
  auto cnt = [&](int cls) { return wl.counts[cls * kCountPitch]; };
  // the long batches (32-point sides) first: the tail of the launch is then made of the short ones
  int used = 0, fb_rank = 0;
  auto run = [&](auto shape_tag, auto pf_tag, auto cls_tag, int type, int fb_k = 0) {  // fb_k: index in the FB order
    using S = typename decltype(shape_tag)::type;
    constexpr bool PF = decltype(pf_tag)::value;
    constexpr int CLS = decltype(cls_tag)::value;
    if constexpr (FB) {
      // nothing of the class for this workgroup: not even the class's preamble (a sparse frame's few batches otherwise
      // start ~1.4 us later per class in front of them: 12-14 us for the 8x8 class, the last one)
      if (!((fb_live >> fb_k) & 1u)) {
        used += ((cnt(CLS) + S::NB - 1) / S::NB + 15) / 16;
        return;
      }
    }
    // (FB: the rotation counts workgroups -- a class's chunk c goes to workgroup (c + chunks of the classes before) % grid)
    const int nbat = run_dct_class<S, PF, SPARSE, false, CLS, false, FB>(
        f, wl.items[CLS], wl.eitems[CLS], cnt(CLS), type, buf, s_binfo[wave], ex, lfs,
        FB ? rotate_wave((int)blockIdx.x, used, (int)gridDim.x) * kWaves + wave : rotate_wave(gw, used, nw), nw, lane, &s_adj,
        wl.fallback[CLS], wl.counts + (kCntFallback0 + CLS) * kCountPitch, sdy, FB ? fb_pre[fb_k] : 0u, wl.fb_any, &fb_rank);
    used += FB ? (nbat + 15) / 16 : nbat;
  };
  run(ShapeTag<std::conditional_t<kDense, D32x32, S32x32>>{}, std::false_type{}, std::integral_constant<int, kClsDct32x32>{}, 5, 0);
  run(ShapeTag<std::conditional_t<kDense, D32x16, S32x16>>{}, std::false_type{}, std::integral_constant<int, kClsDct32x16>{}, 10, 1);
  run(ShapeTag<std::conditional_t<kDense, D16x32, S16x32>>{}, std::false_type{}, std::integral_constant<int, kClsDct16x32>{}, 11, 2);
  run(ShapeTag<S32x8>{}, std::false_type{}, std::integral_constant<int, kClsDct32x8>{}, 8, 3);
  run(ShapeTag<std::conditional_t<kDense, D8x32, S8x32>>{}, std::false_type{}, std::integral_constant<int, kClsDct8x32>{}, 9, 4);
  run(ShapeTag<S16x16>{}, std::true_type{}, std::integral_constant<int, kClsDct16x16>{}, 4, 5);
  run(ShapeTag<S16x8>{}, std::true_type{}, std::integral_constant<int, kClsDct16x8>{}, 6, 6);
  run(ShapeTag<S8x16>{}, std::true_type{}, std::integral_constant<int, kClsDct8x16>{}, 7, 7);
  // (the 8x8 class: only when its kernel ran without the inline fallback; the list stays empty otherwise)
  if constexpr (FB) run(ShapeTag<S8x8>{}, std::true_type{}, std::integral_constant<int, kClsDct8>{}, 0, 8);
  // ALL: the 8x8 class too -- every DCT class in one launch (the dense-route lists of a routed frame; as the form of
  // whole dense frames it lost on the pipelined headline: profiles/r06_f_k1_merged.txt)
  if constexpr (ALL) run(ShapeTag<S8x8>{}, std::true_type{}, std::integral_constant<int, kClsDct8>{}, 0);
}

static_assert(S8x8::NB == kDct8Batch, "k1_plan.h sizes the 8x8 class's grid by its batch");

}  // namespace

void launch_k1_dct(hipStream_t s, const K1Step& step, const FrameDev& f, const WorkLists& wl) {
  // in the order of K1Kernel (k1_plan.h)
  static constexpr K1ClassKernel kTable[] = {
      k1_dct8<kFormDense>,       k1_dct8<kFormSorted>,       k1_dct8<kFormEntries>,       k1_dct8<kFormDirect>,
      k1_dct8<kFormDirect, false, true>,
      k1_dct8<kFormDense, true>, k1_dct8<kFormSorted, true>, k1_dct8<kFormEntries, true>, k1_dct8<kFormDirect, true, true>,
      k1_dct16_32<kFormDense>,   k1_dct16_32<kFormSorted>,   k1_dct16_32<kFormEntries>,   k1_dct16_32<kFormDirect>,
      k1_dct16_32<kFormEntries, true>, k1_dct16_32<kFormDense, false, true>};
  static_assert(sizeof(kTable) / sizeof(kTable[0]) == kK1Special0 - kK1Class0, "one kernel per id of k1_plan.h");
  hipLaunchKernelGGL(kTable[step.kernel - kK1Class0], dim3(step.grid), dim3(step.block), 0, s, f, wl);
}

}  // namespace jxlh
