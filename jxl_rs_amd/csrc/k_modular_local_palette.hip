// Group-local GENERAL palettes (TransformStep::Palette::local_apply -> do_palette_step_general, apply_local.rs:260-294,
// palette.rs:165-262): delta entries added to a prediction of the group's own finished samples, predictors 1..13, for
// every such palette of a batch in one launch -- and the point-wise phases (RCT, look-up palette, copies) of those
// groups in front of and behind it.
//
// k_modular_local_palette: one workgroup per (job, output channel); a job is one general palette of one group.
//  * A workgroup is ONE wavefront and lane l owns row y0 + l of a band of kLpRows rows.  Pixel (x, y) needs (x + 2, y - 1),
//    so the rows run skewed by three columns (step s: lane l is at x = s - 3 l), exactly the wavefront of
//    k5_palette_delta / k5_palette_wp (k_modular.hip), with the per-pixel arithmetic shared through
//    modular_predict_device.h.  With one wavefront per workgroup a step ends in an LDS wait, not in a barrier, and the
//    LDS a workgroup needs (20 KiB, 35 KiB weighted, + 8 KiB palette row) lets several of them share a CU.
//  * NO workgroup waits on another: groups are independent, and a group taller than kLpRows is walked band by band by
//    its own workgroup.  The two rows above a band (for predictor 6 also the five rows of predictor state, kept in
//    context scratch, two sets used in turn) are re-read from what the workgroup itself wrote, ordered at workgroup
//    scope: a release fence and a drained store queue behind the band, workgroup-scope loads in the next.
//  * Global memory is touched in chunks of kLpChunk steps, never inside a step (the reasons at k5_palette_delta): per
//    chunk a lane stores the previous chunk's outputs, turns the next chunk's indices -- requested a whole chunk ago --
//    into palette entries (get_palette_value with palette_size = num_colors + num_deltas; the look-ups are off the
//    steps' dependent path) and requests the chunk after that.  A chunk of a row is 32 contiguous samples and is
//    moved transposed (thread t: column t % 32 of rows t / 32 + 2 i), so that a wave instruction touches two 128-byte
//    row segments.  Rows are strided on both sides: the index has the coded (or scratch) stride, the output the planes'.
//  * The channel's palette row is staged in LDS while it holds <= kLpLdsEntries values and read from global memory
//    beyond that.
//  * Columns outside a row are read from the nearest valid one, rows below the group from its last row: every load and
//    every store stays inside the group's rect, its index rect and its own scratch.
//
// k_modular_local_phase: k_modular_local's streaming pass for a group whose channels are, between phases, partly in the
// arena, partly in its destination rect and partly (an index channel its palette is about to overwrite) in scratch.
#include "jxlh_internal.h"
#include "modular_local_desc.h"
#include "modular_local_device.h"
#include "modular_ops_device.h"
#include "modular_predict_device.h"

namespace jxlh {
namespace {

constexpr int R = kLpRows, C = kLpChunk;
static_assert(R == 64 && C == 32, "one wavefront per workgroup; the mover maps 64 threads onto 64 rows x 32 columns");
constexpr int NI = 32;  // samples per thread and chunk
// LDS layout, in ints.  Ring rows 0 / 1 are the two rows ABOVE the band, fed from s_above one step ahead by lane 0;
// lane l owns ring row l + 2.  s_val holds a pixel's palette entry until its step replaces it by the finished sample.
constexpr int kRing = (R + 2) * 9, kTile = R * (C + 1);
constexpr int kOffRing = 0, kOffIdx = kOffRing + kRing, kOffVal = kOffIdx + kTile, kOffAbove = kOffVal + kTile;
constexpr int kDeltaEnd = kOffAbove + 2 * 128;
constexpr int kOffTe = kDeltaEnd, kOffE = kOffTe + kRing, kOffState = kOffE + 4 * kRing, kOffAboveTe = kOffState + 5 * C;
constexpr int kOffAboveE = kOffAboveTe + 128, kOffDiv = kOffAboveE + 4 * 128, kWpEnd = kOffDiv + 64;

// this wavefront's LDS writes are done and visible to all its lanes (LDS operations of one wavefront execute in order)
__device__ __forceinline__ void wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// what this workgroup stored itself, behind the release fence of the band that stored it
__device__ __forceinline__ int32_t wg_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool WP>
__device__ __forceinline__ void lp_run(const LpLaunch& a, const LpJobDev& job, const int c, int32_t* out,
                                       const size_t ostride, int32_t* sm, int32_t* s_pal) {
  const int l = (int)threadIdx.x;
  const int w = (int)job.w, h = (int)job.h;
  int32_t(*s_ring)[9] = reinterpret_cast<int32_t(*)[9]>(sm + kOffRing);
  int32_t(*s_idx)[C + 1] = reinterpret_cast<int32_t(*)[C + 1]>(sm + kOffIdx);
  int32_t(*s_val)[C + 1] = reinterpret_cast<int32_t(*)[C + 1]>(sm + kOffVal);
  int32_t(*s_above)[128] = reinterpret_cast<int32_t(*)[128]>(sm + kOffAbove);
  int32_t(*s_te)[9] = reinterpret_cast<int32_t(*)[9]>(sm + kOffTe);
  uint32_t(*s_e)[R + 2][9] = reinterpret_cast<uint32_t(*)[R + 2][9]>(sm + kOffE);
  int32_t(*s_state)[C] = reinterpret_cast<int32_t(*)[C]>(sm + kOffState);
  int32_t* s_above_te = sm + kOffAboveTe;
  uint32_t(*s_above_e)[128] = reinterpret_cast<uint32_t(*)[128]>(sm + kOffAboveE);
  uint32_t* s_div = reinterpret_cast<uint32_t*>(sm + kOffDiv);
  const int32_t* __restrict__ index = (job.index.space == kLpArena ? a.arena : a.scratch) + job.index.off;
  const size_t istride = job.index.stride;
  const int32_t* __restrict__ pal_g = a.arena + job.pal_off + (size_t)c * job.palette_size;
  const bool lds = job.lds != 0;
  const int ps = (int)job.palette_size, nd = (int)job.num_deltas, bd = a.bit_depth, predictor = (int)job.predictor;
  if (lds)
    for (int i = l; i < ps; i += R) s_pal[i] = pal_g[i];
  if constexpr (WP) s_div[l] = kWpDivLookup[l];
  // predictor state rows of a band's last row: two sets, written by one band and read by the next
  int32_t* wp_rows = a.scratch + job.wp_rows_off + (size_t)c * 10 * (size_t)w;
  const int mcol = l & 31, mrow0 = l >> 5;
  wave_sync();
  for (int y0 = 0; y0 < h; y0 += R) {
    const int rows = min(R, h - y0);
    const int y = y0 + l;
    const bool live = l < rows, below = y0 > 0;
    const bool publishes = WP && y0 + R < h;  // then rows == R and the band's last row is lane R - 1
    int32_t* wp_mine = wp_rows + (size_t)((y0 / R) & 1) * 5 * (size_t)w;
    const int32_t* wp_prev = wp_rows + (size_t)(((y0 / R) & 1) ^ 1) * 5 * (size_t)w;
    int32_t left_v = 0, leftleft_v = 0, te1 = 0;          // out[y][x - 1], out[y][x - 2], TE(x - 1, y)
    uint32_t e1[4] = {0, 0, 0, 0}, e2[4] = {0, 0, 0, 0};  // E(x - 1, y), E(x - 2, y)
    const int nsteps = w + 3 * (rows - 1);
    const int nchunks = (nsteps + C - 1) / C;
    // chunk k of row r = columns [k C - 3 r, k C - 3 r + C)
    int32_t nq[NI];  // the chunk after the current one, in flight
    auto fetch = [&](int k) {
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int r = mrow0 + 2 * i;
        const int xi = min(max(k * C - 3 * r + mcol, 0), w - 1);
        nq[i] = index[(size_t)min(y0 + r, h - 1) * istride + xi];
      }
    };
    // the indices leave their registers at once; the look-ups read them back from LDS in a rolled loop (32 unrolled
    // get_palette_value bodies next to the 32 loads in flight do not fit the register file)
    auto stage = [&]() {
#pragma unroll
      for (int i = 0; i < NI; i++) s_idx[mrow0 + 2 * i][mcol] = nq[i];
      if (lds) {
#pragma unroll 4
        for (int r = mrow0; r < R; r += 2) s_val[r][mcol] = palette_value(s_pal, 0, s_idx[r][mcol], c, ps, bd);
      } else {
#pragma unroll 4
        for (int r = mrow0; r < R; r += 2) s_val[r][mcol] = palette_value(pal_g, 0, s_idx[r][mcol], c, ps, bd);
      }
    };
    auto flush = [&](int k) {
#pragma unroll 4
      for (int i = 0; i < NI; i++) {
        const int r = mrow0 + 2 * i;
        const int x = k * C - 3 * r + mcol;
        if (r < rows && x >= 0 && x < w) out[(size_t)(y0 + r) * ostride + x] = s_val[r][mcol];
      }
      if constexpr (WP) {
        if (publishes) {  // the last row's predictor state of this chunk: 5 rows x 32 columns
          for (int t = l; t < 5 * C; t += R) {
            const int q = t >> 5, x = k * C - 3 * (R - 1) + (t & 31);
            if (x >= 0 && x < w) wp_mine[(size_t)q * w + x] = s_state[q][t & 31];
          }
        }
      }
    };
    fetch(0);
    stage();
    if (nchunks > 1) fetch(1);
    wave_sync();
    for (int k = 0; k < nchunks; k++) {
      const int s0 = k * C;
      if (below && (s0 & 63) == 0) {
        // columns this band's first rows touch during steps s0 .. s0 + 63: up to s0 + 66 (lane 0 copies column s + 3
        // during step s) -> [lo, hi) into the 128-column window
        const int lo = s0 == 0 ? 0 : s0 + 3, hi = min(w, s0 + 67);
        if (lo < hi) {
          constexpr int NR = WP ? 7 : 2;  // 2 output rows (+ TE + 4 E rows)
          for (int t = l; t < NR * (hi - lo); t += R) {
            const int r = t % NR, col = lo + t / NR;
            if (r < 2) {
              s_above[r][col & 127] = wg_load(&out[(size_t)(y0 - 1 - r) * ostride + col]);
            } else {
              const int32_t vv = wg_load(&wp_prev[(size_t)(r - 2) * w + col]);
              if (r == 2) s_above_te[col & 127] = vv;
              else s_above_e[r - 3][col & 127] = (uint32_t)vv;
            }
          }
          wave_sync();
        }
      }
      if (below && s0 == 0) {  // the rings' view of the rows above, for step 0: columns 0..2 / column 0
        if (l < 3) {
          s_ring[1][l] = s_above[0][l];
          if constexpr (WP) {
            s_te[1][l] = s_above_te[l];
#pragma unroll
            for (int q = 0; q < 4; q++) s_e[q][1][l] = s_above_e[q][l];
          }
        }
        if (l == 0) s_ring[0][0] = s_above[1][0];
        wave_sync();
      }
      const int send = min(C, nsteps - s0);
      for (int j = 0; j < send; j++) {
        const int s = s0 + j;
        const int x = s - 3 * l;
        const bool active = live && x >= 0 && x < w;
        // one batch of LDS reads, no branches: values that do not exist (first rows / columns) are read from valid
        // addresses and discarded by the selects
        const int32_t idx = s_idx[l][j];
        const int32_t ent = s_val[l][j];
        const int cm = (x - 1) & 7, c0 = x & 7, cp = (x + 1) & 7;
        const int32_t t_m1 = s_ring[l + 1][cm], t_0 = s_ring[l + 1][c0], t_p1 = s_ring[l + 1][cp], tt_0 = s_ring[l][c0];
        int32_t val;
        if constexpr (WP) {
          WpIn in;
          in.x = x, in.w = w, in.has_top = y > 0, in.has_toptop = y > 1;
          in.left_v = left_v, in.t_m1 = t_m1, in.t_0 = t_0, in.t_p1 = t_p1, in.tt_0 = tt_0;
          in.ta_m1 = s_te[l + 1][cm], in.ta_0 = s_te[l + 1][c0], in.ta_p1 = s_te[l + 1][cp], in.te1 = te1;
#pragma unroll
          for (int q = 0; q < 4; q++) {
            in.ea_m1[q] = s_e[q][l + 1][cm];
            in.ea_0[q] = s_e[q][l + 1][c0];
            in.ea_p1[q] = s_e[q][l + 1][cp];
            in.e1[q] = e1[q], in.e2[q] = e2[q];
          }
          const WpOut px = wp_pixel(job.wp, s_div, in, idx, nd, ent);
          val = px.val;
          if (active) {
            s_te[l + 2][c0] = px.te;
#pragma unroll
            for (int q = 0; q < 4; q++) {
              s_e[q][l + 2][c0] = px.e[q];
              e2[q] = e1[q];
              e1[q] = px.e[q];
            }
            if (publishes && l == R - 1) {
              s_state[0][j] = px.te;
#pragma unroll
              for (int q = 0; q < 4; q++) s_state[1 + q][j] = (int32_t)px.e[q];
            }
            te1 = px.te;
          }
        } else {
          const int32_t t_p2 = s_ring[l + 1][(x + 2) & 7];
          // PredictionData::get_rows, modular/predict.rs:96-128
          const int64_t left = x > 0 ? left_v : (y > 0 ? t_0 : 0);
          const int64_t top = y > 0 ? t_0 : left;
          const int64_t topleft = (x > 0 && y > 0) ? t_m1 : left;
          const int64_t topright = (x + 1 < w && y > 0) ? t_p1 : top;
          const int64_t leftleft = x > 1 ? leftleft_v : left;
          const int64_t toptop = y > 1 ? tt_0 : top;
          const int64_t toprightright = (x + 2 < w && y > 0) ? t_p2 : topright;
          const int64_t pred = predict_uniform(predictor, left, top, toptop, topleft, topright, leftleft, toprightright);
          val = idx < nd ? (int32_t)(uint32_t)(uint64_t)(pred + (int64_t)ent) : ent;
        }
        if (active) {
          s_val[l][j] = val;
          s_ring[l + 2][c0] = val;
          leftleft_v = left_v;
          left_v = val;
        }
        if (below && l == 0) {  // the rows above, one step ahead (columns past the row's end are never selected)
          const int ca = (s + 3) & 127, cr = (s + 3) & 7;
          s_ring[1][cr] = s_above[0][ca];
          s_ring[0][(s + 1) & 7] = s_above[1][(s + 1) & 127];
          if constexpr (WP) {
            s_te[1][cr] = s_above_te[ca];
#pragma unroll
            for (int q = 0; q < 4; q++) s_e[q][1][cr] = s_above_e[q][ca];
          }
        }
        wave_sync();
      }
      flush(k);
      if (k + 1 < nchunks) stage();  // chunk k + 1 (the flush's LDS reads are ahead of these writes in the queue)
      if (k + 2 < nchunks) fetch(k + 2);
      wave_sync();  // the staged chunk is visible; loads stay in flight
    }
    if (y0 + R < h) {
      // the band below re-reads this band's last two rows (and state rows): stores ordered at workgroup scope and landed
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
}

__global__ __launch_bounds__(kLpRows) void k_modular_local_palette(const LpLaunch a) {
  extern __shared__ int32_t lp_sm[];
  const LocalItem item = a.items[blockIdx.x];
  const LpJobDev& job = a.jobs[item.group];
  const int c = (int)item.row0;  // the output channel
  const uint32_t slot = job.out_slot[c];
  // (a select chain: indexing the kernel argument dynamically would copy it to scratch)
  int32_t* plane = slot == 0 ? a.out[0] : slot == 1 ? a.out[1] : slot == 2 ? a.out[2] : a.out[3];
  // ... and its row stride: a frame plane's and an extra channel's sample store differ (jxl_hip_local_extra.h)
  const size_t ostride = slot == 0 ? a.slot_stride[0] : slot == 1 ? a.slot_stride[1] : slot == 2 ? a.slot_stride[2] : a.slot_stride[3];
  int32_t* out = plane + (size_t)job.y0 * ostride + job.x0;  // no __restrict__: rows are read back
  int32_t* s_pal = lp_sm + (a.weighted ? kWpEnd : kDeltaEnd);
  if (job.predictor == 6) lp_run<true>(a, job, c, out, ostride, lp_sm, s_pal);
  else lp_run<false>(a, job, c, out, ostride, lp_sm, s_pal);
}

// kMixed: the slots' planes have strides of their own (slot_stride: colour planes beside extra channels); otherwise all
// share out_stride and one row offset serves the four
template <bool kMixed>
__global__ __launch_bounds__(256) void k_modular_local_phase(const LpLaunch a) {
  const LocalItem item = a.items[blockIdx.x];
  const LpPhaseDev& g = a.phases[item.group];
  const uint32_t w = g.w, nvx = (w + 3) >> 2;
  const uint32_t total = min(g.rows_per_item, g.h - item.row0) * nvx;  // (an item holds about 2048 four-sample vectors)
  for (uint32_t i = threadIdx.x; i < total; i += 256) {
    const uint32_t y = item.row0 + i / nvx, x = (i % nvx) * 4;
    const uint32_t cnt = min(4u, w - x);
    const size_t out_at = (size_t)(g.y0 + y) * a.out_stride + g.x0 + x;
    auto at = [&](int t) {
      if constexpr (kMixed) return (size_t)(g.y0 + y) * a.slot_stride[t] + g.x0 + x;
      else return out_at;
    };
    auto fetch = [&](int t) {
      const LpPlane& p = g.src[t];
      if (p.space == kLpNone) return make_int4(0, 0, 0, 0);
      if (p.space == kLpOut) return load_some(a.out[t] + at(t), cnt);
      return load_some((p.space == kLpArena ? a.arena : a.scratch) + p.off + (size_t)y * p.stride + x, cnt);
    };
    Slots s;
    s.r0 = fetch(0);
    s.r1 = fetch(1);
    s.r2 = fetch(2);
    s.r3 = fetch(3);
    for (uint32_t k = 0; k < g.n_ops; k++) {
      const LocalOpDev& op = g.ops[k];
      if (op.kind == JXLH_LOCAL_RCT) apply_rct(s, op);
      else apply_palette(s, op, a.arena + op.pal_off, a.bit_depth);
    }
    auto put = [&](int t, int4 v) {
      const LpPlane& p = g.dst[t];
      if (p.space == kLpOut) store_some(a.out[t] + at(t), v, cnt);
      else if (p.space == kLpScratch) store_some(a.scratch + p.off + (size_t)y * p.stride + x, v, cnt);
    };
    put(0, s.r0);
    put(1, s.r1);
    put(2, s.r2);
    put(3, s.r3);
    if (g.fan) {
      store_some(a.fan[0] + out_at, s.r0, cnt);  // (planes of slot 0's stride: out_stride)
      store_some(a.fan[1] + out_at, s.r0, cnt);
    }
  }
}

}  // namespace

size_t modular_local_palette_lds_bytes(bool weighted, bool lds_palette) {
  return sizeof(int32_t) * ((size_t)(weighted ? kWpEnd : kDeltaEnd) + (lds_palette ? kLpLdsEntries : 0));
}

void launch_modular_local_palette(hipStream_t s, const LpLaunch& a) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_modular_local_palette, dim3(a.n_items), dim3(kLpRows),
                     modular_local_palette_lds_bytes(a.weighted != 0, a.lds_palette != 0), s, a);
}

void launch_modular_local_phase(hipStream_t s, const LpLaunch& a) {
  if (a.n_items == 0) return;
  if (a.mixed) hipLaunchKernelGGL(k_modular_local_phase<true>, dim3(a.n_items), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_modular_local_phase<false>, dim3(a.n_items), dim3(256), 0, s, a);
}

}  // namespace jxlh
