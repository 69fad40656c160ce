// K4 RCT, K5 Palette and the sample conversions -- Modular transforms on whole i32 planes (the GPU does not tile:
// neighbour-border plumbing of transforms/step.rs vanishes).  All arithmetic is wrapping 32-bit, as in the
// reference's SIMD paths.  The inverse Squeeze lives in k_squeeze.hip and k_smooth_unsqueeze.hip.
//
// Reference: rct.rs:14-157; palette.rs:24-199.
#include "jxlh_internal.h"
#include "modular_convert_device.h"
#include "modular_ops_device.h"  // wadd / wsub, rct_op, rct_permute, kDeltaPalette, palette_value
#include "modular_predict_device.h"  // predict_one, WpParams, kWpDivLookup, wp_pixel

namespace jxlh {
namespace {

// perm: which output plane receives w0/w1/w2 (rct.rs:132-156)
template <int OP>
__global__ void k4_rct(int32_t* __restrict__ p0, int32_t* __restrict__ p1, int32_t* __restrict__ p2, size_t n,
                       int perm, size_t nvec) {
  int32_t* o[3];
  rct_permute<int32_t*>(perm, p0, p1, p2, o);
  // nvec = n / 4 when the three planes are 16-byte aligned (launch_rct), else 0: everything takes the scalar loop
  const size_t stride = (size_t)gridDim.x * blockDim.x;
#ifndef JXLH_RCT_NT
#define JXLH_RCT_NT true  // streamed once, in place: `nt` on both directions 0.29-0.34 -> 0.254-0.259 ms at 8192^2 x 3 (6.3 TB/s)
#endif
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const int4 a = gload_i4<JXLH_RCT_NT>(p0 + 4 * i);
    const int4 b = gload_i4<JXLH_RCT_NT>(p1 + 4 * i);
    const int4 c = gload_i4<JXLH_RCT_NT>(p2 + 4 * i);
    int4 x, y, z;
    rct_op<OP>(a.x, b.x, c.x, x.x, y.x, z.x);
    rct_op<OP>(a.y, b.y, c.y, x.y, y.y, z.y);
    rct_op<OP>(a.z, b.z, c.z, x.z, y.z, z.z);
    rct_op<OP>(a.w, b.w, c.w, x.w, y.w, z.w);
    gstore_i4<JXLH_RCT_NT>(o[0] + 4 * i, x);
    gstore_i4<JXLH_RCT_NT>(o[1] + 4 * i, y);
    gstore_i4<JXLH_RCT_NT>(o[2] + 4 * i, z);
  }
  // tail
  for (size_t i = nvec * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    int32_t x, y, z;
    rct_op<OP>(p0[i], p1[i], p2[i], x, y, z);
    o[0][i] = x;
    o[1][i] = y;
    o[2][i] = z;
  }
}

// the same on rows of w samples at a pitch of `stride` samples (padded planes: the padding is not touched); row y of
// the grid's y dimension and beyond, one sample per thread along x
template <int OP>
__global__ void k4_rct_rows(int32_t* __restrict__ p0, int32_t* __restrict__ p1, int32_t* __restrict__ p2, uint32_t w,
                            uint32_t h, size_t stride, int perm) {
  int32_t* o[3];
  rct_permute<int32_t*>(perm, p0, p1, p2, o);
  for (uint32_t y = blockIdx.y; y < h; y += gridDim.y) {
    const size_t row = (size_t)y * stride;
    for (uint32_t x = blockIdx.x * blockDim.x + threadIdx.x; x < w; x += gridDim.x * blockDim.x) {
      int32_t a, b, c;
      rct_op<OP>(p0[row + x], p1[row + x], p2[row + x], a, b, c);
      o[0][row + x] = a;
      o[1][row + x] = b;
      o[2][row + x] = c;
    }
  }
}

// ---- palette step with delta entries and / or a neighbour predictor (do_palette_step_general, palette.rs:228-251)
// Entries below num_deltas are ADDED to a prediction from already reconstructed neighbours (left, top row up to
// x + 2, the row above that): a raster-order dependency.  Pixel (x, y) can go once (x - 1, y) and (x + 2, y - 1)
// are done, so all pixels with the same x + 3y are independent -- a wavefront of w + 3h steps:
//  * a workgroup owns a band of kDeltaRows rows of one channel, lane l = row; at step s lane l handles x = s - 3l.
//    A row's recent outputs live in an LDS ring of 8 columns (the row below reads columns x - 1 .. x + 2, the one
//    after that column x, while the owner is writing x + 3 / x + 6), its own left / leftleft in registers; one
//    LDS-only barrier per step.
//  * bands are pipelined ACROSS workgroups: band k trails band k - 1 by 3 * kDeltaRows steps.  The producer
//    publishes its completed step count every kDeltaPublish steps (device-scope fence, then one store); the consumer
//    copies the next 64 columns of the two rows above it into LDS every 64 steps, after the counter says they are
//    final, with device-coherent loads (they bypass the CU's L1, which may hold the lines from before they were
//    written).  A waiting band only depends on bands with a lower block index, which were dispatched earlier.
constexpr int kDeltaRows = 256;
constexpr int kDeltaPublish = 32;

// `out` already holds the palette entry of every pixel (the parallel gather kernel ran first): the wavefront only
// adds the prediction where index < num_deltas.
//
// Global memory is touched in CHUNKS of kDeltaChunk steps, never inside a step.  A wave with loads and stores both
// outstanding has to drain everything (one in-order vmcnt, vmcnt(0)) whenever it needs a loaded value, so a per-step
// "load the column 8 steps ahead, store this column" costs a full memory round trip per step, prefetch or not --
// that, not the prediction, was the 0.7-1.6 us step of the first version.  Per chunk a lane now: stores the outputs of
// the previous chunk (LDS -> global), moves the next chunk's index / entry values from registers to LDS (they were
// requested a whole chunk ago) and requests the chunk after that.  Steps read and write LDS only (lane-private rows of
// 33 dwords: conflict-free).  Progress is published one chunk late, right before a chunk's stores are issued, when
// the previous chunk's stores have long been acknowledged: the fence is free.
constexpr int kDeltaChunk = 32;
static_assert(kDeltaPublish == kDeltaChunk, "progress is published per chunk");

template <int PREDICTOR>
__global__ __launch_bounds__(kDeltaRows) void k5_palette_delta(const int32_t* __restrict__ index, int w, int h,
                                                               int num_deltas, int32_t* out_base, int* progress_base) {
  constexpr int C = kDeltaChunk;
  // rows 0 / 1 of the ring are the two rows ABOVE the band (y0 - 2, y0 - 1), fed from s_above one step ahead by lane
  // 0, so that every lane reads its neighbours the same way, unconditionally and in one batch; lane l owns row l + 2
  __shared__ int32_t s_ring[kDeltaRows + 2][9];
  __shared__ int32_t s_idx[kDeltaRows][C + 1], s_ent[kDeltaRows][C + 1], s_outc[kDeltaRows][C + 1];
  __shared__ int32_t s_above[2][128];  // rows y0 - 1 and y0 - 2 (of the previous band), a window of 128 columns
  __shared__ int s_avail;
  const int c = blockIdx.x, band = blockIdx.y, nbands = gridDim.y, l = threadIdx.x;
  int32_t* out = out_base + (size_t)c * (size_t)w * h;  // no __restrict__: rows are read back
  int* progress = progress_base + (size_t)c * nbands;
  const int y0 = band * kDeltaRows;
  const int rows = min(kDeltaRows, h - y0);
  const int y = y0 + l;
  const bool live = l < rows;
  int32_t left_v = 0, leftleft_v = 0;  // out[y][x - 1], out[y][x - 2]
  const int nsteps = w + 3 * (rows - 1);
  const int nchunks = (nsteps + C - 1) / C;
  // steps the previous band (always kDeltaRows rows) takes; its last row finishes column x at step x + 3*(R-1)
  const int prod_steps = w + 3 * (kDeltaRows - 1);
  int avail = 0;  // completed (and stored) steps of the previous band, as last observed
  // Chunk k of row r = columns [k C - 3 r, k C - 3 r + C): 32 contiguous samples.  The chunk is moved TRANSPOSED:
  // thread t handles column t % 32 of rows t / 32 + 8 i, so that a wave instruction touches two 128-byte row segments
  // (a lane fetching its own row's samples costs the texture path one cache-line request per lane: ~0.25 us per
  // instruction, which was the whole step time); the LDS tiles turn rows back into lanes.  Columns outside the row
  // read the nearest valid one, rows below the image read its last row; neither is ever used.
  static_assert(C == 32 && kDeltaRows == 256, "the mover mapping below assumes 32-column chunks and 256-row bands");
  constexpr int NI = 32;  // rows per thread and chunk
  const int mcol = l & 31, mrow0 = l >> 5;
  int32_t nq_i[NI], nq_e[NI];  // the chunk after the current one, in flight
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const int r = mrow0 + 8 * i;
      const int xi = min(max(k * C - 3 * r + mcol, 0), w - 1);
      const size_t off = (size_t)min(y0 + r, h - 1) * w + xi;
      nq_i[i] = index[off];
      nq_e[i] = out[off];
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      s_idx[mrow0 + 8 * i][mcol] = nq_i[i];
      s_ent[mrow0 + 8 * i][mcol] = nq_e[i];
    }
  };
  auto flush = [&](int k) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const int r = mrow0 + 8 * i;
      const int x = k * C - 3 * r + mcol;
      // agent-scope (write-through) stores: the band below reads these rows from another XCD, whose L2 is not
      // coherent with this one's.  With plain stores every publish needs a release fence = a write-back of this
      // XCD's whole L2 (measured ~10 us per chunk, 60 % of a band's time); written through, "visible to the
      // agent" is simply "acknowledged", which the publish below waits for with vmcnt(0).
      if (r < rows && x >= 0 && x < w)
        __hip_atomic_store(&out[(size_t)(y0 + r) * w + x], s_outc[r][mcol], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  fetch(0);
  stage();
  if (nchunks > 1) fetch(1);
  __syncthreads();
  for (int k = 0; k < nchunks; k++) {
    const int s0 = k * C;
    if (band > 0 && (s0 & 63) == 0) {
      // columns this band's first rows touch during steps s0 .. s0 + 63: up to s0 + 66 -> copy [lo, hi)
      const int lo = s0 == 0 ? 0 : s0 + 3, hi = min(w, s0 + 67);  // lane 0 copies column s + 3 during step s
      if (lo < hi) {
        const int need = min(prod_steps, (hi - 1) + 3 * (kDeltaRows - 1) + 1);
        if (avail < need) {
          if (l == 0) {
            int v;
            while ((v = __hip_atomic_load(&progress[band - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) < need)
              __builtin_amdgcn_s_sleep(2);
            s_avail = v;
          }
          __syncthreads();
          avail = s_avail;
        }
        for (int t = l; t < 2 * (hi - lo); t += kDeltaRows) {
          const int r = t & 1, col = lo + (t >> 1);
          s_above[r][col & 127] =
              __hip_atomic_load(&out[(size_t)(y0 - 1 - r) * w + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
      }
    }
    if (band > 0 && s0 == 0) {  // the ring's view of the rows above, for step 0: columns 0..2 / column 0
      if (l < 3) s_ring[1][l] = s_above[0][l];
      if (l == 0) s_ring[0][0] = s_above[1][0];
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    const int send = min(C, nsteps - s0);
    for (int j = 0; j < send; j++) {
      const int s = s0 + j;
      const int x = s - 3 * l;
      // one batch of LDS reads, no branches: values that do not exist (first rows / columns) are read from valid
      // addresses and discarded by the selects below
      const int32_t idx = s_idx[l][j];
      const int32_t ent = s_ent[l][j];
      const int32_t t_m1 = s_ring[l + 1][(x - 1) & 7], t_0 = s_ring[l + 1][x & 7], t_p1 = s_ring[l + 1][(x + 1) & 7];
      const int32_t t_p2 = s_ring[l + 1][(x + 2) & 7], tt_0 = s_ring[l][x & 7];
      const bool active = live && x >= 0 && x < w;
      // PredictionData::get_rows, modular/predict.rs:96-128
      const int64_t left = x > 0 ? left_v : (y > 0 ? t_0 : 0);
      const int64_t top = y > 0 ? t_0 : left;
      const int64_t topleft = (x > 0 && y > 0) ? t_m1 : left;
      const int64_t topright = (x + 1 < w && y > 0) ? t_p1 : top;
      const int64_t leftleft = x > 1 ? leftleft_v : left;
      const int64_t toptop = y > 1 ? tt_0 : top;
      const int64_t toprightright = (x + 2 < w && y > 0) ? t_p2 : topright;
      const int64_t pred = predict_one<PREDICTOR>(left, top, toptop, topleft, topright, leftleft, toprightright);
      const int32_t val = idx < num_deltas ? (int32_t)(uint32_t)(uint64_t)(pred + (int64_t)ent) : ent;
      if (active) {
        s_outc[l][j] = val;
        s_ring[l + 2][x & 7] = val;
        leftleft_v = left_v;
        left_v = val;
      }
      if (band > 0 && l == 0) {  // the rows above, one step ahead (columns past the row's end are never selected)
        s_ring[1][(s + 3) & 7] = s_above[0][(s + 3) & 127];
        s_ring[0][(s + 1) & 7] = s_above[1][(s + 1) & 127];
      }
      // LDS writes of this step visible to the workgroup
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    // chunk boundary: what chunk k - 1 stored a whole chunk ago is what the band below may now read
    if (band + 1 < nbands && k > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's write-through stores of chunk k - 1 have landed
      __syncthreads();                                  // ... and every other thread's
      if (l == 0) __hip_atomic_store(&progress[band], s0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flush(k);
    if (k + 1 < nchunks) stage();  // chunk k + 1 (every lane is past its last read of chunk k: the step barriers)
    if (k + 2 < nchunks) fetch(k + 2);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the staged chunk is visible; loads stay in flight
  }
  if (band + 1 < nbands) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (l == 0) __hip_atomic_store(&progress[band], nsteps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- the same step with Predictor::Weighted (do_palette_step_general, palette.rs:200-227): EVERY pixel runs the
// self-correcting predictor (WeightedPredictorState::predict_and_property + update_errors, modular/predict.rs:312-517),
// delta entries are added to its prediction.  The predictor's state is, per pixel, the signed error TE of the final
// prediction and the four sub-predictors' absolute errors E[4]; pixel (x, y) reads TE / E of (x - 1 .. x + 1, y - 1)
// and of (x - 1, y), (x - 2, y).  The reference keeps two rows of them and ADDS E(x, y) into the previous row's slot
// x + 1 (:508-515), so that the "north" sum of the next pixel already contains its west neighbour's errors; here every
// row keeps its own E in the LDS ring next to its outputs and the lane adds its own E(x - 1, y) / E(x - 2, y) from
// registers: err_n = E(x, y-1) + E(x-1, y), err_nw = E(x-1, y-1) + E(x-2, y), err_ne = E(x+1, y-1), with the
// reference's edge rules (pos_nw = max(x-1, 0), pos_ne = min(x+1, w-1) index the SAME summed slots).  Same wavefront
// as k5_palette_delta (x + 3y), same band pipeline; a band's last row also publishes its TE / E row for the band below.

// wp_rows: per channel and band, five rows of w ints (TE, E0..E3 of the band's last row).
// Memory movement as in k5_palette_delta: chunks of 32 steps moved as coalesced row segments through LDS, neighbour and
// state reads in one unconditional batch (the rows above the band are fed into ring rows 0 / 1 one step ahead by lane
// 0), outputs and the published state row written through at agent scope.
__global__ __launch_bounds__(kDeltaRows) void k5_palette_wp(const int32_t* __restrict__ index, int w, int h,
                                                            int num_deltas, int32_t* out_base, int* progress_base,
                                                            int32_t* wp_rows_base, const WpParams P) {
  constexpr int C = kDeltaChunk;
  // ring row 0 / 1 = rows y0 - 2 / y0 - 1, lane l owns row l + 2 (s_te / s_e: row 1 = y0 - 1, lane l owns row l + 2)
  __shared__ int32_t s_ring[kDeltaRows + 2][9];
  __shared__ int32_t s_te[kDeltaRows + 2][9];
  __shared__ uint32_t s_e[4][kDeltaRows + 2][9];
  __shared__ int32_t s_idx[kDeltaRows][C + 1], s_ent[kDeltaRows][C + 1], s_outc[kDeltaRows][C + 1];
  __shared__ int32_t s_state[5][C];    // TE, E0..E3 of the band's last row for the current chunk
  __shared__ int32_t s_above[2][128];  // out rows y0 - 1 and y0 - 2 (of the previous band), a window of 128 columns
  __shared__ int32_t s_above_te[128];  // TE and E of row y0 - 1
  __shared__ uint32_t s_above_e[4][128];
  __shared__ int s_avail;
  // the division table in LDS: from constant memory each lookup is a global load on the step's dependent path (two
  // rounds per step, ~0.4 us each -- most of what this kernel's step cost over k5_palette_delta's)
  __shared__ uint32_t s_div[64];
  const int c = blockIdx.x, band = blockIdx.y, nbands = gridDim.y, l = threadIdx.x;
  if (l < 64) s_div[l] = kWpDivLookup[l];
  int32_t* out = out_base + (size_t)c * (size_t)w * h;
  int* progress = progress_base + (size_t)c * nbands;
  int32_t* wp_mine = wp_rows_base + ((size_t)c * nbands + band) * 5 * (size_t)w;        // written for the band below
  const int32_t* wp_prev = wp_rows_base + ((size_t)c * nbands + band - 1) * 5 * (size_t)w;  // read when band > 0
  const int y0 = band * kDeltaRows;
  const int rows = min(kDeltaRows, h - y0);
  const int y = y0 + l;
  const bool live = l < rows;
  const bool publishes = band + 1 < nbands;  // then rows == kDeltaRows and the last row is lane kDeltaRows - 1
  int32_t left_v = 0, te1 = 0;              // out[y][x - 1], TE(x - 1, y)
  uint32_t e1[4] = {0, 0, 0, 0}, e2[4] = {0, 0, 0, 0};  // E(x - 1, y), E(x - 2, y)
  const int nsteps = w + 3 * (rows - 1);
  const int nchunks = (nsteps + C - 1) / C;
  const int prod_steps = w + 3 * (kDeltaRows - 1);
  int avail = 0;
  static_assert(C == 32 && kDeltaRows == 256, "the mover mapping below assumes 32-column chunks and 256-row bands");
  constexpr int NI = 32;
  const int mcol = l & 31, mrow0 = l >> 5;
  int32_t nq_i[NI], nq_e[NI];
  auto fetch = [&](int k) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const int r = mrow0 + 8 * i;
      const int xi = min(max(k * C - 3 * r + mcol, 0), w - 1);
      const size_t off = (size_t)min(y0 + r, h - 1) * w + xi;
      nq_i[i] = index[off];
      nq_e[i] = out[off];
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      s_idx[mrow0 + 8 * i][mcol] = nq_i[i];
      s_ent[mrow0 + 8 * i][mcol] = nq_e[i];
    }
  };
  auto flush = [&](int k) {
#pragma unroll
    for (int i = 0; i < NI; i++) {
      const int r = mrow0 + 8 * i;
      const int x = k * C - 3 * r + mcol;
      if (r < rows && x >= 0 && x < w)
        __hip_atomic_store(&out[(size_t)(y0 + r) * w + x], s_outc[r][mcol], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (publishes && l < 5 * C) {  // the last row's predictor state of this chunk: 5 rows x 32 columns
      const int q = l >> 5, x = k * C - 3 * (kDeltaRows - 1) + mcol;
      if (x >= 0 && x < w)
        __hip_atomic_store(&wp_mine[(size_t)q * w + x], s_state[q][mcol], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  fetch(0);
  stage();
  if (nchunks > 1) fetch(1);
  __syncthreads();
  for (int k = 0; k < nchunks; k++) {
    const int s0 = k * C;
    if (band > 0 && (s0 & 63) == 0) {
      const int lo = s0 == 0 ? 0 : s0 + 3, hi = min(w, s0 + 67);  // lane 0 copies column s + 3 during step s
      if (lo < hi) {
        const int need = min(prod_steps, (hi - 1) + 3 * (kDeltaRows - 1) + 1);
        if (avail < need) {
          if (l == 0) {
            int v;
            while ((v = __hip_atomic_load(&progress[band - 1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) < need)
              __builtin_amdgcn_s_sleep(2);
            s_avail = v;
          }
          __syncthreads();
          avail = s_avail;
        }
        // 2 output rows + TE + 4 E rows of the columns [lo, hi), device-coherent loads
        for (int t = l; t < 7 * (hi - lo); t += kDeltaRows) {
          const int r = t % 7, col = lo + t / 7;
          if (r < 2) {
            s_above[r][col & 127] =
                __hip_atomic_load(&out[(size_t)(y0 - 1 - r) * w + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            const int32_t vv = __hip_atomic_load(&wp_prev[(size_t)(r - 2) * w + col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (r == 2) s_above_te[col & 127] = vv;
            else s_above_e[r - 3][col & 127] = (uint32_t)vv;
          }
        }
        __syncthreads();
      }
    }
    if (band > 0 && s0 == 0) {  // the rings' view of the row(s) above, for step 0: columns 0..2 / column 0
      if (l < 3) {
        s_ring[1][l] = s_above[0][l];
        s_te[1][l] = s_above_te[l];
#pragma unroll
        for (int q = 0; q < 4; q++) s_e[q][1][l] = s_above_e[q][l];
      }
      if (l == 0) s_ring[0][0] = s_above[1][0];
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    const int send = min(C, nsteps - s0);
    for (int j = 0; j < send; j++) {
      const int s = s0 + j;
      const int x = s - 3 * l;
      const bool active = live && x >= 0 && x < w;
      // one batch of LDS reads; what does not exist is read from valid addresses and discarded by the selects
      const int32_t idx = s_idx[l][j];
      const int32_t entry = s_ent[l][j];
      const int cm = (x - 1) & 7, c0 = x & 7, cp = (x + 1) & 7;
      const int32_t t_m1 = s_ring[l + 1][cm], t_0 = s_ring[l + 1][c0], t_p1 = s_ring[l + 1][cp], tt_0 = s_ring[l][c0];
      const int32_t ta_m1 = s_te[l + 1][cm], ta_0 = s_te[l + 1][c0], ta_p1 = s_te[l + 1][cp];
      uint32_t ea_m1[4], ea_0[4], ea_p1[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        ea_m1[q] = s_e[q][l + 1][cm];
        ea_0[q] = s_e[q][l + 1][c0];
        ea_p1[q] = s_e[q][l + 1][cp];
      }
      WpIn in;
      in.x = x, in.w = w, in.has_top = y > 0, in.has_toptop = y > 1;
      in.left_v = left_v, in.t_m1 = t_m1, in.t_0 = t_0, in.t_p1 = t_p1, in.tt_0 = tt_0;
      in.ta_m1 = ta_m1, in.ta_0 = ta_0, in.ta_p1 = ta_p1, in.te1 = te1;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        in.ea_m1[q] = ea_m1[q], in.ea_0[q] = ea_0[q], in.ea_p1[q] = ea_p1[q];
        in.e1[q] = e1[q], in.e2[q] = e2[q];
      }
      const WpOut px = wp_pixel(P, s_div, in, idx, num_deltas, entry);
      const int32_t val = px.val, te = px.te;
      uint32_t e[4];
#pragma unroll
      for (int q = 0; q < 4; q++) e[q] = px.e[q];
      if (active) {
        s_outc[l][j] = val;
        s_ring[l + 2][c0] = val;
        s_te[l + 2][c0] = te;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          s_e[q][l + 2][c0] = e[q];
          e2[q] = e1[q];
          e1[q] = e[q];
        }
        if (publishes && l == kDeltaRows - 1) {
          s_state[0][j] = te;
#pragma unroll
          for (int q = 0; q < 4; q++) s_state[1 + q][j] = (int32_t)e[q];
        }
        te1 = te;
        left_v = val;
      }
      if (band > 0 && l == 0) {  // the rows above, one step ahead (columns past the row's end are never selected)
        const int ca = (s + 3) & 127, cr = (s + 3) & 7;
        s_ring[1][cr] = s_above[0][ca];
        s_te[1][cr] = s_above_te[ca];
#pragma unroll
        for (int q = 0; q < 4; q++) s_e[q][1][cr] = s_above_e[q][ca];
        s_ring[0][(s + 1) & 7] = s_above[1][(s + 1) & 127];
      }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    if (publishes && k > 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's write-through stores of chunk k - 1 have landed
      __syncthreads();
      if (l == 0) __hip_atomic_store(&progress[band], s0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    flush(k);
    if (k + 1 < nchunks) stage();
    if (k + 2 < nchunks) fetch(k + 2);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  }
  if (publishes) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (l == 0) __hip_atomic_store(&progress[band], nsteps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// LDS_PAL: the explicit palette (num_colors x nb_channels entries, <= kPalLdsEntries) is staged in LDS
// once per workgroup (persistent grid), so the per-pixel gathers never leave the CU.
constexpr int kPalLdsEntries = 12288;  // 48 KB
template <bool LDS_PAL>
__global__ __launch_bounds__(256) void k5_palette(const int32_t* __restrict__ index, size_t n,
                                                  const int32_t* __restrict__ palette_g, int num_colors, size_t pstride_g,
                                                  int nb_channels, int bit_depth, int32_t* __restrict__ out,
                                                  size_t ostride, size_t nvec) {
  __shared__ int32_t s_pal[LDS_PAL ? kPalLdsEntries : 1];
  const int32_t* palette = palette_g;
  size_t pstride = pstride_g;
  if constexpr (LDS_PAL) {
    for (int i = threadIdx.x; i < num_colors * nb_channels; i += 256)
      s_pal[i] = palette_g[(size_t)(i / num_colors) * pstride_g + (i % num_colors)];
    __syncthreads();
    palette = s_pal;
    pstride = (size_t)num_colors;
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
#ifndef JXLH_PAL_NT
#define JXLH_PAL_NT true  // index read once, planes written once: 0.229 -> 0.224 ms at 8192^2
#endif
    const int4 idx = gload_i4<JXLH_PAL_NT>(index + 4 * i);
    for (int c = 0; c < nb_channels; c++) {
      int4 v;
      v.x = palette_value(palette, pstride, idx.x, c, num_colors, bit_depth);
      v.y = palette_value(palette, pstride, idx.y, c, num_colors, bit_depth);
      v.z = palette_value(palette, pstride, idx.z, c, num_colors, bit_depth);
      v.w = palette_value(palette, pstride, idx.w, c, num_colors, bit_depth);
      if ((ostride & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        gstore_i4<JXLH_PAL_NT>(out + (size_t)c * ostride + 4 * i, v);
      } else {  // channel planes are only 4-byte aligned
        int32_t* o = out + (size_t)c * ostride + i * 4;
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
      }
    }
  }
  for (size_t i = nvec * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t idx = index[i];
    for (int c = 0; c < nb_channels; c++)
      out[(size_t)c * ostride + i] = palette_value(palette, pstride, idx, c, num_colors, bit_depth);
  }
}

}  // namespace

void launch_rct(hipStream_t s, int32_t* p0, int32_t* p1, int32_t* p2, size_t n, int op, int perm) {
  if (n == 0) return;
  const unsigned grid = (unsigned)min((size_t)8192, (n / 4 + 255) / 256 + 1);
  // sub-ranges of planes (band-sharded runs) may start anywhere: vector accesses only for 16-byte aligned planes
  const bool aligned = ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2)) & 15) == 0;
  const size_t nvec = aligned ? n / 4 : 0;
  switch (op) {
    case 0: hipLaunchKernelGGL(k4_rct<0>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    case 1: hipLaunchKernelGGL(k4_rct<1>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    case 2: hipLaunchKernelGGL(k4_rct<2>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    case 3: hipLaunchKernelGGL(k4_rct<3>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    case 4: hipLaunchKernelGGL(k4_rct<4>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    case 5: hipLaunchKernelGGL(k4_rct<5>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
    default: hipLaunchKernelGGL(k4_rct<6>, dim3(grid), dim3(256), 0, s, p0, p1, p2, n, perm, nvec); break;
  }
}

void launch_rct_rows(hipStream_t s, int32_t* p0, int32_t* p1, int32_t* p2, uint32_t w, uint32_t h, size_t stride, int op,
                     int perm) {
  if (w == 0 || h == 0) return;
  const dim3 grid(min(64u, (w + 255) / 256), min(h, 16384u));  // ONE launch whatever the row count
  switch (op) {
    case 0: hipLaunchKernelGGL(k4_rct_rows<0>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    case 1: hipLaunchKernelGGL(k4_rct_rows<1>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    case 2: hipLaunchKernelGGL(k4_rct_rows<2>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    case 3: hipLaunchKernelGGL(k4_rct_rows<3>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    case 4: hipLaunchKernelGGL(k4_rct_rows<4>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    case 5: hipLaunchKernelGGL(k4_rct_rows<5>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
    default: hipLaunchKernelGGL(k4_rct_rows<6>, grid, dim3(256), 0, s, p0, p1, p2, w, h, stride, perm); break;
  }
}

void launch_palette(hipStream_t s, const int32_t* index, size_t n, const int32_t* palette, int num_colors,
                    size_t palette_stride, int nb_channels, int bit_depth, int32_t* out, size_t out_channel_stride) {
  if (n == 0) return;
  const size_t ostride = out_channel_stride ? out_channel_stride : n;
  const size_t nvec = (reinterpret_cast<uintptr_t>(index) & 15) == 0 ? n / 4 : 0;  // int4 index loads need alignment
  if (num_colors > 0 && (size_t)num_colors * nb_channels <= (size_t)kPalLdsEntries) {
    // persistent grid (the palette is staged once per workgroup): 3 workgroups of 48 KB LDS per CU
    const unsigned grid = (unsigned)min((size_t)768, (n / 4 + 255) / 256 + 1);
    hipLaunchKernelGGL(k5_palette<true>, dim3(grid), dim3(256), 0, s, index, n, palette, num_colors, palette_stride,
                       nb_channels, bit_depth, out, ostride, nvec);
  } else {
    const unsigned grid = (unsigned)min((size_t)8192, (n + 255) / 256);
    hipLaunchKernelGGL(k5_palette<false>, dim3(grid), dim3(256), 0, s, index, n, palette, num_colors, palette_stride,
                       nb_channels, bit_depth, out, ostride, nvec);
  }
}

// progress: nb_channels * palette_delta_bands(h) ints of device scratch
int palette_delta_bands(int h) { return (h + kDeltaRows - 1) / kDeltaRows; }
// Weighted predictor: header = p1c, p2c, p3ca..p3ce, w0..w3; wp_rows: nb_channels * bands * 5 * w ints of scratch
void launch_palette_wp(hipStream_t s, const int32_t* index, int w, int h, const int32_t* palette, int num_colors,
                       int num_deltas, size_t palette_stride, int nb_channels, int bit_depth, const uint32_t header[11],
                       int32_t* out, int* progress, int32_t* wp_rows) {
  if (w <= 0 || h <= 0) return;
  launch_palette(s, index, (size_t)w * h, palette, num_colors + num_deltas, palette_stride, nb_channels, bit_depth, out);
  const int nbands = palette_delta_bands(h);
  (void)hipMemsetAsync(progress, 0, sizeof(int) * (size_t)nb_channels * nbands, s);
  WpParams P;
  P.p1c = (int32_t)header[0];
  P.p2c = (int32_t)header[1];
  for (int i = 0; i < 5; i++) P.p3c[i] = (int32_t)header[2 + i];
  for (int i = 0; i < 4; i++) P.w[i] = header[7 + i];
  hipLaunchKernelGGL(k5_palette_wp, dim3(nb_channels, nbands), dim3(kDeltaRows), 0, s, index, w, h, num_deltas, out,
                     progress, wp_rows, P);
}

void launch_palette_delta(hipStream_t s, const int32_t* index, int w, int h, const int32_t* palette, int num_colors,
                          int num_deltas, size_t palette_stride, int nb_channels, int bit_depth, int predictor,
                          int32_t* out, int* progress) {
  if (w <= 0 || h <= 0) return;
  // every pixel's palette entry, in parallel (get_palette_value with palette_size = num_colors + num_deltas) ...
  launch_palette(s, index, (size_t)w * h, palette, num_colors + num_deltas, palette_stride, nb_channels, bit_depth, out);
  if (num_deltas <= 0 && predictor == 0) return;
  // ... then the wavefront adds the predictions (entries below num_deltas, incl. the implicit negative indices)
  const int nbands = palette_delta_bands(h);
  (void)hipMemsetAsync(progress, 0, sizeof(int) * (size_t)nb_channels * nbands, s);
  const dim3 grid(nb_channels, nbands), block(kDeltaRows);
#define JXLH_DELTA(P) \
  case P: hipLaunchKernelGGL(k5_palette_delta<P>, grid, block, 0, s, index, w, h, num_deltas, out, progress); break
  switch (predictor) {
    JXLH_DELTA(0); JXLH_DELTA(1); JXLH_DELTA(2); JXLH_DELTA(3); JXLH_DELTA(4); JXLH_DELTA(5); JXLH_DELTA(7);
    JXLH_DELTA(8); JXLH_DELTA(9); JXLH_DELTA(10); JXLH_DELTA(11); JXLH_DELTA(12); JXLH_DELTA(13);
    default: break;
  }
#undef JXLH_DELTA
}

namespace {
// ConvertI32ToU8Stage x3 (render/stages/convert.rs:672-691) + interleave: 4 pixels per thread
template <int CH>
__global__ __launch_bounds__(256) void k_i32_to_rgb8(const int32_t* __restrict__ p0, const int32_t* __restrict__ p1,
                                                     const int32_t* __restrict__ p2, size_t stride, int w, int h,
                                                     int32_t mult, int32_t maxv, uint8_t* __restrict__ out,
                                                     size_t out_stride) {
  const int x4 = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int y = blockIdx.y;
  if (x4 >= w || y >= h) return;
  const int32_t* __restrict__ pl[3] = {p0, p1, p2};
  uint32_t q[4][3];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int32_t v = x4 + i < w ? pl[c][(size_t)y * stride + x4 + i] : 0;
      const int32_t scaled = (int32_t)((uint32_t)v * (uint32_t)mult);
      const int32_t zeroclip = scaled < 0 ? 0 : scaled;
      q[i][c] = (uint32_t)(scaled > maxv ? maxv : zeroclip) & 0xffu;
    }
  uint8_t* o = out + (size_t)y * out_stride + (size_t)x4 * CH;
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (x4 + i < w) {
      o[i * CH] = (uint8_t)q[i][0];
      o[i * CH + 1] = (uint8_t)q[i][1];
      o[i * CH + 2] = (uint8_t)q[i][2];
      if constexpr (CH == 4) o[i * CH + 3] = 255;
    }
}

// ConvertModularToF32Stage, integer samples (convert.rs:488-533)
__global__ void k_modular_to_f32(const int32_t* __restrict__ in, size_t n, float scale, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (float)in[i] * scale;
}
// ConvertModularToF32Stage, floating-point samples (convert.rs:416-486 int_to_float / int_to_float_generic): a `bits`-bit
// float with `exp_bits` exponent bits stored in an integer -> binary32.  The generic form covers the reference's two
// fast paths as well: binary32 passes through bit for bit, binary16 widens exactly like the hardware conversion
// (signalling NaNs keep their payload here; the reference's f16 SIMD path quiets them).
__global__ void k_float_samples_to_f32(const int32_t* __restrict__ in, size_t n, uint32_t bits, uint32_t exp_bits,
                                       float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = float_sample_to_f32((uint32_t)in[i], bits, exp_bits);
}
// ConvertModularXYBToF32Stage (convert.rs:306-343)
__global__ void k_modular_xyb_to_f32(const int32_t* __restrict__ y, const int32_t* __restrict__ x,
                                     const int32_t* __restrict__ b, size_t n, float sx, float sy, float sb,
                                     float* __restrict__ ox, float* __restrict__ oy, float* __restrict__ ob) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float fy = (float)y[i];
  ox[i] = (float)x[i] * sx;
  oy[i] = fy * sy;
  ob[i] = ((float)b[i] + fy) * sb;
}
}  // namespace

void launch_i32_to_rgb8(hipStream_t s, const int32_t* const planes[3], size_t stride, int w, int h, int32_t mult,
                        int32_t maxv, int channels, uint8_t* out, size_t out_stride) {
  if (w <= 0 || h <= 0) return;
  const dim3 grid(((w + 3) / 4 + 255) / 256, h);
  if (channels == 3)
    hipLaunchKernelGGL(k_i32_to_rgb8<3>, grid, dim3(256), 0, s, planes[0], planes[1], planes[2], stride, w, h, mult, maxv,
                       out, out_stride);
  else
    hipLaunchKernelGGL(k_i32_to_rgb8<4>, grid, dim3(256), 0, s, planes[0], planes[1], planes[2], stride, w, h, mult, maxv,
                       out, out_stride);
}
void launch_modular_to_f32(hipStream_t s, const int32_t* in, size_t n, float scale, float* out) {
  if (n) hipLaunchKernelGGL(k_modular_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n, scale, out);
}
void launch_float_samples_to_f32(hipStream_t s, const int32_t* in, size_t n, uint32_t bits, uint32_t exp_bits, float* out) {
  if (n)
    hipLaunchKernelGGL(k_float_samples_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, n, bits, exp_bits, out);
}
void launch_modular_xyb_to_f32(hipStream_t s, const int32_t* y, const int32_t* x, const int32_t* b, size_t n,
                               const float scale[3], float* ox, float* oy, float* ob) {
  if (n)
    hipLaunchKernelGGL(k_modular_xyb_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, x, b, n, scale[0],
                       scale[1], scale[2], ox, oy, ob);
}

}  // namespace jxlh
