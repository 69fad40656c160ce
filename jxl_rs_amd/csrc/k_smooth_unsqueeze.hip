// Smooth unsqueeze: what a squeeze step runs while its residual channel has not arrived (progressive previews;
// transforms/step.rs:138-150 picks the kind, :841-851 dispatches): smooth_h / smooth_v / smooth_2d_unsqueeze
// (squeeze.rs:908-1225).  A pure 5x5 stencil on the average channel -- unlike the regular step there is no
// recurrence, so it is one thread per column of a 64 x 32 tile of average samples, walking eight rows with a sliding window; the
// tile's 68 x 36 window is staged through LDS once.  Three kernels over one tile body: a rectangle of one plane
// (jxlh_smooth_unsqueeze), whole channels with the plane in blockIdx.z, and three channels with the inverse RCT applied
// in registers (jxlh_unsqueeze_chain_preview).
// Arithmetic order is the reference's (four partial sums of <= 4 FMAs from zero, (a + b) + (c + d), +-0.5,
// truncating convert: the scalar / NEON / wasm as_i32; the x86 back-ends' cvtps rounds a second time, see
// DESIGN.md 4).
#include "jxlh_internal.h"
#include "modular_ops_device.h"  // rct_op, rct_permute

namespace jxlh {

struct SmTap {
  int n;
  float w;
};
#define SW2 0.62646443f
#define SW10 0.24413736f
#define SW18 0.06118795f
#define SW26 -0.01328634f
#define SW34 -0.03355509f
#define SW50 -0.02015225f
#define SW58 -0.01033307f
#define SW74 -0.00056067f
#define SV1 0.69472290f
#define SV9 0.27861324f
#define SV17 0.07666797f
#define SV25 -0.00778371f
#define SV41 -0.03143468f
#define SV49 -0.02150597f
#define SV65 -0.00434251f
#define SV73 -0.00078780f
// n < 0: the slot is empty (the 2-D kernel's third partial sum has three taps)
__device__ static constexpr SmTap kSm2d[4][16] = {
    {{1, SW58}, {2, SW50}, {3, SW74}, {5, SW58}, {6, SW18}, {7, SW10}, {8, SW34}, {10, SW50},
     {11, SW10}, {12, SW2}, {13, SW26}, {-1, 0.f}, {15, SW74}, {16, SW34}, {17, SW26}, {18, SW50}},
    {{1, SW74}, {2, SW50}, {3, SW58}, {6, SW34}, {7, SW10}, {8, SW18}, {9, SW58}, {11, SW26},
     {12, SW2}, {13, SW10}, {14, SW50}, {-1, 0.f}, {16, SW50}, {17, SW26}, {18, SW34}, {19, SW74}},
    {{5, SW74}, {6, SW34}, {7, SW26}, {8, SW50}, {10, SW50}, {11, SW10}, {12, SW2}, {13, SW26},
     {15, SW58}, {16, SW18}, {17, SW10}, {-1, 0.f}, {18, SW34}, {21, SW58}, {22, SW50}, {23, SW74}},
    {{6, SW50}, {7, SW26}, {8, SW34}, {9, SW74}, {11, SW26}, {12, SW2}, {13, SW10}, {14, SW50},
     {16, SW34}, {17, SW10}, {18, SW18}, {-1, 0.f}, {19, SW58}, {21, SW74}, {22, SW50}, {23, SW58}}};
__device__ static constexpr SmTap kSm1d[2][16] = {
    {{1, SV73}, {2, SV65}, {5, SV65}, {6, SV25}, {7, SV17}, {8, SV41}, {10, SV49}, {11, SV9},
     {12, SV1}, {13, SV25}, {15, SV65}, {16, SV25}, {17, SV17}, {18, SV41}, {21, SV73}, {22, SV65}},
    {{2, SV65}, {3, SV73}, {6, SV41}, {7, SV17}, {8, SV25}, {9, SV65}, {11, SV25}, {12, SV1},
     {13, SV9}, {14, SV49}, {16, SV41}, {17, SV17}, {18, SV25}, {19, SV65}, {22, SV65}, {23, SV73}}};

// RNE: the x86 back-ends' as_i32 (cvtps2dq: round to nearest even, jxl_simd/src/x86_64/avx.rs:580) instead of the
// truncation of the scalar / NEON / wasm ones (scalar.rs:178): what a reference build running on an x86 host produces
template <bool TWO_D, int WHICH, bool RNE>
__device__ __forceinline__ int32_t smooth_eval(const float (&n)[25]) {
  float part[4];
#pragma unroll
  for (int g = 0; g < 4; g++) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      constexpr const SmTap* t = TWO_D ? kSm2d[WHICH] : kSm1d[WHICH & 1];
      const SmTap tp = t[4 * g + k];
      if (tp.n >= 0) acc = __fmaf_rn(n[tp.n], tp.w, acc);
    }
    part[g] = acc;
  }
  const float sum = __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3]));
  const float biased = __fadd_rn(sum, copysignf(0.5f, sum));
  return RNE ? (int32_t)rintf(biased) : (int32_t)biased;
}

#define JXLH_SM_TX 64
#define JXLH_SM_WAVES 4
#define JXLH_SM_RPT 8                                 // consecutive rows one thread walks with a sliding window
#define JXLH_SM_TY (JXLH_SM_WAVES * JXLH_SM_RPT)      // average rows per workgroup: 36 window rows for 32 (1.125x)
// KIND 0: horizontal (out = 2 in_x), 1: vertical, 2: both.  nx x ny = average samples the rectangle covers.
// One workgroup's tile of NCH planes of one geometry: NCH == 1 is a plane on its own; NCH == 3 stages the three
// channels' windows, a thread produces the same output samples of all three, and the inverse RCT (`op`, the planes of
// `out` already permuted: out[k] receives w_k) runs on them in registers before the one store.
// pair: base and stride keep every sample pair 8-byte aligned.  The tile's first average sample in the rectangle comes
// from blockIdx.x / .y (whole planes, rectangles) or, LISTED, from the caller (listed cells: the cell's own tile count)
struct SmoothGeom {
  size_t in_stride, out_stride;
  int in_w, in_h, cx0, cy0, out_w, out_h, nx, ny;
};
__device__ __forceinline__ void smooth_rct(int op, int32_t& a, int32_t& b, int32_t& c) {
  const int32_t v0 = a, v1 = b, v2 = c;
  switch (op) {  // wave-uniform
    case 0: break;
    case 1: rct_op<1>(v0, v1, v2, a, b, c); break;
    case 2: rct_op<2>(v0, v1, v2, a, b, c); break;
    case 3: rct_op<3>(v0, v1, v2, a, b, c); break;
    case 4: rct_op<4>(v0, v1, v2, a, b, c); break;
    case 5: rct_op<5>(v0, v1, v2, a, b, c); break;
    default: rct_op<6>(v0, v1, v2, a, b, c); break;
  }
}
template <int KIND, bool RNE, int NCH, bool LISTED = false>
__device__ __forceinline__ void smooth_tile(float (&tile)[NCH][JXLH_SM_TY + 4][JXLH_SM_TX + 4 + 1], const int32_t* const (&in)[NCH],
                                            int32_t* const (&out)[NCH], const SmoothGeom& g, bool pair, int op, int listed_bx = 0,
                                            int listed_by = 0) {
  const int tid = threadIdx.x;
  const int bx = LISTED ? listed_bx : blockIdx.x * JXLH_SM_TX, by = LISTED ? listed_by : blockIdx.y * JXLH_SM_TY;
  // The window, (TY + 4) x (TX + 4) samples per plane, is fetched as a flat list, thread t taking samples t, t + 256, ...:
  // no branch between the loads, so all of a thread's fetches are in flight before the first is written to LDS (one
  // wave per row with lanes 0..3 fetching the extra columns under a branch waited for every load in turn).  The last
  // round's surplus threads repeat the last sample.  Rows mirror ( -1 -> 0, h -> h - 1 ), columns clamp:
  // load_row_to_scratch, step.rs:386-416
  const int wave = __builtin_amdgcn_readfirstlane(tid / JXLH_SM_TX), lane = tid % JXLH_SM_TX;
  constexpr int WIN_W = JXLH_SM_TX + 4, WIN_N = WIN_W * (JXLH_SM_TY + 4), NT = JXLH_SM_TX * JXLH_SM_WAVES;
  constexpr int ROUNDS = (WIN_N + NT - 1) / NT;
  int32_t fetched[ROUNDS][NCH];
#pragma unroll
  for (int i = 0; i < ROUNDS; i++) {
    const int idx = min(tid + i * NT, WIN_N - 1), r = idx / WIN_W, c = idx - r * WIN_W;
    int y = g.cy0 + by + r - 2;
    y = g.in_h == 1 ? 0 : (y < 0 ? -y - 1 : (y >= g.in_h ? 2 * g.in_h - 1 - y : y));
    y = min(max(y, 0), g.in_h - 1);  // only rows no live thread reads can still be outside
    const int x = min(max(g.cx0 + bx + c - 2, 0), g.in_w - 1);
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) fetched[i][ch] = in[ch][(size_t)y * g.in_stride + x];
  }
#pragma unroll
  for (int i = 0; i < ROUNDS; i++) {
    const int idx = min(tid + i * NT, WIN_N - 1), r = idx / WIN_W, c = idx - r * WIN_W;
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) tile[ch][r][c] = (float)fetched[i][ch];
  }
  __syncthreads();
  const int ix = bx + lane;
  if (ix >= g.nx) return;
  const bool both = 2 * ix + 1 < g.out_w;
  float win[NCH][5][5];  // window rows; the first four are loaded once, then one new row per step
#pragma unroll
  for (int ch = 0; ch < NCH; ch++)
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 5; c++) win[ch][r][c] = tile[ch][wave * JXLH_SM_RPT + r][lane + c];
#pragma unroll
  for (int k = 0; k < JXLH_SM_RPT; k++) {
    const int ly = wave * JXLH_SM_RPT + k, iy = by + ly;
    if (iy >= g.ny) return;  // wave-uniform
    // v[ch]: KIND 2: the 2 x 2 outputs row by row; KIND 0: the pair along x; KIND 1: the pair along y
    int32_t v[NCH][KIND == 2 ? 4 : 2];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
#pragma unroll
      for (int c = 0; c < 5; c++) win[ch][4][c] = tile[ch][ly + 4][lane + c];
      float n[25];
#pragma unroll
      for (int r = 0; r < 5; r++)
#pragma unroll
        for (int c = 0; c < 5; c++) n[KIND == 1 ? 5 * c + r : 5 * r + c] = win[ch][r][c];
      if constexpr (KIND == 2) {
        v[ch][0] = smooth_eval<true, 0, RNE>(n);
        v[ch][1] = smooth_eval<true, 1, RNE>(n);
        v[ch][2] = smooth_eval<true, 2, RNE>(n);
        v[ch][3] = smooth_eval<true, 3, RNE>(n);
      } else {
        v[ch][0] = smooth_eval<false, 0, RNE>(n);
        v[ch][1] = smooth_eval<false, 1, RNE>(n);
      }
    }
    if constexpr (NCH == 3) {
#pragma unroll
      for (int j = 0; j < (KIND == 2 ? 4 : 2); j++) smooth_rct(op, v[0][j], v[1][j], v[2][j]);
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
      if constexpr (KIND == 2) {
        int32_t* p0 = out[ch] + (size_t)(2 * iy) * g.out_stride + 2 * ix;
        if (pair && both) {
          *(int2*)p0 = make_int2(v[ch][0], v[ch][1]);
          if (2 * iy + 1 < g.out_h) *(int2*)(p0 + g.out_stride) = make_int2(v[ch][2], v[ch][3]);
        } else {
          p0[0] = v[ch][0];
          if (both) p0[1] = v[ch][1];
          if (2 * iy + 1 < g.out_h) {
            p0[g.out_stride] = v[ch][2];
            if (both) p0[g.out_stride + 1] = v[ch][3];
          }
        }
      } else if constexpr (KIND == 0) {
        int32_t* p = out[ch] + (size_t)iy * g.out_stride + 2 * ix;
        if (pair && both) {
          *(int2*)p = make_int2(v[ch][0], v[ch][1]);
        } else {
          p[0] = v[ch][0];
          if (both) p[1] = v[ch][1];
        }
      } else {
        int32_t* p = out[ch] + (size_t)(2 * iy) * g.out_stride + ix;
        p[0] = v[ch][0];
        if (2 * iy + 1 < g.out_h) p[g.out_stride] = v[ch][1];
      }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ch++)
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 5; c++) win[ch][r][c] = win[ch][r + 1][c];
  }
}

// a rectangle of one plane (jxlh_smooth_unsqueeze)
template <int KIND, bool PAIR, bool RNE>
__global__ __launch_bounds__(JXLH_SM_TX* JXLH_SM_WAVES) void k6_smooth_unsqueeze(
    const int32_t* __restrict__ in, size_t in_stride, int in_w, int in_h, int cx0, int cy0, int32_t* __restrict__ out,
    size_t out_stride, int out_w, int out_h, int nx, int ny) {
  __shared__ float tile[1][JXLH_SM_TY + 4][JXLH_SM_TX + 4 + 1];
  const int32_t* const iv[1] = {in};
  int32_t* const ov[1] = {out};
  smooth_tile<KIND, RNE, 1>(tile, iv, ov, SmoothGeom{in_stride, out_stride, in_w, in_h, cx0, cy0, out_w, out_h, nx, ny}, PAIR, 0);
}

// whole channels of a preview chain (jxlh_unsqueeze_chain_preview): the plane in blockIdx.z
struct SmoothPlanes {
  const int32_t* in[3];
  int32_t* out[3];
};
template <int KIND, bool RNE>
__global__ __launch_bounds__(JXLH_SM_TX* JXLH_SM_WAVES) void k6_smooth_unsqueeze_planes(const SmoothPlanes pl, const SmoothGeom g,
                                                                                         int pair) {
  __shared__ float tile[1][JXLH_SM_TY + 4][JXLH_SM_TX + 4 + 1];
  const int32_t* const iv[1] = {pl.in[blockIdx.z]};
  int32_t* const ov[1] = {pl.out[blockIdx.z]};
  smooth_tile<KIND, RNE, 1>(tile, iv, ov, g, pair != 0, 0);
}
// ... the last level with the RCT behind it: three planes, 3 x 36 x 69 floats of LDS
template <int KIND, bool RNE>
__global__ __launch_bounds__(JXLH_SM_TX* JXLH_SM_WAVES) void k6_smooth_unsqueeze_rct(const SmoothPlanes pl, const SmoothGeom g, int pair,
                                                                                      int op) {
  __shared__ float tile[3][JXLH_SM_TY + 4][JXLH_SM_TX + 4 + 1];
  const int32_t* const iv[3] = {pl.in[0], pl.in[1], pl.in[2]};
  int32_t* const ov[3] = {pl.out[0], pl.out[1], pl.out[2]};
  smooth_tile<KIND, RNE, 3>(tile, iv, ov, g, pair != 0, op);
}

void launch_smooth_unsqueeze(hipStream_t s, int kind, const int32_t* in, size_t in_stride, int in_w, int in_h, int x0,
                             int y0, int32_t* out, size_t out_stride, int out_w, int out_h, bool cvt_rne) {
  const bool fx = kind != 1, fy = kind != 0;
  // the reference returns with the output untouched when the rectangle has no complete pair (squeeze.rs:921-923)
  if ((fx ? out_w / 2 : out_w) == 0 || (fy ? out_h / 2 : out_h) == 0) return;
  const int nx = fx ? (out_w + 1) / 2 : out_w, ny = fy ? (out_h + 1) / 2 : out_h;
  const int cx0 = fx ? x0 / 2 : x0, cy0 = fy ? y0 / 2 : y0;
  const dim3 grid((nx + JXLH_SM_TX - 1) / JXLH_SM_TX, (ny + JXLH_SM_TY - 1) / JXLH_SM_TY);
  const dim3 block(JXLH_SM_TX * JXLH_SM_WAVES);
  const bool pair = (uintptr_t)out % 8 == 0 && out_stride % 2 == 0;
#define JXLH_SM_LAUNCH1(K, P, R)                                                                                    \
  hipLaunchKernelGGL((k6_smooth_unsqueeze<K, P, R>), grid, block, 0, s, in, in_stride, in_w, in_h, cx0, cy0, out,   \
                     out_stride, out_w, out_h, nx, ny)
#define JXLH_SM_LAUNCH(K, P)                  \
  do {                                        \
    if (cvt_rne) JXLH_SM_LAUNCH1(K, P, true); \
    else JXLH_SM_LAUNCH1(K, P, false);        \
  } while (0)
  if (kind == 0) {
    if (pair) JXLH_SM_LAUNCH(0, true); else JXLH_SM_LAUNCH(0, false);
  } else if (kind == 1) {
    JXLH_SM_LAUNCH(1, false);
  } else {
    if (pair) JXLH_SM_LAUNCH(2, true); else JXLH_SM_LAUNCH(2, false);
  }
#undef JXLH_SM_LAUNCH
#undef JXLH_SM_LAUNCH1
}

// whole channels: kind JXLH_SMOOTH_*; op < 0: n_planes (<= 3) planes on their own; else three planes + the inverse RCT
void launch_smooth_unsqueeze_planes(hipStream_t s, int kind, int n_planes, const int32_t* const in[], size_t in_stride, int in_w,
                                    int in_h, int32_t* const out[], size_t out_stride, int out_w, int out_h, bool cvt_rne, int op,
                                    int perm) {
  const bool fx = kind != 1, fy = kind != 0;
  if ((fx ? out_w / 2 : out_w) == 0 || (fy ? out_h / 2 : out_h) == 0) return;
  const SmoothGeom g{in_stride, out_stride, in_w, in_h, 0, 0, out_w, out_h, fx ? (out_w + 1) / 2 : out_w, fy ? (out_h + 1) / 2 : out_h};
  SmoothPlanes pl{};
  bool pair = out_stride % 2 == 0 && kind != 1;
  for (int p = 0; p < n_planes; p++) {
    pl.in[p] = in[p];
    pl.out[p] = out[p];
    pair = pair && (uintptr_t)out[p] % 8 == 0;
  }
  if (op >= 0) rct_permute<int32_t*>(perm, out[0], out[1], out[2], pl.out);  // which plane receives w0 / w1 / w2 (as k4_rct)
  const dim3 grid((g.nx + JXLH_SM_TX - 1) / JXLH_SM_TX, (g.ny + JXLH_SM_TY - 1) / JXLH_SM_TY, op >= 0 ? 1 : n_planes);
  const dim3 block(JXLH_SM_TX * JXLH_SM_WAVES);
#define JXLH_SM_LAUNCH(K, R)                                                                                      \
  do {                                                                                                            \
    if (op >= 0) hipLaunchKernelGGL((k6_smooth_unsqueeze_rct<K, R>), grid, block, 0, s, pl, g, (int)pair, op);    \
    else hipLaunchKernelGGL((k6_smooth_unsqueeze_planes<K, R>), grid, block, 0, s, pl, g, (int)pair);             \
  } while (0)
  switch (kind * 2 + (cvt_rne ? 1 : 0)) {
    case 0: JXLH_SM_LAUNCH(0, false); break;
    case 1: JXLH_SM_LAUNCH(0, true); break;
    case 2: JXLH_SM_LAUNCH(1, false); break;
    case 3: JXLH_SM_LAUNCH(1, true); break;
    case 4: JXLH_SM_LAUNCH(2, false); break;
    default: JXLH_SM_LAUNCH(2, true); break;
  }
#undef JXLH_SM_LAUNCH
}

// The smooth cells of a partly arrived level (jxlh_unsqueeze_chain_preview_tiles, squeeze_preview_plan.h): one launch over
// the listed cells, tiles_per_cell workgroups each (what a full 1-D cell needs; a cell that needs fewer -- a 2-D one, a
// ragged last one -- sends the surplus home), the plane in blockIdx.y.  A cell is jxlh_smooth_unsqueeze on its rect: 1-D
// along the level's axis from the level's average (in1), or 2-D from the average the level before reads (in2).  A cell
// without one complete pair on a doubled axis is what the reference leaves of a fresh buffer: zero.
static_assert(JXLH_SQC_TX == JXLH_SM_TX && JXLH_SQC_TY == JXLH_SM_TY, "squeeze_preview_plan.h counts the workgroups of a cell");
struct SmoothCellsArgs {
  const int32_t* in1[3];
  const int32_t* in2[3];
  int32_t* out[3];
  size_t in1_stride, in2_stride, out_stride;
  int in1_w, in1_h, in2_w, in2_h;
  const SqTileSmoothCell* cells;
  uint32_t tiles_x, tiles_per_cell;
};
template <bool HORIZ, bool RNE>
__global__ __launch_bounds__(JXLH_SM_TX* JXLH_SM_WAVES) void k6_smooth_unsqueeze_cells(const SmoothCellsArgs A) {
  __shared__ float tile[1][JXLH_SM_TY + 4][JXLH_SM_TX + 4 + 1];
  const uint32_t cell = blockIdx.x / A.tiles_per_cell, t = blockIdx.x - cell * A.tiles_per_cell;
  const SqTileSmoothCell c = A.cells[cell];
  const bool two_d = (c.h_kind & 3) == JXLH_PREVIEW_SMOOTH_2D;
  const int w = c.w, h = c.h_kind >> 2;
  const bool fx = two_d || HORIZ, fy = two_d || !HORIZ;
  const int nx = fx ? (w + 1) / 2 : w, ny = fy ? (h + 1) / 2 : h;
  const int bx = (int)(t % A.tiles_x) * JXLH_SM_TX, by = (int)(t / A.tiles_x) * JXLH_SM_TY;
  if (bx >= nx || by >= ny) return;  // workgroup-uniform, in front of every barrier
  int32_t* const o = A.out[blockIdx.y] + (size_t)c.y0 * A.out_stride + c.x0;
  if ((fx ? w / 2 : w) == 0 || (fy ? h / 2 : h) == 0) {
    const int ox0 = fx ? 2 * bx : bx, oy0 = fy ? 2 * by : by;
    const int ow = min(w - ox0, fx ? 2 * JXLH_SM_TX : JXLH_SM_TX), oh = min(h - oy0, fy ? 2 * JXLH_SM_TY : JXLH_SM_TY);
    for (int i = threadIdx.x; i < ow * oh; i += JXLH_SM_TX * JXLH_SM_WAVES) o[(size_t)(oy0 + i / ow) * A.out_stride + ox0 + i % ow] = 0;
    return;
  }
  int32_t* const ov[1] = {o};
  const bool pair = ((uintptr_t)o & 7) == 0 && (A.out_stride & 1) == 0;
  if (two_d) {
    const int32_t* const iv[1] = {A.in2[blockIdx.y]};
    smooth_tile<2, RNE, 1, true>(tile, iv, ov, SmoothGeom{A.in2_stride, A.out_stride, A.in2_w, A.in2_h, c.x0 / 2, c.y0 / 2, w, h, nx, ny}, pair, 0,
                           bx, by);
  } else {
    const int32_t* const iv[1] = {A.in1[blockIdx.y]};
    smooth_tile<HORIZ ? 0 : 1, RNE, 1, true>(tile, iv, ov,
                                       SmoothGeom{A.in1_stride, A.out_stride, A.in1_w, A.in1_h, HORIZ ? c.x0 / 2 : c.x0,
                                                  HORIZ ? c.y0 : c.y0 / 2, w, h, nx, ny},
                                       pair, 0, bx, by);
  }
}

void launch_smooth_unsqueeze_cells(hipStream_t s, bool horizontal, int n_planes, const int32_t* const in1[], size_t in1_stride,
                                   int in1_w, int in1_h, const int32_t* const in2[], size_t in2_stride, int in2_w, int in2_h,
                                   int32_t* const out[], size_t out_stride, const SqTileSmoothCell* cells, uint32_t n_cells,
                                   uint32_t tiles_x, uint32_t tiles_per_cell, bool cvt_rne) {
  if (n_cells == 0) return;
  SmoothCellsArgs A{};
  for (int p = 0; p < n_planes; p++) {
    A.in1[p] = in1[p];
    A.in2[p] = in2[p];
    A.out[p] = out[p];
  }
  A.in1_stride = in1_stride;
  A.in2_stride = in2_stride;
  A.out_stride = out_stride;
  A.in1_w = in1_w;
  A.in1_h = in1_h;
  A.in2_w = in2_w;
  A.in2_h = in2_h;
  A.cells = cells;
  A.tiles_x = tiles_x;
  A.tiles_per_cell = tiles_per_cell;
  const dim3 grid(n_cells * tiles_per_cell, n_planes), block(JXLH_SM_TX * JXLH_SM_WAVES);
  if (horizontal) {
    if (cvt_rne) hipLaunchKernelGGL((k6_smooth_unsqueeze_cells<true, true>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k6_smooth_unsqueeze_cells<true, false>), grid, block, 0, s, A);
  } else {
    if (cvt_rne) hipLaunchKernelGGL((k6_smooth_unsqueeze_cells<false, true>), grid, block, 0, s, A);
    else hipLaunchKernelGGL((k6_smooth_unsqueeze_cells<false, false>), grid, block, 0, s, A);
  }
}

}  // namespace jxlh
