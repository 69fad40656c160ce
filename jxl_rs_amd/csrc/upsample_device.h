// The per-thread pieces of Upsample<N> (jxl/src/render/stages/upsample.rs) that k_upsample.hip and k_lf_preview.hip
// share: the mirrored 5x5 window that slides down a column, its minimum / maximum, and one output row of the N x N patch
// (25 taps in the reference's order: three accumulators, tap t feeds accumulator t % 3, the first three taps plain
// products, the rest FMAs, (acc0 + acc1) + acc2, clamped to the window's range).
#pragma once
#include <hip/hip_runtime.h>

namespace jxlh {

__device__ __forceinline__ int mirror_idx(int v, int s) {
  while (v < 0 || v >= s) v = v < 0 ? -v - 1 : 2 * s - v - 1;
  return v;
}

// the five mirrored columns around input column x of an image w wide
__device__ __forceinline__ void ups_columns(int x, int w, int (&xs)[5]) {
#pragma unroll
  for (int k = 0; k < 5; k++) xs[k] = mirror_idx(x - 2 + k, w);
}

// rows y0 - 2 .. y0 + 1 into window rows 1..4: ups_window_advance shifts before it loads
__device__ __forceinline__ void ups_window_prime(const float* __restrict__ in, size_t in_stride, int h, int y0,
                                                 const int (&xs)[5], float (&win)[25]) {
#pragma unroll
  for (int ky = 0; ky < 4; ky++) {
    const float* __restrict__ row = in + (size_t)mirror_idx(y0 - 2 + ky, h) * in_stride;
#pragma unroll
    for (int kx = 0; kx < 5; kx++) win[(ky + 1) * 5 + kx] = row[xs[kx]];
  }
}

// the window of input row y from the window of row y - 1 (or the primed one): a row costs 5 loads instead of 25
__device__ __forceinline__ void ups_window_advance(const float* __restrict__ in, size_t in_stride, int h, int y,
                                                   const int (&xs)[5], float (&win)[25]) {
#pragma unroll
  for (int t = 0; t < 20; t++) win[t] = win[t + 5];
  const float* __restrict__ row = in + (size_t)mirror_idx(y + 2, h) * in_stride;
#pragma unroll
  for (int kx = 0; kx < 5; kx++) win[20 + kx] = row[xs[kx]];
}

__device__ __forceinline__ void ups_minmax(const float (&win)[25], float& mn, float& mx) {
  mn = win[0];
  mx = win[0];
#pragma unroll
  for (int t = 1; t < 25; t++) {
    mn = win[t] < mn ? win[t] : mn;
    mx = win[t] > mx ? win[t] : mx;
  }
}

// one output sample: the window against the 25 taps at k (uniform across the wavefront)
__device__ __forceinline__ float ups_taps(const float (&win)[25], float mn, float mx, const float* __restrict__ k) {
  float a0 = win[0] * k[0], a1 = win[1] * k[1], a2 = win[2] * k[2];
#pragma unroll
  for (int t = 3; t < 25; t += 3) {
    a0 = __builtin_fmaf(win[t], k[t], a0);
    if (t + 1 < 25) a1 = __builtin_fmaf(win[t + 1], k[t + 1], a1);
    if (t + 2 < 25) a2 = __builtin_fmaf(win[t + 2], k[t + 2], a2);
  }
  float q = (a0 + a1) + a2;
  q = q > mn ? q : mn;
  q = q < mx ? q : mx;
  return q;
}

// row oy of the N x N patch; kernels[(oy * N + ox) * 25 + ky * 5 + kx]
template <int N>
__device__ __forceinline__ void ups_patch_row(const float (&win)[25], float mn, float mx, const float* __restrict__ kernels,
                                              int oy, float (&v)[N]) {
#pragma unroll
  for (int ox = 0; ox < N; ox++) v[ox] = ups_taps(win, mn, mx, kernels + (oy * N + ox) * 25);
}

}  // namespace jxlh
