// 2x / 4x / 8x upsampling: Upsample<N> of the reference (jxl/src/render/stages/upsample.rs).
// Every input pixel expands into an N x N patch; output (oy, ox) of the patch is a 5x5 convolution of the
// input window around the pixel with kernel[oy][ox] (25 taps, :175-215: three accumulators, tap t feeds
// accumulator t % 3, the first three taps are plain products, the rest FMAs; result (acc0 + acc1) + acc2),
// clamped to the minimum / maximum of the window (compute_minmax, :115-172).  BORDER (2, 2): the window is
// mirrored at the edges of the input image (util/mirror.rs:8-19).
//
// One thread = a short column of input pixels (the window slides down): 25 window values in registers, N*N*25 FMAs against weights whose index
// is uniform across the wavefront (scalar loads of the kernel table), N rows of N contiguous outputs
// (16-byte stores for N >= 4).  Bound: for N = 2 the 4 B/px read + 16 B/px write; for N = 8 the 1600 FMAs
// per input pixel (25 per output pixel) put it near the f32 vector roof instead -- still no MFMA shape:
// the 25-tap kernels differ per output phase and the data is a sliding window.
#include <algorithm>

#include "jxlh_internal.h"
#include "upsample_device.h"

namespace jxlh {
namespace {

// R consecutive input rows per thread: the 5x5 window slides down, so a row costs 5 loads instead of 25
template <int N, int R>
__global__ __launch_bounds__(256) void k_upsample(const float* __restrict__ in, size_t in_stride, int w, int h,
                                                  const float* __restrict__ kernels, float* __restrict__ out,
                                                  size_t out_stride, int out_w, int out_h) {
  // a workgroup = 256 neighbouring columns: every output row gets 256 * N contiguous floats from it
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y0 = blockIdx.y * R;
  if (x >= w || y0 >= h) return;
  float win[25];
  int xs[5];
  ups_columns(x, w, xs);
  ups_window_prime(in, in_stride, h, y0, xs, win);
#pragma unroll 1
  for (int r = 0; r < R; r++) {
    const int y = y0 + r;
    if (y >= h) break;
    ups_window_advance(in, in_stride, h, y, xs, win);
    float mn, mx;
    ups_minmax(win, mn, mx);
#pragma unroll
    for (int oy = 0; oy < N; oy++) {
      float v[N];
      ups_patch_row<N>(win, mn, mx, kernels, oy, v);
      const int oyy = y * N + oy;
      if (oyy >= out_h) continue;
      float* __restrict__ dst = out + (size_t)oyy * out_stride + (size_t)x * N;
      if (x * N + N <= out_w) {
        if constexpr (N == 2) {
          *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
          for (int i = 0; i < N; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < N; i++)
          if (x * N + i < out_w) dst[i] = v[i];
      }
    }
  }
}

constexpr int kRows2 = 8, kRows4 = 4, kRows8 = 2;

// The three colour planes of a row range in one launch (jxlh_frame_repaint_groups): pointers by value, blockIdx.z the
// channel
struct UpsampleRowsPlanes {
  const float* in[3];
  float* out[3];
};

// k_upsample on input rows [iy0, iy1) of all three planes: blockIdx.y walks the range in strips of R, blockIdx.z is the
// channel.  The window is mirrored at the edges of the IMAGE (h), not of the range: rows outside [iy0, iy1) are read and
// never written, and exactly output rows [N * iy0, min(N * iy1, out_h)) are.  Same helpers, same R per N, same stores as
// k_upsample: the arithmetic, tap order and clamp are its own.
template <int N, int R>
__global__ __launch_bounds__(256) void k_upsample_rows(UpsampleRowsPlanes pl, size_t in_stride, int w, int h, int iy0, int iy1,
                                                       const float* __restrict__ kernels, size_t out_stride, int out_w,
                                                       int out_h) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int y0 = iy0 + blockIdx.y * R;
  if (x >= w || y0 >= iy1) return;
  const int c = blockIdx.z;
  const float* __restrict__ in = c == 0 ? pl.in[0] : c == 1 ? pl.in[1] : pl.in[2];
  float* __restrict__ out = c == 0 ? pl.out[0] : c == 1 ? pl.out[1] : pl.out[2];
  float win[25];
  int xs[5];
  ups_columns(x, w, xs);
  ups_window_prime(in, in_stride, h, y0, xs, win);
#pragma unroll 1
  for (int r = 0; r < R; r++) {
    const int y = y0 + r;
    if (y >= iy1) break;
    ups_window_advance(in, in_stride, h, y, xs, win);
    float mn, mx;
    ups_minmax(win, mn, mx);
#pragma unroll
    for (int oy = 0; oy < N; oy++) {
      float v[N];
      ups_patch_row<N>(win, mn, mx, kernels, oy, v);
      const int oyy = y * N + oy;
      if (oyy >= out_h) continue;
      float* __restrict__ dst = out + (size_t)oyy * out_stride + (size_t)x * N;
      if (x * N + N <= out_w) {
        if constexpr (N == 2) {
          *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
          for (int i = 0; i < N; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < N; i++)
          if (x * N + i < out_w) dst[i] = v[i];
      }
    }
  }
}

}  // namespace

// kernels: n*n*25 floats on the device, [(oy*n + ox)*25 + ky*5 + kx]; out rows 16-byte aligned
void launch_upsample(hipStream_t s, int n, const float* in, size_t in_stride, int w, int h, const float* kernels,
                     float* out, size_t out_stride, int out_w, int out_h) {
  if (w <= 0 || h <= 0) return;
  const dim3 block(256);
  auto grid = [&](int rows) { return dim3((w + 255) / 256, (h + rows - 1) / rows); };
  if (n == 2)
    hipLaunchKernelGGL((k_upsample<2, kRows2>), grid(kRows2), block, 0, s, in, in_stride, w, h, kernels, out, out_stride,
                       out_w, out_h);
  else if (n == 4)
    hipLaunchKernelGGL((k_upsample<4, kRows4>), grid(kRows4), block, 0, s, in, in_stride, w, h, kernels, out, out_stride,
                       out_w, out_h);
  else
    hipLaunchKernelGGL((k_upsample<8, kRows8>), grid(kRows8), block, 0, s, in, in_stride, w, h, kernels, out, out_stride,
                       out_w, out_h);
}

// input rows [iy0, iy1) (0 <= iy0 < iy1 <= h) of three planes that share strides and sizes, in one launch per 32768
// strips of rows (the grid's y extent); everything else as launch_upsample
void launch_upsample_rows(hipStream_t s, int n, const float* const in[3], size_t in_stride, int w, int h, int iy0, int iy1,
                          const float* kernels, float* const out[3], size_t out_stride, int out_w, int out_h) {
  if (w <= 0 || h <= 0 || iy0 < 0 || iy1 > h || iy0 >= iy1) return;
  UpsampleRowsPlanes pl;
  for (int c = 0; c < 3; c++) pl.in[c] = in[c], pl.out[c] = out[c];
  const dim3 block(256);
  const int rows = n == 2 ? kRows2 : n == 4 ? kRows4 : kRows8;
  constexpr int kMaxStrips = 32768;
  for (int a = iy0; a < iy1; a += kMaxStrips * rows) {
    const int b = (int)std::min<long long>(iy1, (long long)a + (long long)kMaxStrips * rows);
    const dim3 grid((w + 255) / 256, (b - a + rows - 1) / rows, 3);
    if (n == 2)
      hipLaunchKernelGGL((k_upsample_rows<2, kRows2>), grid, block, 0, s, pl, in_stride, w, h, a, b, kernels, out_stride, out_w,
                         out_h);
    else if (n == 4)
      hipLaunchKernelGGL((k_upsample_rows<4, kRows4>), grid, block, 0, s, pl, in_stride, w, h, a, b, kernels, out_stride, out_w,
                         out_h);
    else
      hipLaunchKernelGGL((k_upsample_rows<8, kRows8>), grid, block, 0, s, pl, in_stride, w, h, a, b, kernels, out_stride, out_w,
                         out_h);
  }
}

}  // namespace jxlh
