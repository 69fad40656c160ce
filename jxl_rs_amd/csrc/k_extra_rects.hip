// Extra channels by rect (jxl_hip_extra_rects.h, ec_rects_plan.h): the two kernels behind them.
//
// k_ec_scatter: the rects of one jxlh_frame_set_extra_channel_rects call, from one block of i32 samples into the
// channels' sample planes, in one launch.  A workgroup takes a piece of kEcPieceW x kEcPieceH samples of a rect; it
// finds its rect by bisection over the descriptors' `first` -- everything it addresses a descriptor with is uniform
// (blockIdx and the loop), so the descriptors arrive through scalar loads.  Four consecutive samples per lane: one
// 16-byte access on both sides where the host found the rect aligned for it (EcScatterDesc::vec), else 4-byte ones.
// Nothing outside a rect is written.  Pure data movement: bound by the 8 B per sample it moves.
//
// k_ec_finish<N>: the dirty tiles of a run (EcItem), one workgroup per tile of kEcTileW x kEcTileH source samples.
// N = 1 is ConvertModularToF32Stage on the tile (convert.rs) into the channel's f32 plane.  N = 2, 4, 8 is that
// conversion fused into Upsample<N> (upsample.rs): the tile's i32 samples and their 2-sample halo, mirrored against the
// WHOLE channel, are converted once into LDS (20 x 68 floats); then a lane is a column, a wave four rows, the 5 x 5
// window slides down the column out of LDS and the N x N patches go to the channel's `out` plane as in k_upsample --
// the loaders, the tap order, the three accumulators and the clamp are upsample_device.h's, used on the LDS tile as
// they are on a plane.  No f32 plane exists for such a channel.  The conversion is exact per sample, so the result has
// the bits of k_modular_to_f32 + k_upsample.  One kernel per factor: the window and the patch are sized by N, and a
// uniform switch would have every factor pay for the registers of N = 8.
#include "ec_rects_plan.h"
#include "jxlh_internal.h"
#include "modular_convert_device.h"
#include "upsample_device.h"

namespace jxlh {
namespace {

__global__ __launch_bounds__(256) void k_ec_scatter(const int32_t* __restrict__ src, const EcScatterDesc* __restrict__ descs,
                                                    uint32_t n, uint64_t pieces, EcPlanes planes) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t g = blockIdx.x; g < pieces; g += gridDim.x) {
    uint32_t lo = 0, hi = n;  // the last descriptor whose first <= g
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (descs[mid].first <= g) lo = mid;
      else hi = mid;
    }
    const EcScatterDesc d = descs[lo];
    const uint64_t piece = g - d.first;
    const uint32_t px = (uint32_t)(piece % d.npx), py = (uint32_t)(piece / d.npx);
    const uint32_t x = px * kEcPieceW + (tid & 63u) * 4u;
    if (x >= d.w) continue;
    const int32_t* __restrict__ s0 = src + d.src_off + x;
    int32_t* __restrict__ t0 = planes.raw[d.ec] + d.dst_off + x;
#pragma unroll
    for (uint32_t j = 0; j < kEcPieceH / 4; j++) {
      const uint32_t y = py * kEcPieceH + (tid >> 6) + 4u * j;
      if (y >= d.h) break;
      const int32_t* __restrict__ s = s0 + (uint64_t)y * d.src_stride;
      int32_t* __restrict__ t = t0 + (uint64_t)y * d.dst_stride;
      if (d.vec && x + 4u <= d.w) {
        *reinterpret_cast<int4*>(t) = *reinterpret_cast<const int4*>(s);
      } else {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
          if (x + i < d.w) t[i] = s[i];
      }
    }
  }
}

// ConvertModularToF32Stage of one sample of channel c (uniform branch: the format is the channel's)
__device__ __forceinline__ float ec_convert(const EcChannelDesc& c, int32_t v) {
  return c.exp_bits ? float_sample_to_f32((uint32_t)v, c.bits, c.exp_bits) : (float)v * c.scale;
}

constexpr int kEcLdsW = (int)(kEcTileW + 2 * kEcHalo), kEcLdsH = (int)(kEcTileH + 2 * kEcHalo);

template <int N>
__global__ __launch_bounds__(256) void k_ec_finish(const EcChannelDesc* __restrict__ chans, const EcItem* __restrict__ items,
                                                   const float* __restrict__ kernels) {
  static_assert(kEcTileW == 64 && kEcTileH == 16, "a lane per column, a wave per four rows");
  const EcItem it = items[blockIdx.x];
  const EcChannelDesc c = chans[it.ec];
  const int w = (int)c.w, h = (int)c.h;
  const int x0 = (int)((it.tile % c.ntx) * kEcTileW), y0 = (int)((it.tile / c.ntx) * kEcTileH);
  const int col = (int)(threadIdx.x & 63u), r0 = (int)(threadIdx.x >> 6) * 4;
  if constexpr (N == 1) {
    const int x = x0 + col;
    if (x >= w) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int y = y0 + r0 + r;
      if (y >= h) break;
      c.dst[(size_t)y * c.dst_stride + x] = ec_convert(c, c.raw[(size_t)y * c.w + x]);
    }
  } else {
    __shared__ float tile[kEcLdsH * kEcLdsW];
    // the tile and its halo, converted: only the columns and rows a window of the tile's own samples reads (the tile
    // is cut at the channel's edge, and mirroring never reaches further than the halo beyond it)
    const int x_last = min(x0 + (int)kEcTileW, w) - 1 + (int)kEcHalo, y_last = min(y0 + (int)kEcTileH, h) - 1 + (int)kEcHalo;
    for (int i = (int)threadIdx.x; i < kEcLdsH * kEcLdsW; i += 256) {
      const int ly = i / kEcLdsW, lx = i - ly * kEcLdsW;
      const int gx = x0 - (int)kEcHalo + lx, gy = y0 - (int)kEcHalo + ly;
      if (gx > x_last || gy > y_last) continue;
      tile[i] = ec_convert(c, c.raw[(size_t)mirror_idx(gy, h) * c.w + mirror_idx(gx, w)]);
    }
    __syncthreads();
    const int x = x0 + col;
    if (x >= w || y0 + r0 >= h) return;
    // local coordinates: sample (x, y) sits at tile[(y - y0 + 2) * kEcLdsW + x - x0 + 2]; inside the tile nothing mirrors
    float win[25];
    int xs[5];
    ups_columns(col + (int)kEcHalo, kEcLdsW, xs);
    ups_window_prime(tile, (size_t)kEcLdsW, kEcLdsH, r0 + (int)kEcHalo, xs, win);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
      const int y = y0 + r0 + r;
      if (y >= h) break;
      ups_window_advance(tile, (size_t)kEcLdsW, kEcLdsH, r0 + r + (int)kEcHalo, xs, win);
      float mn, mx;
      ups_minmax(win, mn, mx);
#pragma unroll
      for (int oy = 0; oy < N; oy++) {
        float v[N];
        ups_patch_row<N>(win, mn, mx, kernels, oy, v);
        const int oyy = y * N + oy;
        if (oyy >= (int)c.out_h) continue;
        float* __restrict__ dst = c.dst + (size_t)oyy * c.dst_stride + (size_t)x * N;
        if (x * N + N <= (int)c.out_w) {
          if constexpr (N == 2) {
            *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
          } else {
#pragma unroll
            for (int i = 0; i < N; i += 4) *reinterpret_cast<float4*>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < N; i++)
            if (x * N + i < (int)c.out_w) dst[i] = v[i];
        }
      }
    }
  }
}

}  // namespace

void launch_ec_scatter(hipStream_t s, const int32_t* src, const EcScatterDesc* descs, uint32_t n, uint64_t pieces,
                       const EcPlanes& planes) {
  if (n == 0 || pieces == 0) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(pieces, 1u << 20);  // beyond that a workgroup takes several pieces
  hipLaunchKernelGGL(k_ec_scatter, dim3(grid), dim3(256), 0, s, src, descs, n, pieces, planes);
}

// items: `count` tiles of channels whose factor is n; kernels: launch_upsample's (unused for n == 1)
void launch_ec_finish(hipStream_t s, int n, const EcChannelDesc* chans, const EcItem* items, uint32_t count,
                      const float* kernels) {
  if (count == 0) return;
  const dim3 grid(count), block(256);
  if (n == 1) hipLaunchKernelGGL((k_ec_finish<1>), grid, block, 0, s, chans, items, kernels);
  else if (n == 2) hipLaunchKernelGGL((k_ec_finish<2>), grid, block, 0, s, chans, items, kernels);
  else if (n == 4) hipLaunchKernelGGL((k_ec_finish<4>), grid, block, 0, s, chans, items, kernels);
  else hipLaunchKernelGGL((k_ec_finish<8>), grid, block, 0, s, chans, items, kernels);
}

}  // namespace jxlh
