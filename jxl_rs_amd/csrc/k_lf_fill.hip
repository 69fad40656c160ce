// The fill of groups whose HF has not arrived (upsample_lf_group, jxl/src/frame/decode.rs:51-158, taken by
// decode_and_render_varct_and_noise for a group with DataStatus::Zero, :744-752): the three colour buffers of such a
// group are the LF image upsampled 8x (Upsample8x with the file's weights8) instead of a transform's output.  For every
// LF pixel (= 8x8 block) of a listed group this writes the 8 x 8 patch into the planes K1 writes, in the layout of the
// run (pix_layout(f): raster, or the 8x8-tiled form ahead of the fused filters), whole blocks up to xblocks*8 x
// yblocks*8.  The 5x5 window reads the WHOLE LF image and mirrors only at the image's edges: a group's pixels are the
// group's rect of Upsample8x applied to the whole image.  (The reference works on a per-group copy with a persistent
// scratch row; it reads that row beyond what it filled in two geometries -- jxl_hip.h says which -- and those are not
// reproduced.)
//
// Layout, as k_upsample<8>: a thread is a short column of kFillRows LF pixels, the 25-value window slides down in
// registers (upsample_device.h, the arithmetic of k_upsample.hip and k_lf_preview.hip unchanged), the tap weights are
// indexed uniformly across the wavefront (scalar loads; the 6400-byte table lives in the scalar cache).  A workgroup is
// one channel of one listed group: 32 LF columns x 8 runs of 4 LF rows.  The grid is (listed group, channel): no image
// axis is a grid dimension.  A patch is computed in two halves of 4 rows (32 values in registers, indexed statically):
//   tiled   the half is 128 contiguous bytes of the block's 256 ((y & 4) * 8 + (x & 7) * 4 + (y & 3)): for each x the
//           four rows are one 16-byte store, eight stores complete the line
//   raster  each of the four rows is two 16-byte stores; the 32 lanes of a row run write 1 KB of a plane row
// Bound: the stores -- 786 KB out against 12 KB in per group; the 1600 FMAs per LF pixel are ~a third of the store time.
#include "jxlh_internal.h"
#include "upsample_device.h"

namespace jxlh {
namespace {

constexpr int kFillThreads = 256;  // 32 LF columns x 8 runs of kFillRows LF rows = the 32 x 32 blocks of a group
constexpr int kFillRows = 4;
static_assert(kGroupBlocks == 32 && (kFillThreads / 32) * kFillRows == kGroupBlocks, "a workgroup covers one group");

__global__ __launch_bounds__(kFillThreads) void k_lf_fill(const FrameDev f, const float* __restrict__ kernels,
                                                          const int* __restrict__ groups) {
  const int g = groups[blockIdx.x];
  const int c = (int)blockIdx.y;
  const int bx = (g % f.xgroups) * kGroupBlocks + (int)(threadIdx.x & 31);
  const int by0 = (g / f.xgroups) * kGroupBlocks + (int)(threadIdx.x >> 5) * kFillRows;
  if (bx >= f.xblocks || by0 >= f.yblocks) return;
  const float* __restrict__ in = f.lf[c];
  float* __restrict__ out = f.planes[c];
  float win[25];
  int xs[5];
  ups_columns(bx, f.xblocks, xs);
  ups_window_prime(in, (size_t)f.xblocks, f.yblocks, by0, xs, win);
#pragma unroll 1
  for (int r = 0; r < kFillRows; r++) {
    const int by = by0 + r;
    if (by >= f.yblocks) break;
    ups_window_advance(in, (size_t)f.xblocks, f.yblocks, by, xs, win);
    float mn, mx;
    ups_minmax(win, mn, mx);
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      float v[4][8];
#pragma unroll
      for (int oy = 0; oy < 4; oy++) ups_patch_row<8>(win, mn, mx, kernels, half * 4 + oy, v[oy]);
      if (f.tiled) {
        float* __restrict__ dst = out + ((size_t)by * f.xblocks + bx) * 64 + half * 32;
#pragma unroll
        for (int x = 0; x < 8; x++)
          *reinterpret_cast<float4*>(dst + x * 4) = make_float4(v[0][x], v[1][x], v[2][x], v[3][x]);
      } else {
        float* __restrict__ dst = out + (size_t)(by * 8 + half * 4) * f.plane_stride + (size_t)bx * 8;
#pragma unroll
        for (int oy = 0; oy < 4; oy++) {
          float* __restrict__ row = dst + (size_t)oy * f.plane_stride;
          *reinterpret_cast<float4*>(row) = make_float4(v[oy][0], v[oy][1], v[oy][2], v[oy][3]);
          *reinterpret_cast<float4*>(row + 4) = make_float4(v[oy][4], v[oy][5], v[oy][6], v[oy][7]);
        }
      }
    }
  }
}

}  // namespace

// groups: n group ids on the device, each < xgroups * ygroups; kernels: the 8 * 8 * 25 expanded taps of factor 8
void launch_lf_fill(hipStream_t s, const FrameDev& f, const float* kernels, const int* groups, int n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_lf_fill, dim3((unsigned)n, 3), dim3(kFillThreads), 0, s, f, kernels, groups);
}

}  // namespace jxlh
