// The intake of a Modular frame: ConvertModularToF32Stage x3 or ConvertModularXYBToF32Stage (render/stages/convert.rs
// :316-342, :416-533; frame/render.rs:554-563) from the context's i32 sample planes into the frame layout the filters,
// patches, splines, upsampling, noise, blending and the save tail read -- all three channels of a row range in one
// launch (the XYB form needs Y while it writes B).
//
// A lane takes 4 consecutive samples of one row: one 16-byte load and one 16-byte store per channel (source and
// destination rows are 16-byte aligned: both are the context's own planes, row stride a multiple of 64 samples); the
// last strip of a row whose width is no multiple of 4 is done sample by sample, so nothing beyond a row's w samples is
// read or written.  The padding of the frame layout (whole 8x8 blocks, rows of round_up(xblocks * 8, 64) samples) is
// left alone: no consumer reads it ("Modular frames").
//
// Grid: x = 64-lane strips of 256 samples, y = groups of 4 rows (either axis of a frame is at most 2^20: at most 2^18
// workgroup rows), z = channel for the per-channel forms (a sub-sampled channel has its own width and row range).
// Expressions as the reference's: (float)v * scale -- one round-to-nearest-even conversion, one multiply --; the XYB
// sum before the product.
#include "jxlh_internal.h"
#include "modular_convert_device.h"

namespace jxlh {
namespace {

template <int FORM>
__device__ __forceinline__ float convert_sample(int32_t v, float scale, uint32_t bits, uint32_t exp_bits) {
  if constexpr (FORM == kIntakeFloat) return float_sample_to_f32((uint32_t)v, bits, exp_bits);
  else return (float)v * scale;
}

template <int FORM>
__global__ __launch_bounds__(256) void k_modular_intake(const IntakeLaunch a) {
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int x = (blockIdx.x * 64 + lane) * 4;
  if constexpr (FORM == kIntakeXyb) {
    const int y = a.y0[0] + (int)blockIdx.y * 4 + sub;
    if (x >= a.w[0] || y >= a.y1[0]) return;
    const size_t so = (size_t)y * a.src_stride + (size_t)x, dof = (size_t)y * a.dst_stride + (size_t)x;
    const int32_t* __restrict__ sy = a.src[0] + so;
    const int32_t* __restrict__ sx = a.src[1] + so;
    const int32_t* __restrict__ sb = a.src[2] + so;
    float* __restrict__ ox = a.dst[0] + dof;
    float* __restrict__ oy = a.dst[1] + dof;
    float* __restrict__ ob = a.dst[2] + dof;
    if (x + 4 <= a.w[0]) {
      const int4 vy = gload_i4<false>(sy), vx = gload_i4<false>(sx), vb = gload_i4<false>(sb);
      const float fy0 = (float)vy.x, fy1 = (float)vy.y, fy2 = (float)vy.z, fy3 = (float)vy.w;
      gstore_f4<false>(ox, make_float4((float)vx.x * a.scale[0], (float)vx.y * a.scale[0], (float)vx.z * a.scale[0],
                                       (float)vx.w * a.scale[0]));
      gstore_f4<false>(oy, make_float4(fy0 * a.scale[1], fy1 * a.scale[1], fy2 * a.scale[1], fy3 * a.scale[1]));
      gstore_f4<false>(ob, make_float4(((float)vb.x + fy0) * a.scale[2], ((float)vb.y + fy1) * a.scale[2],
                                       ((float)vb.z + fy2) * a.scale[2], ((float)vb.w + fy3) * a.scale[2]));
    } else {
      for (int i = 0; i < a.w[0] - x; i++) {
        const float fy = (float)sy[i];
        ox[i] = (float)sx[i] * a.scale[0];
        oy[i] = fy * a.scale[1];
        ob[i] = ((float)sb[i] + fy) * a.scale[2];
      }
    }
  } else {
    // blockIdx.z is wave-uniform: the channel's members are selected with constant indices so that the launch
    // structure stays in the kernel-argument segment (no scratch copy for a dynamic index)
    const int c = blockIdx.z;
    const int32_t* __restrict__ src = c == 0 ? a.src[0] : c == 1 ? a.src[1] : a.src[2];
    float* __restrict__ dst = c == 0 ? a.dst[0] : c == 1 ? a.dst[1] : a.dst[2];
    const int w = c == 0 ? a.w[0] : c == 1 ? a.w[1] : a.w[2];
    const int y0 = c == 0 ? a.y0[0] : c == 1 ? a.y0[1] : a.y0[2];
    const int y1 = c == 0 ? a.y1[0] : c == 1 ? a.y1[1] : a.y1[2];
    const float scale = c == 0 ? a.scale[0] : c == 1 ? a.scale[1] : a.scale[2];
    const int y = y0 + (int)blockIdx.y * 4 + sub;
    if (x >= w || y >= y1) return;
    src += (size_t)y * a.src_stride + (size_t)x;
    dst += (size_t)y * a.dst_stride + (size_t)x;
    if (x + 4 <= w) {
      const int4 v = gload_i4<false>(src);
      gstore_f4<false>(dst, make_float4(convert_sample<FORM>(v.x, scale, a.bits, a.exp_bits),
                                        convert_sample<FORM>(v.y, scale, a.bits, a.exp_bits),
                                        convert_sample<FORM>(v.z, scale, a.bits, a.exp_bits),
                                        convert_sample<FORM>(v.w, scale, a.bits, a.exp_bits)));
    } else {
      for (int i = 0; i < w - x; i++) dst[i] = convert_sample<FORM>(src[i], scale, a.bits, a.exp_bits);
    }
  }
}

__global__ __launch_bounds__(256) void k_fill_f32(float* __restrict__ p, size_t n, float v) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace

void launch_modular_intake(hipStream_t s, const IntakeLaunch& a) {
  const int nc = a.form == kIntakeXyb ? 1 : 3;
  int wmax = 0, rows = 0;
  for (int c = 0; c < nc; c++) {
    if (a.y1[c] <= a.y0[c] || a.w[c] <= 0) continue;
    wmax = max(wmax, a.w[c]);
    rows = max(rows, a.y1[c] - a.y0[c]);
  }
  if (wmax <= 0 || rows <= 0) return;
  const dim3 grid((unsigned)((wmax + 255) / 256), (unsigned)((rows + 3) / 4), (unsigned)nc), block(256);
  if (a.form == kIntakeXyb) hipLaunchKernelGGL(k_modular_intake<kIntakeXyb>, grid, block, 0, s, a);
  else if (a.form == kIntakeFloat) hipLaunchKernelGGL(k_modular_intake<kIntakeFloat>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_modular_intake<kIntakeInt>, grid, block, 0, s, a);
}

// one value for every element (the constant sigma plane of a Modular frame, features/epf.rs:81-84)
void launch_fill_f32(hipStream_t s, float* p, size_t n, float v) {
  if (n) hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

}  // namespace jxlh
