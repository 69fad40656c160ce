// Output stages for an XYB frame shown as 8-bit sRGB, fused into ONE elementwise pass over the
// filtered planes (12 B/px in, 3-4 B/px out instead of three f32 round trips and a 12 B/px D2H):
//   XybStage             jxl/src/render/stages/xyb.rs:208-240   (cube + opsin inverse matrix, FMAs)
//   FromLinearStage/sRGB jxl/src/color/tf.rs:13-44, util/rational_poly.rs:20-35 (sqrt, two Horner
//                        chains with FMAs, IEEE division)
//   ConvertF32ToU8Stage  jxl/src/render/stages/convert.rs:570-606 (x255, 32x32 dither table,
//                        clamp, round to nearest even like the AVX2 store) + interleaved save
// in the order frame/render.rs:757-762, :118 chains them.  Bit-exact vs the oracle's FMA build.
// The colour stage itself (to_display_rgb) lives in color_device.h, shared with k_blend.hip.
#include "color_device.h"
#include "jxlh_internal.h"

namespace jxlh {
namespace {

__constant__ float kDitherDev[32 * 32] = {
#include "dither_table.inc"
};

constexpr int kOutThreads = 256;

__device__ __forceinline__ uint32_t to_u8(float v, const float* __restrict__ dither, int x, int y, int c) {
  const float d = dither[((y + c * 13) & 31) * 32 + ((x + c * 23) & 31)];
  const float dithered = v * 255.0f + d;
  float clamped = dithered > 0.0f ? dithered : 0.0f;
  clamped = clamped < 255.0f ? clamped : 255.0f;
  return (uint32_t)__builtin_rintf(clamped);
}

__device__ __forceinline__ uint32_t to_u16(float v) {  // f32_to_u16_simd (convert.rs:743-761), 16-bit
  float clamped = v > 0.0f ? v : 0.0f;
  clamped = clamped < 1.0f ? clamped : 1.0f;
  return (uint32_t)__builtin_rintf(clamped * 65535.0f);
}

// one thread = 4 consecutive pixels of one row; 16-bit samples (no dither), little endian
template <int CH, int MODE>
__global__ __launch_bounds__(kOutThreads) void k_xyb_to_rgb16(const float* __restrict__ px, const float* __restrict__ py,
                                                              const float* __restrict__ pb, uint32_t stride, int w,
                                                              int y0, int rows, const XybParamsDev p, const TfParamsDev t,
                                                              uint16_t* __restrict__ out, size_t out_stride_elems) {
  const int x4 = (blockIdx.x * kOutThreads + threadIdx.x) * 4;
  const int r = blockIdx.y;
  if (x4 >= w || r >= rows) return;
  const size_t in = (size_t)(y0 + r) * stride + x4;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (x4 + i >= w) break;
    float rr, gg, bb;
    to_display_rgb<MODE>(p, t, px[in + i], py[in + i], pb[in + i], rr, gg, bb);
    uint16_t* o = out + (size_t)r * out_stride_elems + (size_t)(x4 + i) * CH;
    o[0] = (uint16_t)to_u16(rr);
    o[1] = (uint16_t)to_u16(gg);
    o[2] = (uint16_t)to_u16(bb);
    if constexpr (CH == 4) o[3] = 65535;
  }
}

// one thread = 4 consecutive pixels of one row
template <int CH, int MODE>
__global__ __launch_bounds__(kOutThreads) void k_xyb_to_rgb8(const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pb, uint32_t stride, int w,
                                                             int y0, int rows, const XybParamsDev p, const TfParamsDev t,
                                                             uint8_t* __restrict__ out, size_t out_stride, int aligned) {
  __shared__ float s_dither[32 * 32];
  for (int i = threadIdx.x; i < 32 * 32; i += kOutThreads) s_dither[i] = kDitherDev[i];
  __syncthreads();
  const int x4 = (blockIdx.x * kOutThreads + threadIdx.x) * 4;
  const int r = blockIdx.y;
  if (x4 >= w || r >= rows) return;
  const int y = y0 + r;
  const size_t in = (size_t)y * stride + x4;
  float vx[4], vy[4], vb[4];
  if (x4 + 4 <= w) {
    const float4 a = *reinterpret_cast<const float4*>(px + in), b = *reinterpret_cast<const float4*>(py + in),
                 c = *reinterpret_cast<const float4*>(pb + in);
    vx[0] = a.x; vx[1] = a.y; vx[2] = a.z; vx[3] = a.w;
    vy[0] = b.x; vy[1] = b.y; vy[2] = b.z; vy[3] = b.w;
    vb[0] = c.x; vb[1] = c.y; vb[2] = c.z; vb[3] = c.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const bool ok = x4 + i < w;
      vx[i] = ok ? px[in + i] : 0.0f;
      vy[i] = ok ? py[in + i] : 0.0f;
      vb[i] = ok ? pb[in + i] : 0.0f;
    }
  }
  uint32_t q[4][3];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float rr, gg, bb;
    to_display_rgb<MODE>(p, t, vx[i], vy[i], vb[i], rr, gg, bb);
    q[i][0] = to_u8(rr, s_dither, x4 + i, y, 0);
    q[i][1] = to_u8(gg, s_dither, x4 + i, y, 1);
    q[i][2] = to_u8(bb, s_dither, x4 + i, y, 2);
  }
  uint8_t* o = out + (size_t)r * out_stride + (size_t)x4 * CH;
  if (aligned && x4 + 4 <= w) {
    uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
    if constexpr (CH == 3) {
      o32[0] = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
      o32[1] = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
      o32[2] = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) o32[i] = q[i][0] | (q[i][1] << 8) | (q[i][2] << 16) | 0xff000000u;
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (x4 + i < w) {
        o[i * CH] = (uint8_t)q[i][0];
        o[i * CH + 1] = (uint8_t)q[i][1];
        o[i * CH + 2] = (uint8_t)q[i][2];
        if constexpr (CH == 4) o[i * CH + 3] = 255;
      }
    }
  }
}

// YCbCr frame with sub-sampled chroma, straight from K1's output: HorizontalChromaUpsample / VerticalChromaUpsample
// (the arithmetic of k_chroma.hip: blend = fma(neighbour, 0.25, centre * 0.75), horizontal stage first, mirrored at the
// edges of the sub-sampled channel) evaluated per output pixel, then YcbcrToRgbStage and the integer conversion.
// Used when nothing sits between the transforms and the output (no filters, upsampling or noise): the full-resolution
// chroma planes are then never written or read back.
__device__ __forceinline__ int mirror_idx(int v, int s) {
  while (v < 0 || v >= s) v = v < 0 ? -v - 1 : 2 * s - v - 1;
  return v;
}
__device__ __forceinline__ float chroma_blend(float neighbour, float centre) {
  return __builtin_fmaf(neighbour, 0.25f, centre * 0.75f);
}

template <int CH, bool U16>
__global__ __launch_bounds__(kOutThreads) void k_ycbcr_sub_to_rgb(const SubPlanesDev sp, uint32_t stride, int w, int y0,
                                                                  int rows, void* __restrict__ out, size_t out_stride,
                                                                  int aligned) {
  __shared__ float s_dither[32 * 32];
  if constexpr (!U16) {
    for (int i = threadIdx.x; i < 32 * 32; i += kOutThreads) s_dither[i] = kDitherDev[i];
    __syncthreads();
  }
  const int x4 = (blockIdx.x * kOutThreads + threadIdx.x) * 4;
  const int r = blockIdx.y;
  if (x4 >= w || r >= rows) return;
  const int y = y0 + r;
  float v[3][4];
  const bool whole = x4 + 4 <= w;
  auto load4 = [&](const float* __restrict__ row, int x0, int n, float (&o)[4]) {  // row[x0 .. x0+3], zero past n
    if (x0 + 4 <= n && ((reinterpret_cast<uintptr_t>(row + x0) & 15) == 0)) {
      const float4 t = *reinterpret_cast<const float4*>(row + x0);
      o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) o[i] = x0 + i < n ? row[x0 + i] : 0.0f;
    }
  };
  auto mirror1 = [](int v, int n) {  // one reflection, then clamped: exact for the +-1 / +-2 excursions used here
    v = v < 0 ? -v - 1 : (v >= n ? 2 * n - v - 1 : v);
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
  };
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* __restrict__ p = sp.p[c];
    const int hs = sp.hs[c], vs = sp.vs[c];
    if (!(hs | vs)) {
      load4(p + (size_t)y * stride, x4, w, v[c]);
      continue;
    }
    const int cw = sp.cw[c], ch = sp.ch[c];
    const int sy = y >> vs;
    const float* __restrict__ row_c = p + (size_t)sy * stride;
    const float* __restrict__ row_n = p + (size_t)(vs ? mirror1((y & 1) ? sy + 1 : sy - 1, ch) : sy) * stride;
    float hc[4], hn[4];  // the horizontal stage's output at the four pixels, centre row and neighbour row
    if (hs) {
      // pixels x4 .. x4+3 sit on sub-samples s0, s0, s0+1, s0+1 (x4 is a multiple of 4) with horizontal neighbours
      // s0-1, s0+1, s0, s0+2
      const int s0 = x4 >> 1;
      const int ia = mirror1(s0 - 1, cw), ib = min(s0, cw - 1), ic = mirror1(s0 + 1, cw), id = mirror1(s0 + 2, cw);
      const float ca = row_c[ia], cb = row_c[ib], cc = row_c[ic], cd = row_c[id];
      hc[0] = chroma_blend(ca, cb);
      hc[1] = chroma_blend(cc, cb);
      hc[2] = chroma_blend(cb, cc);
      hc[3] = chroma_blend(cd, cc);
      if (vs) {
        const float na = row_n[ia], nb = row_n[ib], nc = row_n[ic], nd = row_n[id];
        hn[0] = chroma_blend(na, nb);
        hn[1] = chroma_blend(nc, nb);
        hn[2] = chroma_blend(nb, nc);
        hn[3] = chroma_blend(nd, nc);
      }
    } else {
      load4(row_c, x4, w, hc);
      load4(row_n, x4, w, hn);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) v[c][i] = vs ? chroma_blend(hn[i], hc[i]) : hc[i];
  }
  (void)whole;
  uint32_t q[4][3];
  const XybParamsDev xp = {};
  const TfParamsDev tp = {};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float rr, gg, bb;
    to_display_rgb<kModeYcbcr>(xp, tp, v[0][i], v[1][i], v[2][i], rr, gg, bb);
    if constexpr (U16) {
      q[i][0] = to_u16(rr);
      q[i][1] = to_u16(gg);
      q[i][2] = to_u16(bb);
    } else {
      q[i][0] = to_u8(rr, s_dither, x4 + i, y, 0);
      q[i][1] = to_u8(gg, s_dither, x4 + i, y, 1);
      q[i][2] = to_u8(bb, s_dither, x4 + i, y, 2);
    }
  }
  if constexpr (U16) {
    uint16_t* o = static_cast<uint16_t*>(out) + (size_t)r * out_stride + (size_t)x4 * CH;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (x4 + i < w) {
        o[i * CH] = (uint16_t)q[i][0];
        o[i * CH + 1] = (uint16_t)q[i][1];
        o[i * CH + 2] = (uint16_t)q[i][2];
        if constexpr (CH == 4) o[i * CH + 3] = 65535;
      }
  } else {
    uint8_t* o = static_cast<uint8_t*>(out) + (size_t)r * out_stride + (size_t)x4 * CH;
    if (aligned && x4 + 4 <= w) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(o);
      if constexpr (CH == 3) {
        o32[0] = q[0][0] | (q[0][1] << 8) | (q[0][2] << 16) | (q[1][0] << 24);
        o32[1] = q[1][1] | (q[1][2] << 8) | (q[2][0] << 16) | (q[2][1] << 24);
        o32[2] = q[2][2] | (q[3][0] << 8) | (q[3][1] << 16) | (q[3][2] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) o32[i] = q[i][0] | (q[i][1] << 8) | (q[i][2] << 16) | 0xff000000u;
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (x4 + i < w) {
          o[i * CH] = (uint8_t)q[i][0];
          o[i * CH + 1] = (uint8_t)q[i][1];
          o[i * CH + 2] = (uint8_t)q[i][2];
          if constexpr (CH == 4) o[i * CH + 3] = 255;
        }
    }
  }
}

}  // namespace

// out_stride: bytes (8-bit) or elements (16-bit)
void launch_ycbcr_sub_to_rgb(hipStream_t s, const SubPlanesDev& sp, size_t stride, int w, int y0, int rows, int channels,
                             int bits, void* out, size_t out_stride) {
  if (w <= 0 || rows <= 0) return;
  const dim3 grid((unsigned)(((w + 3) / 4 + kOutThreads - 1) / kOutThreads), (unsigned)rows);
  const int aligned = ((reinterpret_cast<uintptr_t>(out) | out_stride) & 3) == 0;
  if (bits == 8) {
    if (channels == 3)
      hipLaunchKernelGGL((k_ycbcr_sub_to_rgb<3, false>), grid, dim3(kOutThreads), 0, s, sp, (uint32_t)stride, w, y0, rows,
                         out, out_stride, aligned);
    else
      hipLaunchKernelGGL((k_ycbcr_sub_to_rgb<4, false>), grid, dim3(kOutThreads), 0, s, sp, (uint32_t)stride, w, y0, rows,
                         out, out_stride, aligned);
  } else {
    if (channels == 3)
      hipLaunchKernelGGL((k_ycbcr_sub_to_rgb<3, true>), grid, dim3(kOutThreads), 0, s, sp, (uint32_t)stride, w, y0, rows,
                         out, out_stride, aligned);
    else
      hipLaunchKernelGGL((k_ycbcr_sub_to_rgb<4, true>), grid, dim3(kOutThreads), 0, s, sp, (uint32_t)stride, w, y0, rows,
                         out, out_stride, aligned);
  }
}

template <int MODE>
void launch8_mode(hipStream_t s, const float* const planes[3], size_t stride, int w, int y0, int rows, const XybParamsDev& q,
                  const TfParamsDev& t, int channels, uint8_t* out, size_t out_stride) {
  const dim3 grid((unsigned)(((w + 3) / 4 + kOutThreads - 1) / kOutThreads), (unsigned)rows);
  const int aligned = ((reinterpret_cast<uintptr_t>(out) | out_stride) & 3) == 0;
  if (channels == 3)
    hipLaunchKernelGGL((k_xyb_to_rgb8<3, MODE>), grid, dim3(kOutThreads), 0, s, planes[0], planes[1], planes[2],
                       (uint32_t)stride, w, y0, rows, q, t, out, out_stride, aligned);
  else
    hipLaunchKernelGGL((k_xyb_to_rgb8<4, MODE>), grid, dim3(kOutThreads), 0, s, planes[0], planes[1], planes[2],
                       (uint32_t)stride, w, y0, rows, q, t, out, out_stride, aligned);
}
template <int MODE>
void launch16_mode(hipStream_t s, const float* const planes[3], size_t stride, int w, int y0, int rows,
                   const XybParamsDev& q, const TfParamsDev& t, int channels, uint16_t* out, size_t out_stride_elems) {
  const dim3 grid((unsigned)(((w + 3) / 4 + kOutThreads - 1) / kOutThreads), (unsigned)rows);
  if (channels == 3)
    hipLaunchKernelGGL((k_xyb_to_rgb16<3, MODE>), grid, dim3(kOutThreads), 0, s, planes[0], planes[1], planes[2],
                       (uint32_t)stride, w, y0, rows, q, t, out, out_stride_elems);
  else
    hipLaunchKernelGGL((k_xyb_to_rgb16<4, MODE>), grid, dim3(kOutThreads), 0, s, planes[0], planes[1], planes[2],
                       (uint32_t)stride, w, y0, rows, q, t, out, out_stride_elems);
}

// mode: kTfLinear..kTfGamma (XYB frame + that transfer function), kModeYcbcr, kModeNone
void launch_xyb_to_rgb8(hipStream_t s, const float* const planes[3], size_t stride, int w, int y0, int rows, int mode,
                        const XybParamsDev& q, const TfParamsDev& t, int channels, uint8_t* out, size_t out_stride) {
  if (w <= 0 || rows <= 0) return;
  switch (mode) {
    case kTfLinear: launch8_mode<kTfLinear>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kTfSrgb: launch8_mode<kTfSrgb>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kTfBt709: launch8_mode<kTfBt709>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kTfPq: launch8_mode<kTfPq>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kTfHlg: launch8_mode<kTfHlg>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kTfGamma: launch8_mode<kTfGamma>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    case kModeYcbcr: launch8_mode<kModeYcbcr>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
    default: launch8_mode<kModeNone>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride); break;
  }
}

void launch_xyb_to_rgb16(hipStream_t s, const float* const planes[3], size_t stride, int w, int y0, int rows, int mode,
                         const XybParamsDev& q, const TfParamsDev& t, int channels, uint16_t* out, size_t out_stride_elems) {
  if (w <= 0 || rows <= 0) return;
  switch (mode) {
    case kTfLinear: launch16_mode<kTfLinear>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kTfSrgb: launch16_mode<kTfSrgb>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kTfBt709: launch16_mode<kTfBt709>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kTfPq: launch16_mode<kTfPq>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kTfHlg: launch16_mode<kTfHlg>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kTfGamma: launch16_mode<kTfGamma>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    case kModeYcbcr: launch16_mode<kModeYcbcr>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
    default: launch16_mode<kModeNone>(s, planes, stride, w, y0, rows, q, t, channels, out, out_stride_elems); break;
  }
}

}  // namespace jxlh
