// The two integer read-outs that keep a kernel of their own; the 16-bit read-outs are the identity case of k_save.hip.
// Both end in the conversions of jxl/src/render/stages/convert.rs:570-606, :743-761 and the packed interleaved store of
// save_device.h; bit-exact vs the oracle's FMA build.
//   k_xyb_to_rgb8       the frame's colour stage (color_device.h) and ConvertF32ToU8Stage in ONE pass over the finished
//                       planes (12 B/px in, 3-4 B/px out), in the order frame/render.rs:757-762, :118 chains them.  The
//                       colour mode is a template argument and the launch takes a dozen scalars: k_save_rows<U8>, which
//                       carries the save's whole launch structure, measured 27-31 % slower on this case.
//   k_ycbcr_sub_to_rgb  a YCbCr frame whose chroma is still sub-sampled (a recompressed JPEG with nothing between the
//                       transforms and the output), from K1's output: the chroma upsampling evaluated per output pixel,
//                       then YcbcrToRgbStage (render/stages/ycbcr.rs:35-78) and either integer conversion.
#include "jxlh_internal.h"
#include "save_device.h"

namespace jxlh {
namespace {

constexpr int kOutThreads = 256;

// what convert_sample reads: the integer conversions at full depth, native byte order
struct OutConvert {
  float maxv;
  int big_endian;
  [[maybe_unused]] static constexpr bool kF16Clamp = false;  // (read by the f16 conversion only)
};

// q -> the lane's 4 x CH samples at `o`: one packed store of whole dwords, or sample by sample where `o` is not dword
// aligned and in the row's last, partial lane (n < 4 pixels)
template <int BPS, int CH>
__device__ __forceinline__ void store_lane(uint8_t* o, const uint32_t (&q)[4][CH], int n) {
  constexpr int PB = CH * BPS;
  if (n >= 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    uint32_t wd[PB];
    pack_words<BPS, CH, 4>(q, wd);
    store_words<PB>(o, wd);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < n) {
#pragma unroll
        for (int k = 0; k < CH; k++) store_sample<BPS>(o + (i * CH + k) * BPS, q[i][k]);
      }
  }
}

// one thread = 4 consecutive pixels of one row; `out` is the origin of the whole image, rows out_stride bytes apart
template <int CH, int MODE>
__global__ __launch_bounds__(kOutThreads) void k_xyb_to_rgb8(const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pb, uint32_t stride, int w,
                                                             int y0, int rows, const XybParamsDev p, const TfParamsDev t,
                                                             uint8_t* __restrict__ out, size_t out_stride) {
  __shared__ float s_dither[32 * 32];
  for (int i = threadIdx.x; i < 32 * 32; i += kOutThreads) s_dither[i] = kSaveDitherDev[i];
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
  const OutConvert cv = {255.0f, 0};
  uint32_t q[4][CH];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    float rgb[3];
    to_display_rgb<MODE>(p, t, vx[i], vy[i], vb[i], rgb[0], rgb[1], rgb[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) q[i][k] = convert_sample<kSaveU8>(cv, s_dither, rgb[k], x4 + i, y, k);
    if constexpr (CH == 4) q[i][3] = 255u;
  }
  store_lane<1, CH>(out + (size_t)y * out_stride + (size_t)x4 * CH, q, w - x4);
}

// HorizontalChromaUpsample / VerticalChromaUpsample with the arithmetic of k_chroma.hip: blend = fma(neighbour, 0.25,
// centre * 0.75), horizontal stage first, mirrored at the edges of the sub-sampled channel.  The full-resolution chroma
// planes are never written or read back.
__device__ __forceinline__ float chroma_blend(float neighbour, float centre) {
  return __builtin_fmaf(neighbour, 0.25f, centre * 0.75f);
}

// one thread = 4 consecutive pixels of one row; `out` is the origin of the whole image, rows out_stride bytes apart
template <int CH, int FMT>
__global__ __launch_bounds__(kOutThreads) void k_ycbcr_sub_to_rgb(const SubPlanesDev sp, uint32_t stride, int w, int y0,
                                                                  int rows, uint8_t* __restrict__ out, size_t out_stride) {
  constexpr int BPS = sample_bytes<FMT>(), PB = CH * BPS;
  __shared__ float s_dither[FMT == kSaveU8 ? 32 * 32 : 1];
  if constexpr (FMT == kSaveU8) {
    for (int i = threadIdx.x; i < 32 * 32; i += kOutThreads) s_dither[i] = kSaveDitherDev[i];
    __syncthreads();
  }
  const int x4 = (blockIdx.x * kOutThreads + threadIdx.x) * 4;
  const int r = blockIdx.y;
  if (x4 >= w || r >= rows) return;
  const int y = y0 + r;
  float v[3][4];
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
  colour_px<kModeYcbcr, 4>(XybParamsDev{}, TfParamsDev{}, v);
  const OutConvert cv = {FMT == kSaveU8 ? 255.0f : 65535.0f, 0};
  uint32_t q[4][CH];
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) q[i][k] = convert_sample<FMT>(cv, s_dither, v[k][i], x4 + i, y, k);
    if constexpr (CH == 4) q[i][3] = FMT == kSaveU8 ? 255u : 65535u;
  }
  store_lane<BPS, CH>(out + (size_t)y * out_stride + (size_t)x4 * PB, q, w - x4);
}

}  // namespace

// rows [y0, y0 + rows) into the image whose origin is `out`, rows out_stride bytes apart
void launch_ycbcr_sub_to_rgb(hipStream_t s, const SubPlanesDev& sp, size_t stride, int w, int y0, int rows, int channels,
                             int bits, uint8_t* out, size_t out_stride) {
  if (w <= 0 || rows <= 0) return;
  const dim3 grid((unsigned)(((w + 3) / 4 + kOutThreads - 1) / kOutThreads), (unsigned)rows);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kOutThreads), 0, s, sp, (uint32_t)stride, w, y0, rows, out, out_stride);
  };
  if (bits == 8)
    channels == 3 ? launch(k_ycbcr_sub_to_rgb<3, kSaveU8>) : launch(k_ycbcr_sub_to_rgb<4, kSaveU8>);
  else
    channels == 3 ? launch(k_ycbcr_sub_to_rgb<3, kSaveU16>) : launch(k_ycbcr_sub_to_rgb<4, kSaveU16>);
}

namespace {
template <int MODE>
void launch8_mode(hipStream_t s, const float* const planes[3], size_t stride, int w, int y0, int rows, const XybParamsDev& q,
                  const TfParamsDev& t, int channels, uint8_t* out, size_t out_stride) {
  const dim3 grid((unsigned)(((w + 3) / 4 + kOutThreads - 1) / kOutThreads), (unsigned)rows);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kOutThreads), 0, s, planes[0], planes[1], planes[2], (uint32_t)stride, w, y0,
                       rows, q, t, out, out_stride);
  };
  channels == 3 ? launch(k_xyb_to_rgb8<3, MODE>) : launch(k_xyb_to_rgb8<4, MODE>);
}
}  // namespace

// mode: kTfLinear..kTfGamma (XYB frame + that transfer function), kModeYcbcr, kModeNone; out / out_stride as above
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

}  // namespace jxlh
