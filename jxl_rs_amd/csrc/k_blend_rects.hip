// The rect-list form of k_blend (jxlh_frame_blend_rects, jxlh_stage_blend_rects): the pixels of a list of IMAGE
// rectangles recomposed in ONE launch, with exactly k_blend's per-pixel work -- 16-byte source loads, the frame side
// read sample by sample at its arbitrary offset, the colour stage as a uniform switch, blend_pixel<NEC> -- and stores
// that never leave a rect.  A translation unit of its own, for the reason k_save_rects.hip gives: k_blend.hip's nine
// kernels serve jxlh_frame_blend with measured times and recorded register counts, and built apart they keep their
// instruction streams.
//
// Layout.  The list (blend_rects_plan.h) lives in device memory and a workgroup's rect depends on blockIdx alone, so
// the bisection over `first` and the descriptor are scalar loads.  Workgroup = kBlendRectRows rows of a rect (a wave
// each) x kBlendRectPixels pixels from the rect's x0 rounded down to a multiple of four: lane = four consecutive pixels
// at a 16-byte-aligned x.  A lane whose four pixels all lie in the rect stores 16 bytes per channel; a lane cut by the
// rect's left or right edge stores its samples singly; a sample outside the rect is never stored.  The canvas is
// neither source nor frame, and a pixel's 3 + NEC values are all read before any is stored: overlapping rects write
// equal values twice and nothing races.  No LDS.
#include "blend_device.h"
#include "blend_rects_plan.h"
#include "color_device.h"
#include "jxlh_internal.h"

namespace jxlh {
namespace {

constexpr int kPx = 4;
static_assert(kBlendRectRows == 4 && kBlendRectPixels == 64 * kPx, "a wave a row, a lane four pixels");

// the rect of workgroup g: the last one whose first workgroup is <= g
__device__ __forceinline__ BlendRectWork find_rect(const BlendRectWork* __restrict__ work, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (work[mid].first <= g) lo = mid;
    else hi = mid;
  }
  return work[lo];
}

__device__ __forceinline__ void unpack4(const float4& v, float (&o)[kPx]) {
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
  o[3] = v.w;
}

// the colour stage `mode` on four pixels' first three channels
template <int MODE, int NCH>
__device__ __forceinline__ void colour4(const XybParamsDev& p, const TfParamsDev& t, float (&px)[kPx][NCH]) {
#pragma unroll
  for (int i = 0; i < kPx; i++) {
    float r, g, b;
    to_display_rgb<MODE>(p, t, px[i][0], px[i][1], px[i][2], r, g, b);
    px[i][0] = r;
    px[i][1] = g;
    px[i][2] = b;
  }
}

template <int NEC>
__global__ __launch_bounds__(256) void k_blend_rects(const BlendLaunch a, const BlendRectWork* __restrict__ work,
                                                     const uint32_t n) {
  constexpr int NCH = 3 + NEC;
  const BlendRectWork r = find_rect(work, n, blockIdx.x);
  const uint32_t local = blockIdx.x - r.first, bx = local % r.nbx, by = local / r.nbx;
  const uint32_t row = by * kBlendRectRows + (threadIdx.x >> 6);
  if (row >= r.h) return;
  const int y = (int)(r.y0 + row);
  const int xl = (int)r.x0, xr = (int)(r.x0 + r.w);  // the rect's columns [xl, xr), inside the image
  const int x = (int)((r.x0 & ~3u) + (bx * 64 + (threadIdx.x & 63)) * kPx);
  if (x >= xr || x + kPx <= xl) return;
  // the frame cut to the image, in image coordinates
  const int fx0 = max(a.x0, 0), fx1 = min(a.x0 + a.fw, a.iw);
  const int fy0 = max(a.y0, 0), fy1 = min(a.y0 + a.fh, a.ih);
  // the source: zeros where the channel's slot is not set
  float4 src[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    src[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.src[c]) src[c] = *reinterpret_cast<const float4*>(a.src[c] + (size_t)y * a.src_stride[c] + x);
  }
  if (y >= fy0 && y < fy1 && x < fx1 && x + kPx > fx0) {
    float fg[kPx][NCH], bg[kPx][NCH];
    bool in[kPx];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float s[kPx];
      unpack4(src[c], s);
      const float* __restrict__ frow = a.frame[c] + (size_t)(y - a.y0) * a.frame_stride[c];
#pragma unroll
      for (int i = 0; i < kPx; i++) {
        in[i] = x + i >= fx0 && x + i < fx1;
        fg[i][c] = s[i];
        bg[i][c] = in[i] ? frow[x + i - a.x0] : 0.0f;
      }
    }
    switch (a.mode) {  // the same for every lane
      case kTfLinear: colour4<kTfLinear>(a.xyb, a.tf, bg); break;
      case kTfSrgb: colour4<kTfSrgb>(a.xyb, a.tf, bg); break;
      case kTfBt709: colour4<kTfBt709>(a.xyb, a.tf, bg); break;
      case kTfPq: colour4<kTfPq>(a.xyb, a.tf, bg); break;
      case kTfHlg: colour4<kTfHlg>(a.xyb, a.tf, bg); break;
      case kTfGamma: colour4<kTfGamma>(a.xyb, a.tf, bg); break;
      case kModeYcbcr: colour4<kModeYcbcr>(a.xyb, a.tf, bg); break;
      default: break;  // kModeNone
    }
#pragma unroll
    for (int i = 0; i < kPx; i++) blend_pixel<NEC>(bg[i], fg[i], a.blend, a.ec_alpha, a.ec_assoc);
#pragma unroll
    for (int c = 0; c < NCH; c++)
      src[c] = make_float4(in[0] ? bg[0][c] : fg[0][c], in[1] ? bg[1][c] : fg[1][c], in[2] ? bg[2][c] : fg[2][c],
                           in[3] ? bg[3][c] : fg[3][c]);
  }
  if (x >= xl && x + kPx <= xr) {
#pragma unroll
    for (int c = 0; c < NCH; c++) *reinterpret_cast<float4*>(a.out[c] + (size_t)y * a.out_stride + x) = src[c];
  } else {
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float* __restrict__ o = a.out[c] + (size_t)y * a.out_stride + x;
      if (x >= xl && x < xr) o[0] = src[c].x;
      if (x + 1 >= xl && x + 1 < xr) o[1] = src[c].y;
      if (x + 2 >= xl && x + 2 < xr) o[2] = src[c].z;
      if (x + 3 >= xl && x + 3 < xr) o[3] = src[c].w;
    }
  }
}

}  // namespace

// jxlh_frame_blend_rects: the n rects of the device-resident list `work` in one launch of `groups` workgroups
// (blend_rects_plan.h: below 2^31).  a.out: planes whose rows are 16-byte aligned (out_stride a multiple of four).
void launch_blend_rects(hipStream_t s, int num_ec, const BlendLaunch& a, const BlendRectWork* work, uint32_t n,
                        uint32_t groups) {
  if (n == 0 || groups == 0 || a.iw <= 0 || a.ih <= 0) return;
  const dim3 grid(groups), block(256);
  switch (num_ec) {
#define JXLH_BLEND_RECTS_CASE(N) \
  case N: k_blend_rects<N><<<grid, block, 0, s>>>(a, work, n); break;
    JXLH_BLEND_RECTS_CASE(0)
    JXLH_BLEND_RECTS_CASE(1)
    JXLH_BLEND_RECTS_CASE(2)
    JXLH_BLEND_RECTS_CASE(3)
    JXLH_BLEND_RECTS_CASE(4)
    JXLH_BLEND_RECTS_CASE(5)
    JXLH_BLEND_RECTS_CASE(6)
    JXLH_BLEND_RECTS_CASE(7)
    JXLH_BLEND_RECTS_CASE(8)
#undef JXLH_BLEND_RECTS_CASE
    default: break;
  }
}

}  // namespace jxlh
