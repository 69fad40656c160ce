// Frame blending and extension to the image size in one pass over the IMAGE:
//   BlendingStage                 jxl/src/render/stages/blending.rs:97-166  (perform_blending with the frame as bg and the
//                                 source slot as fg, through blend_pixel of blend_device.h)
//   ExtendToImageDimensionsStage  jxl/src/render/stages/extend.rs:59-84     (image pixels outside the frame = the source)
// with the frame's colour stage (color_device.h) applied to the frame's samples in registers first.
//
// Layout.  The image is cut into tiles of 256 px x 4 rows, one workgroup of 256 threads each: wave = row, lane = four
// consecutive pixels.  Canvas and slot rows are 256-B aligned, so every access on the image side is one 16-byte access
// per lane and channel (a wave moves 1 KiB of a row); the frame side sits at an arbitrary x0 and is read sample by
// sample (consecutive lanes still read consecutive 16-byte groups).  A tile that does not meet the frame -- decided on
// workgroup-uniform values -- copies source to canvas and never enters the blend.  A pixel's 3 + NEC values are all read
// before any of them is stored, and the canvas is a buffer of its own: running the pass again gives the same canvas.
// No LDS, no reuse: (3 + NEC) x 4 B x (2 reads + 1 write) per blended pixel, (3 + NEC) x 4 B x 2 per extended pixel.
//
// NEC is a template parameter (the pixel lives in register arrays); the colour stage is a wavefront-uniform runtime
// switch, so the kernel exists nine times and not seventy-two.
#include "blend_device.h"
#include "color_device.h"
#include "jxlh_internal.h"

namespace jxlh {
namespace {

constexpr int kBlendTileW = 256, kBlendTileH = 4, kBlendPx = 4;

__device__ __forceinline__ void unpack4(const float4& v, float (&o)[kBlendPx]) {
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
  o[3] = v.w;
}

// the colour stage `mode` on four pixels' first three channels
template <int MODE, int NCH>
__device__ __forceinline__ void colour4(const XybParamsDev& p, const TfParamsDev& t, float (&px)[kBlendPx][NCH]) {
#pragma unroll
  for (int i = 0; i < kBlendPx; i++) {
    float r, g, b;
    to_display_rgb<MODE>(p, t, px[i][0], px[i][1], px[i][2], r, g, b);
    px[i][0] = r;
    px[i][1] = g;
    px[i][2] = b;
  }
}

template <int NEC>
__global__ __launch_bounds__(256) void k_blend(const BlendLaunch a, const int ntx) {
  constexpr int NCH = 3 + NEC;
  const int tx = (int)(blockIdx.x % (uint32_t)ntx), ty = (int)(blockIdx.x / (uint32_t)ntx);
  const int x = tx * kBlendTileW + (int)(threadIdx.x & 63) * kBlendPx;
  const int y = ty * kBlendTileH + (int)(threadIdx.x >> 6);
  if (x >= a.iw || y >= a.ih) return;
  // the frame cut to the image, in image coordinates
  const int fx0 = max(a.x0, 0), fx1 = min(a.x0 + a.fw, a.iw);
  const int fy0 = max(a.y0, 0), fy1 = min(a.y0 + a.fh, a.ih);
  const bool tile_meets_frame = tx * kBlendTileW < fx1 && (tx + 1) * kBlendTileW > fx0 && ty * kBlendTileH < fy1 &&
                                (ty + 1) * kBlendTileH > fy0;
  // the source: zeros where the channel's slot is not set
  float4 src[NCH];
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    src[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.src[c]) src[c] = *reinterpret_cast<const float4*>(a.src[c] + (size_t)y * a.src_stride[c] + x);
  }
  if (tile_meets_frame && y >= fy0 && y < fy1 && x < fx1 && x + kBlendPx > fx0) {
    float fg[kBlendPx][NCH], bg[kBlendPx][NCH];
    bool in[kBlendPx];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
      float s[kBlendPx];
      unpack4(src[c], s);
      const float* __restrict__ row = a.frame[c] + (size_t)(y - a.y0) * a.frame_stride[c];
#pragma unroll
      for (int i = 0; i < kBlendPx; i++) {
        in[i] = x + i >= fx0 && x + i < fx1;
        fg[i][c] = s[i];
        bg[i][c] = in[i] ? row[x + i - a.x0] : 0.0f;
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
    for (int i = 0; i < kBlendPx; i++) blend_pixel<NEC>(bg[i], fg[i], a.blend, a.ec_alpha, a.ec_assoc);
#pragma unroll
    for (int c = 0; c < NCH; c++)
      src[c] = make_float4(in[0] ? bg[0][c] : fg[0][c], in[1] ? bg[1][c] : fg[1][c], in[2] ? bg[2][c] : fg[2][c],
                           in[3] ? bg[3][c] : fg[3][c]);
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) *reinterpret_cast<float4*>(a.out[c] + (size_t)y * a.out_stride + x) = src[c];
}

}  // namespace

void launch_blend(hipStream_t s, int num_ec, const BlendLaunch& a) {
  if (a.iw <= 0 || a.ih <= 0) return;
  const int ntx = (a.iw + kBlendTileW - 1) / kBlendTileW, nty = (a.ih + kBlendTileH - 1) / kBlendTileH;
  const dim3 grid((unsigned)((size_t)ntx * nty)), block(256);
  switch (num_ec) {
#define JXLH_BLEND_CASE(N) \
  case N: k_blend<N><<<grid, block, 0, s>>>(a, ntx); break;
    JXLH_BLEND_CASE(0)
    JXLH_BLEND_CASE(1)
    JXLH_BLEND_CASE(2)
    JXLH_BLEND_CASE(3)
    JXLH_BLEND_CASE(4)
    JXLH_BLEND_CASE(5)
    JXLH_BLEND_CASE(6)
    JXLH_BLEND_CASE(7)
    JXLH_BLEND_CASE(8)
#undef JXLH_BLEND_CASE
    default: break;
  }
}

}  // namespace jxlh
