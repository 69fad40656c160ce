// The pieces the save kernels are made of, shared by k_save.hip (row bands) and k_save_rects.hip (rectangle lists), so
// that the two cannot differ in a sample: the loads, the colour stage's dispatch, spot colours and premultiplication,
// the conversion of a pixel's samples, the workgroup's tables, and the tile kernels' conversion into the LDS image.
// k_save.hip's header comment describes the layout and the constraints they were written under.
#pragma once
#include "jxlh_internal.h"
#include "save_device.h"

namespace jxlh {
namespace {

constexpr int kSaveThreads = 256;

// NPX consecutive samples of row y from x on, zeros past the row's end
template <int NPX>
__device__ __forceinline__ void load_px(const float* __restrict__ p, uint32_t stride, int x, int y, int w, float (&o)[NPX]) {
  const float* __restrict__ row = p + (size_t)y * stride + x;
  if constexpr (NPX == 4) {
    if (x + 4 <= w && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(row);
      o[0] = v.x;
      o[1] = v.y;
      o[2] = v.z;
      o[3] = v.w;
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < NPX; i++) o[i] = x + i < w ? row[i] : 0.0f;
}

// the colour planes of NPX consecutive pixels of source row y from x on, through the colour stage MODE
template <int MODE, int NPX>
__device__ __forceinline__ void load_colour(const SaveLaunch& a, int x, int y, float (&c)[3][NPX]) {
  load_px<NPX>(a.plane[0], a.stride[0], x, y, a.w, c[0]);
  load_px<NPX>(a.plane[1], a.stride[1], x, y, a.w, c[1]);
  load_px<NPX>(a.plane[2], a.stride[2], x, y, a.w, c[2]);
  colour_px<MODE, NPX>(a.xyb, a.tf, c);
}

// The spot colour list lives in LDS: the loop over it indexes with a variable, which on the launch structure would move
// the whole structure to private memory, and unrolled over the structure it costs 56 scalar registers.
struct SaveSpot {
  const float* plane;
  uint32_t stride;
  float rgba[4];
};

// ... then the spot colours in list order (spot.rs:61-66) and the premultiplication
template <int NPX>
__device__ __forceinline__ void spot_premultiply(const SaveLaunch& a, const SaveSpot* __restrict__ s_spot, int x, int y,
                                                 float (&c)[3][NPX]) {
  for (int s = 0; s < a.n_spot; s++) {
    const SaveSpot sp = s_spot[s];
    float sv[NPX];
    load_px<NPX>(sp.plane, sp.stride, x, y, a.w, sv);
#pragma unroll
    for (int i = 0; i < NPX; i++) {
      const float mix = sp.rgba[3] * sv[i];
#pragma unroll
      for (int k = 0; k < 3; k++) c[k][i] = mix * sp.rgba[k] + (1.0f - mix) * c[k][i];
    }
  }
  if (a.premul_plane) {
    float al[NPX];
    load_px<NPX>(a.premul_plane, a.premul_stride, x, y, a.w, al);
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int i = 0; i < NPX; i++) c[k][i] = c[k][i] * al[i];
  }
}

// ... and the SPP samples of each pixel: colour channels from c, extra channels from their planes, the opaque fill
template <int FMT, int SPP, int NPX>
__device__ __forceinline__ void convert_pixels(const SaveLaunch& a, const float* __restrict__ dither, int x, int y,
                                               const float (&c)[3][NPX], uint32_t (&q)[NPX][SPP]) {
#pragma unroll
  for (int k = 0; k < SPP; k++) {
    const int ch = a.ch[k];  // the same for every lane, like every branch on `a`
    if (ch == kSaveFill) {
#pragma unroll
      for (int i = 0; i < NPX; i++) q[i][k] = a.fill_bits;
      continue;
    }
    float v[NPX];
    if (ch < 3) {
#pragma unroll
      for (int i = 0; i < NPX; i++) {  // three reads and a select on values: no indexing of c by ch
        const float c0 = c[0][i], c1 = c[1][i], c2 = c[2][i];
        v[i] = ch == 0 ? c0 : ch == 1 ? c1 : c2;
      }
    } else {
      load_px<NPX>(a.smp_plane[k], a.smp_stride[k], x, y, a.w, v);
    }
#pragma unroll
    for (int i = 0; i < NPX; i++) q[i][k] = convert_sample<FMT>(a, dither, v[i], x + i + a.dx, y + a.dy, ch);
  }
}

// a.mode (never read without a colour channel named: kModeNone then) as a template argument of F
#define JXLH_SAVE_MODE_SWITCH(mode, F, ...)                 \
  switch (mode) {                                           \
    case kTfLinear: F<kTfLinear>(__VA_ARGS__); break;       \
    case kTfSrgb: F<kTfSrgb>(__VA_ARGS__); break;           \
    case kTfBt709: F<kTfBt709>(__VA_ARGS__); break;         \
    case kTfPq: F<kTfPq>(__VA_ARGS__); break;               \
    case kTfHlg: F<kTfHlg>(__VA_ARGS__); break;             \
    case kTfGamma: F<kTfGamma>(__VA_ARGS__); break;         \
    case kModeYcbcr: F<kModeYcbcr>(__VA_ARGS__); break;     \
    default: F<kModeNone>(__VA_ARGS__); break;              \
  }

template <int MODE>
__device__ __forceinline__ void colour4(const XybParamsDev& p, const TfParamsDev& t, float (&c)[3][4]) {
  colour_px<MODE, 4>(p, t, c);
}

// the workgroup's tables: the dither table (U8 only) and the spot list
template <int FMT>
__device__ __forceinline__ void load_tables(const SaveLaunch& a, float* s_dither, SaveSpot* s_spot) {
  if constexpr (FMT == kSaveU8)
    for (int i = threadIdx.x; i < 32 * 32; i += kSaveThreads) s_dither[i] = kSaveDitherDev[i];
  if (FMT != kSaveU8 && a.n_spot == 0) return;
#pragma unroll
  for (int s = 0; s < JXLH_MAX_EXTRA_CHANNELS; s++)
    if ((int)threadIdx.x == s && s < a.n_spot) {
      s_spot[s].plane = a.spot_plane[s];
      s_spot[s].stride = a.spot_stride[s];
#pragma unroll
      for (int k = 0; k < 4; k++) s_spot[s].rgba[k] = a.spot[s][k];
    }
  __syncthreads();
}

// the first half of k_save_tiles: this wave's rows of the tile, a lane a pixel, converted and written into the LDS image.
// The colour mode is a template argument HERE, around the row loop: with the switch inside the loop the constants of all
// seven curves are live across it and the scalar registers spill.
struct SaveTile {
  int xa, ya, nr, lane, wave;
  uint32_t sh;
  const SaveSpot* spot;
};
template <int FMT, int SPP>
struct tile_convert {
  template <int MODE>
  static __device__ __forceinline__ void run(const SaveLaunch& a, const SaveTile& t, const float* __restrict__ s_dither,
                                             uint32_t* __restrict__ s_tile) {
    constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
    constexpr int TH = save_tile_rows(PB), PW = TH * PB / 4 + 1;
    uint8_t* tile8 = reinterpret_cast<uint8_t*>(s_tile);
    for (int r = t.wave; r < t.nr; r += kSaveThreads / 64) {
      const int x = t.xa + t.lane, y = t.ya + r;
      float c[3][1] = {{0.0f}, {0.0f}, {0.0f}};
      if (a.colour) {
        load_colour<MODE, 1>(a, x, y, c);
        spot_premultiply<1>(a, t.spot, x, y, c);
      }
      uint32_t q[1][SPP];
      convert_pixels<FMT, SPP, 1>(a, s_dither, x, y, c, q);
      const uint32_t at = (uint32_t)t.lane * (PW * 4) + t.sh + (uint32_t)(a.flip_x ? t.nr - 1 - r : r) * PB;
      if constexpr (PB % 4 == 0) {
        if (t.sh == 0) {
          uint32_t wd[PB / 4];
          pack_words<BPS, SPP, 1>(q, wd);
#pragma unroll
          for (int n = 0; n < PB / 4; n++) s_tile[at / 4 + n] = wd[n];
          continue;
        }
      }
#pragma unroll
      for (int k = 0; k < SPP; k++) store_sample<BPS>(tile8 + at + k * BPS, q[0][k]);
    }
  }
};

}  // namespace
}  // namespace jxlh
