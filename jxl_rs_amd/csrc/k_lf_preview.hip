// The full-size preview of an LF frame (Frame::render_lf_frame_rect, jxl/src/frame/lf_preview.rs:24-274) in ONE pass
// over a rect of an LF slot, everything between load and store in registers:
//   Upsample8x              upsample_device.h (the code of k_upsample.hip), the 5x5 window mirrored against the WHOLE
//                           slot image (lf_preview.rs:127-140)
//   XybStage + FromLinear   color_device.h, as the save tail
//   ConvertF32To*Stage      save_device.h.  The preview builds every converter with ::new(0, ..) and hands every row
//                           over at position (0, 0) (lf_preview.rs:60,67,72,208-214): all three channels are pipeline
//                           channel 0 in row 0 to the dither table, the column counts from the rect's left edge, and
//                           f16 is never clamped
//   save                    channel order RGB / BGR, the opaque fill, endianness, the eight orientations against the image
// Moved per LF pixel: 3 x 4 bytes read (the window's other 72 values come from neighbours' lines in cache), 64 pixels
// written; a route through k_upsample<8> and k_save writes and reads 3 x 64 floats in between.
//
// Layout, as k_upsample<8>: a thread is a short column of kPreviewRows LF pixels -- three 25-value windows slide down in
// registers, the tap weights are indexed uniformly across the wavefront (scalar loads) -- and writes 8 image rows of 8
// contiguous pixels per LF pixel.  A wavefront is 64 neighbouring LF columns.  Orientations 1-4 keep an image row an
// output row: a lane's 8 pixels are one contiguous, dword-packed run (reversed in the lane and in the row for a
// horizontal flip), a wavefront's stores 512 contiguous pixels.  Orientations 5-8 turn image columns into output rows:
// the lane stores pixel by pixel, PB bytes each, 8 KB of output rows apart -- scattered stores, taken as they are (the
// preview of a rotated image is rare and the kernel stays one code path through the arithmetic).
// The 8 rows of a patch are a loop (not unrolled: 600 FMAs and 8 colour conversions per trip are code enough), so no
// register array is indexed with a variable and nothing goes to scratch.
#include "jxlh_internal.h"
#include "save_device.h"
#include "upsample_device.h"

namespace jxlh {
namespace {

constexpr int kPreviewThreads = 256;  // 4 wavefronts: 64 LF columns x 4 runs of kPreviewRows LF rows
constexpr int kPreviewRows = 2;

template <int FMT, int SPP, int MODE>
__global__ __launch_bounds__(kPreviewThreads) __attribute__((amdgpu_waves_per_eu(2, 4))) void k_lf_preview(const LfPreviewLaunch a, const uint32_t nbx) {
  constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
  __shared__ float s_dither[32];  // row 0 of the table: the only one the preview reads
  if constexpr (FMT == kSaveU8) {
    if (threadIdx.x < 32) s_dither[threadIdx.x] = kSaveDitherDev[threadIdx.x];
    __syncthreads();
  }
  const uint32_t bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const int tx = (int)(bx * 64 + (threadIdx.x & 63));
  const int ty0 = (int)(by * (kPreviewThreads / 64) + (threadIdx.x >> 6)) * kPreviewRows;
  if (tx >= a.w || ty0 >= a.h) return;
  const int x = a.x0 + tx, y0 = a.y0 + ty0;
  float win[3][25];
  int xs[5];
  ups_columns(x, a.sw, xs);
  ups_window_prime(a.plane[0], a.stride, a.sh, y0, xs, win[0]);
  ups_window_prime(a.plane[1], a.stride, a.sh, y0, xs, win[1]);
  ups_window_prime(a.plane[2], a.stride, a.sh, y0, xs, win[2]);
  const int X0 = x * 8;  // the patch's first image column; it holds 8 pixels iff X0 + 8 <= a.iw
#pragma unroll 1
  for (int r = 0; r < kPreviewRows; r++) {
    if (ty0 + r >= a.h) break;
    const int y = y0 + r;
    float mn[3], mx[3];
    ups_window_advance(a.plane[0], a.stride, a.sh, y, xs, win[0]);
    ups_window_advance(a.plane[1], a.stride, a.sh, y, xs, win[1]);
    ups_window_advance(a.plane[2], a.stride, a.sh, y, xs, win[2]);
    ups_minmax(win[0], mn[0], mx[0]);
    ups_minmax(win[1], mn[1], mx[1]);
    ups_minmax(win[2], mn[2], mx[2]);
#pragma unroll 1
    for (int oy = 0; oy < 8; oy++) {
      const int Y = y * 8 + oy;
      if (Y >= a.ih) break;
      uint32_t q[8][SPP];
#pragma unroll
      for (int ox = 0; ox < 8; ox++) {  // a pixel at a time: the three channels share an output sample's 25 taps
        const float* __restrict__ k = a.kernels + (oy * 8 + ox) * 25;
        float c[3][1];
        c[0][0] = ups_taps(win[0], mn[0], mx[0], k);
        c[1][0] = ups_taps(win[1], mn[1], mx[1], k);
        c[2][0] = ups_taps(win[2], mn[2], mx[2], k);
        colour_px<MODE, 1>(a.xyb, a.tf, c);
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
          q[ox][ch] = convert_sample<FMT>(a, s_dither, a.bgr ? c[2 - ch][0] : c[ch][0], 8 * tx + ox, 0, 0);
        // keep the pixels apart: interleaved, their eight colour conversions hold some 400 registers live
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (SPP == 4) {
#pragma unroll
        for (int i = 0; i < 8; i++) q[i][3] = a.fill_bits;
      }
      if (!a.transpose) {
        uint8_t* row = a.out + (size_t)(a.flip_y ? a.ih - 1 - Y : Y) * a.out_stride;
        if (X0 + 8 <= a.iw) {
          if (a.flip_x) {
#pragma unroll
            for (int k = 0; k < SPP; k++)
#pragma unroll
              for (int i = 0; i < 4; i++) {
                const uint32_t t = q[i][k];
                q[i][k] = q[7 - i][k];
                q[7 - i][k] = t;
              }
          }
          uint8_t* o = row + (size_t)(a.flip_x ? a.iw - 8 - X0 : X0) * PB;
          if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            uint32_t wd[2 * PB];
            pack_words<BPS, SPP, 8>(q, wd);
            store_words<2 * PB>(o, wd);
          } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
              for (int k = 0; k < SPP; k++) store_sample<BPS>(o + (i * SPP + k) * BPS, q[i][k]);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 8; i++)
            if (X0 + i < a.iw) {
              uint8_t* o = row + (size_t)(a.flip_x ? a.iw - 1 - (X0 + i) : X0 + i) * PB;
#pragma unroll
              for (int k = 0; k < SPP; k++) store_sample<BPS>(o + k * BPS, q[i][k]);
            }
        }
      } else {
        // output (ox, oy) = (Y, X), flipped per axis: image column X0 + i is output row X0 + i
        uint8_t* col = a.out + (size_t)(a.flip_x ? a.ih - 1 - Y : Y) * PB;
#pragma unroll
        for (int i = 0; i < 8; i++)
          if (X0 + i < a.iw) {
            uint8_t* o = col + (size_t)(a.flip_y ? a.iw - 1 - (X0 + i) : X0 + i) * a.out_stride;
#pragma unroll
            for (int k = 0; k < SPP; k++) store_sample<BPS>(o + k * BPS, q[i][k]);
          }
      }
    }
  }
}

template <int FMT, int SPP, int MODE>
void launch_one(hipStream_t s, const LfPreviewLaunch& a) {
  // 1-D grid: no image axis is a grid dimension (iw * ih < 2^31 is checked by the caller, a workgroup covers at least
  // 64 image pixels)
  const uint32_t nbx = (uint32_t)((a.w + 63) / 64);
  const uint32_t rows_per_wg = (kPreviewThreads / 64) * kPreviewRows;
  const uint32_t nby = (uint32_t)((a.h + rows_per_wg - 1) / rows_per_wg);
  k_lf_preview<FMT, SPP, MODE><<<dim3(nbx * nby), dim3(kPreviewThreads), 0, s>>>(a, nbx);
}

template <int FMT, int SPP>
void launch_mode(hipStream_t s, const LfPreviewLaunch& a) {
  switch (a.mode) {
    case kTfSrgb: launch_one<FMT, SPP, kTfSrgb>(s, a); break;
    case kTfBt709: launch_one<FMT, SPP, kTfBt709>(s, a); break;
    case kTfPq: launch_one<FMT, SPP, kTfPq>(s, a); break;
    case kTfHlg: launch_one<FMT, SPP, kTfHlg>(s, a); break;
    case kTfGamma: launch_one<FMT, SPP, kTfGamma>(s, a); break;
    default: break;
  }
}

template <int FMT>
void launch_fmt(hipStream_t s, const LfPreviewLaunch& a) {
  if (a.spp == 4)
    launch_mode<FMT, 4>(s, a);
  else
    launch_mode<FMT, 3>(s, a);
}

}  // namespace

void launch_lf_preview(hipStream_t s, const LfPreviewLaunch& a) {
  if (a.w <= 0 || a.h <= 0) return;
  switch (a.format) {
    case kSaveU8: launch_fmt<kSaveU8>(s, a); break;
    case kSaveU16: launch_fmt<kSaveU16>(s, a); break;
    case kSaveF16: launch_fmt<kSaveF16>(s, a); break;
    case kSaveF32: launch_fmt<kSaveF32>(s, a); break;
    default: break;
  }
}

}  // namespace jxlh
