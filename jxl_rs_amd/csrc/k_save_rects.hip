// The rect-list forms of the save kernels (jxlh_frame_save_rects, jxlh_stage_save_rects): the pixels of a list of source
// rectangles in ONE launch, through the pieces k_save.hip's kernels are made of (k_save_pieces.inc), so the samples
// cannot differ from the band save.  A translation unit of its own: with these kernels next to them, the compiler
// allocated the registers of 14 of k_save.hip's 16 tile kernels differently, and those kernels serve the read-outs and
// jxlh_frame_save with measured times; built apart, all 32 keep their instruction streams.
#include "k_save_pieces.inc"
#include "save_rects_plan.h"

namespace jxlh {
namespace {

// The list (save_rects_plan.h) lives in device memory, not in SaveLaunch -- a variable index would move that structure
// to private memory --, and a workgroup's rect depends on blockIdx alone, so the bisection and the descriptor are scalar
// loads.  Every rect carries its own destination origin and pitch: the caller's image, or its block of the staging
// buffer.

// the rect of workgroup g: the last one whose first workgroup is <= g
__device__ __forceinline__ SaveRectWork find_rect(const SaveRectWork* __restrict__ work, uint32_t n, uint32_t g) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (work[mid].first <= g) lo = mid;
    else hi = mid;
  }
  return work[lo];
}

// orientations 1-4: workgroup = kRectRowsPerGroup source rows of a rect (a wave each) x kRectRowPixels pixels from the
// rect's x0 rounded down to a multiple of four: a lane's four pixels stay one 16-byte load per plane and, inside the
// rect, one dword-packed store as in k_save_rows; the pixels of a lane that straddles the rect's left or right edge
// are stored sample by sample, so no byte outside the rect is written.
template <int FMT, int SPP>
__global__ __launch_bounds__(kSaveThreads) void k_save_rows_rects(const SaveLaunch a, const SaveRectWork* __restrict__ work,
                                                                  const uint32_t n) {
  static_assert(kSaveThreads == 64 * kRectRowsPerGroup && kRectRowPixels == 64 * 4, "a wave a row, a lane four pixels");
  constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
  __shared__ float s_dither[FMT == kSaveU8 ? 32 * 32 : 1];
  __shared__ SaveSpot s_spot[JXLH_MAX_EXTRA_CHANNELS];
  load_tables<FMT>(a, s_dither, s_spot);
  const SaveRectWork r = find_rect(work, n, blockIdx.x);
  const uint32_t local = blockIdx.x - r.first, bx = local % r.nbx, by = local / r.nbx;
  const uint32_t row = by * kRectRowsPerGroup + (threadIdx.x >> 6);
  if (row >= r.h) return;
  const int y = (int)(r.y0 + row);
  const int xl = (int)r.x0, xr = (int)(r.x0 + r.w);  // the rect's columns [xl, xr)
  const int x4 = (int)((r.x0 & ~3u) + (bx * 64 + (threadIdx.x & 63)) * 4);
  if (x4 >= xr || x4 + 4 <= xl) return;
  float c[3][4];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int i = 0; i < 4; i++) c[k][i] = 0.0f;
  if (a.colour) {
    load_px<4>(a.plane[0], a.stride[0], x4, y, a.w, c[0]);
    load_px<4>(a.plane[1], a.stride[1], x4, y, a.w, c[1]);
    load_px<4>(a.plane[2], a.stride[2], x4, y, a.w, c[2]);
    JXLH_SAVE_MODE_SWITCH(a.mode, colour4, a.xyb, a.tf, c)
    spot_premultiply<4>(a, s_spot, x4, y, c);
  }
  uint32_t q[4][SPP];
  convert_pixels<FMT, SPP, 4>(a, s_dither, x4, y, c, q);
  const int oy = a.flip_y ? a.h - 1 - y : y;
  uint8_t* orow = a.out + r.origin + (size_t)oy * r.pitch;
  if (x4 >= xl && x4 + 4 <= xr) {
    if (a.flip_x) {
#pragma unroll
      for (int k = 0; k < SPP; k++) {
        const uint32_t t0 = q[0][k], t1 = q[1][k];
        q[0][k] = q[3][k];
        q[1][k] = q[2][k];
        q[2][k] = t1;
        q[3][k] = t0;
      }
    }
    uint8_t* o = orow + (size_t)(a.flip_x ? a.w - 4 - x4 : x4) * PB;
    if ((reinterpret_cast<uintptr_t>(o) & 3) == 0) {
      uint32_t wd[PB];
      pack_words<BPS, SPP, 4>(q, wd);
      store_words<PB>(o, wd);
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int k = 0; k < SPP; k++) store_sample<BPS>(o + (i * SPP + k) * BPS, q[i][k]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (x4 + i >= xl && x4 + i < xr) {
        uint8_t* o = orow + (size_t)(a.flip_x ? a.w - 1 - (x4 + i) : x4 + i) * PB;
#pragma unroll
        for (int k = 0; k < SPP; k++) store_sample<BPS>(o + k * BPS, q[i][k]);
      }
  }
}

// orientations 5-8: workgroup = one tile of k_save_tiles' size, laid from the rect's own corner; the tile's run in an
// output row is stored as k_save_tiles stores it, dwords inside and bytes at its two ends
template <int FMT, int SPP>
__global__ __launch_bounds__(kSaveThreads) void k_save_tiles_rects(const SaveLaunch a, const SaveRectWork* __restrict__ work,
                                                                   const uint32_t n) {
  constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
  constexpr int TH = save_tile_rows(PB), PW = TH * PB / 4 + 1;  // dwords per output row of the image: odd
  constexpr int L2 = PB == 1 ? 4 : PB == 2 ? 5 : 6;               // lanes reading one output row: 2^L2 >= TH * PB / 4
  static_assert(kSaveTile == (int)kRectTileCols && TH == (int)rect_tile_rows(PB), "the plan's tile is the kernel's");
  __shared__ uint32_t s_tile[kSaveTile * PW];
  __shared__ float s_dither[FMT == kSaveU8 ? 32 * 32 : 1];
  __shared__ SaveSpot s_spot[JXLH_MAX_EXTRA_CHANNELS];
  load_tables<FMT>(a, s_dither, s_spot);
  const SaveRectWork r = find_rect(work, n, blockIdx.x);
  const uint32_t local = blockIdx.x - r.first;
  const int tx = (int)(local % r.nbx), ty = (int)(local / r.nbx);
  const int xa = (int)r.x0 + tx * kSaveTile, ya = (int)r.y0 + ty * TH;
  const int yb = min(ya + TH, (int)(r.y0 + r.h)), nr = yb - ya, nc = min(kSaveTile, (int)(r.x0 + r.w) - xa);
  uint8_t* const image = a.out + r.origin;
  const size_t pitch = (size_t)r.pitch;
  const int oxs = a.flip_x ? a.h - yb : ya;
  const bool aligned = (pitch & 3) == 0;
  const uint32_t sh = aligned ? (uint32_t)((reinterpret_cast<uintptr_t>(image) + (size_t)oxs * PB) & 3) : 0u;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  if (lane < nc) {
    const SaveTile t = {xa, ya, nr, lane, wave, sh, s_spot};
    using Convert = tile_convert<FMT, SPP>;
    JXLH_SAVE_MODE_SWITCH(a.colour ? a.mode : (int)kModeNone, Convert::template run, a, t, s_dither, s_tile)
  }
  __syncthreads();
  const uint32_t nb = sh + (uint32_t)nr * PB, nd = (nb + 3) / 4;
  const uint32_t sub = threadIdx.x & ((1u << L2) - 1);
  for (int c = (int)(threadIdx.x >> L2); c < nc; c += kSaveThreads >> L2) {
    const int oy = a.flip_y ? a.w - 1 - (xa + c) : xa + c;
    uint8_t* o = image + (size_t)oy * pitch + (size_t)oxs * PB - sh;  // the image's byte 0
    for (uint32_t j = sub; j < nd; j += 1u << L2) {
      const uint32_t wd = s_tile[c * PW + j];
      const uint32_t lo = max(sh, 4 * j), hi = min(nb, 4 * j + 4);
      if (aligned && hi - lo == 4) {
        *reinterpret_cast<uint32_t*>(o + 4 * j) = wd;
      } else {
        for (uint32_t b = lo; b < hi; b++) o[b] = (uint8_t)(wd >> (8 * (b - 4 * j)));
      }
    }
  }
}

template <int FMT, int SPP>
void launch_rects_fmt_spp(hipStream_t s, const SaveLaunch& a, const SaveRectWork* work, uint32_t n, uint32_t groups) {
  if (a.transpose)
    k_save_tiles_rects<FMT, SPP><<<dim3(groups), dim3(kSaveThreads), 0, s>>>(a, work, n);
  else
    k_save_rows_rects<FMT, SPP><<<dim3(groups), dim3(kSaveThreads), 0, s>>>(a, work, n);
}

template <int FMT>
void launch_rects_fmt(hipStream_t s, const SaveLaunch& a, const SaveRectWork* work, uint32_t n, uint32_t groups) {
  switch (a.spp) {
    case 1: launch_rects_fmt_spp<FMT, 1>(s, a, work, n, groups); break;
    case 2: launch_rects_fmt_spp<FMT, 2>(s, a, work, n, groups); break;
    case 3: launch_rects_fmt_spp<FMT, 3>(s, a, work, n, groups); break;
    case 4: launch_rects_fmt_spp<FMT, 4>(s, a, work, n, groups); break;
    default: break;
  }
}

}  // namespace

// jxlh_frame_save_rects: the n rects of the device-resident list `work` in one launch of `groups` workgroups
// (save_rects_plan.h: below 2^31); a.y0 / a.rows / a.out_stride are not read
void launch_save_rects(hipStream_t s, const SaveLaunch& a, const SaveRectWork* work, uint32_t n, uint32_t groups) {
  if (n == 0 || groups == 0) return;
  switch (a.format) {
    case kSaveU8: launch_rects_fmt<kSaveU8>(s, a, work, n, groups); break;
    case kSaveU16: launch_rects_fmt<kSaveU16>(s, a, work, n, groups); break;
    case kSaveF16: launch_rects_fmt<kSaveF16>(s, a, work, n, groups); break;
    case kSaveF32: launch_rects_fmt<kSaveF32>(s, a, work, n, groups); break;
    default: break;
  }
}

}  // namespace jxlh
