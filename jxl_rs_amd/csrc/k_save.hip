// The save tail of a frame in ONE pass over the finished planes, everything between load and store in registers:
//   colour stage            color_device.h (XybStage + FromLinearStage / YcbcrToRgbStage), as the read-outs
//   SpotColorStage          jxl/src/render/stages/spot.rs:40-67          (scalar loop: two products and a sum, no FMA)
//   PremultiplyAlphaStage   jxl/src/render/stages/premultiply_alpha.rs:47-92
//   ConvertF32ToU8Stage / ConvertF32ToU16Stage / ConvertF32ToF16Stage    jxl/src/render/stages/convert.rs:570-606,
//                           :743-761, :841-860 at any bit depth; f16::from_f32 of jxl/src/util/float16.rs:82-141 in its
//                           integer form (it truncates into f16 denormals and gives every NaN one payload, which the
//                           hardware conversion does not)
//   save stage              jxl/src/render/save.rs:20-50, simple_pipeline/save.rs:14-89: channel order, endianness,
//                           opaque-alpha fill, the eight orientations of headers/image_metadata.rs:85-96
// The planes are only read: a save can be repeated, and several saves of one frame see the same samples.
//
// Layout.  Orientations 1-4 (k_save_rows) keep a source row an output row: a lane takes four consecutive pixels (one
// 16-byte load per plane), a horizontal flip reverses the four pixels and the lane's place in the row, so a lane's
// 4 x pixel-size bytes stay one contiguous, dword-packed store.  Orientations 5-8 (k_save_tiles) turn source columns
// into output rows: a workgroup converts a tile of kSaveTile columns x 64 (32 for pixels wider than 8 bytes) rows, a wave
// reading 64 consecutive pixels of one source row, and writes the packed pixels into an LDS image of the tile's output
// rows; the image is then read along the output rows, a dword per lane, and stored as dwords.  The image starts at the
// byte offset the tile's output run has inside its first dword (the same for every output row when the row stride is a
// multiple of four), so LDS dwords are global dwords; the one or two partial dwords of a run are stored bytewise, as is
// everything when the stride is not a multiple of four.  An output row of the image is TH * pixel bytes + 4 bytes: an
// odd number of dwords, so the 32 lanes of a ds_write_b32 lane group (32 output rows, the same pixel slot) write 32
// different banks for a 4-byte pixel, and the read side is contiguous.
//
// Format and samples per pixel are template parameters (they decide the register arrays and the packing); colour mode,
// spot count, premultiplication, endianness, clamp and the flips are wavefront-uniform branches.  The launch structure
// is indexed with constants only: a variable index (a channel's plane, the spot list) moves the whole structure to
// private memory.  No instantiation uses scratch.
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

// orientations 1-4: workgroup = 1024 consecutive pixels of one source row, lane = 4 of them
template <int FMT, int SPP>
__global__ __launch_bounds__(kSaveThreads) void k_save_rows(const SaveLaunch a, const uint32_t nbx) {
  constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
  __shared__ float s_dither[FMT == kSaveU8 ? 32 * 32 : 1];
  __shared__ SaveSpot s_spot[JXLH_MAX_EXTRA_CHANNELS];
  load_tables<FMT>(a, s_dither, s_spot);
  const uint32_t bx = blockIdx.x % nbx, r = blockIdx.x / nbx;
  const int x4 = (int)(bx * kSaveThreads + threadIdx.x) * 4;
  if (x4 >= a.w) return;
  const int y = a.y0 + (int)r;
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
  uint8_t* row = a.out + (size_t)oy * a.out_stride;
  if (x4 + 4 <= a.w) {
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
    uint8_t* o = row + (size_t)(a.flip_x ? a.w - 4 - x4 : x4) * PB;
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
      if (x4 + i < a.w) {
        uint8_t* o = row + (size_t)(a.flip_x ? a.w - 1 - (x4 + i) : x4 + i) * PB;
#pragma unroll
        for (int k = 0; k < SPP; k++) store_sample<BPS>(o + k * BPS, q[i][k]);
      }
  }
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

// orientations 5-8: workgroup = one tile of kSaveTile source columns x TH source rows = kSaveTile output rows x TH pixels
template <int FMT, int SPP>
__global__ __launch_bounds__(kSaveThreads) void k_save_tiles(const SaveLaunch a, const uint32_t ntx) {
  constexpr int BPS = sample_bytes<FMT>(), PB = SPP * BPS;
  constexpr int TH = save_tile_rows(PB), PW = TH * PB / 4 + 1;  // dwords per output row of the image: odd
  constexpr int L2 = PB == 1 ? 4 : PB == 2 ? 5 : 6;               // lanes reading one output row: 2^L2 >= TH * PB / 4
  __shared__ uint32_t s_tile[kSaveTile * PW];
  __shared__ float s_dither[FMT == kSaveU8 ? 32 * 32 : 1];
  __shared__ SaveSpot s_spot[JXLH_MAX_EXTRA_CHANNELS];
  load_tables<FMT>(a, s_dither, s_spot);
  const int tx = (int)(blockIdx.x % ntx), ty = (int)(blockIdx.x / ntx);
  const int xa = tx * kSaveTile, ya = a.y0 + ty * TH;
  const int yb = min(ya + TH, a.y0 + a.rows), nr = yb - ya, nc = min(kSaveTile, a.w - xa);
  // the tile's run inside an output row: nr pixels from output column oxs on
  const int oxs = a.flip_x ? a.h - yb : ya;
  const bool aligned = (a.out_stride & 3) == 0;
  const uint32_t sh = aligned ? (uint32_t)((reinterpret_cast<uintptr_t>(a.out) + (size_t)oxs * PB) & 3) : 0u;
  const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
  if (lane < nc) {
    const SaveTile t = {xa, ya, nr, lane, wave, sh, s_spot};
    using Convert = tile_convert<FMT, SPP>;
    JXLH_SAVE_MODE_SWITCH(a.colour ? a.mode : (int)kModeNone, Convert::template run, a, t, s_dither, s_tile)
  }
  __syncthreads();
  const uint32_t nb = sh + (uint32_t)nr * PB, nd = (nb + 3) / 4;  // bytes / dwords of an output row's image (nd <= PW)
  const uint32_t sub = threadIdx.x & ((1u << L2) - 1);
  for (int c = (int)(threadIdx.x >> L2); c < nc; c += kSaveThreads >> L2) {
    const int oy = a.flip_y ? a.w - 1 - (xa + c) : xa + c;
    uint8_t* o = a.out + (size_t)oy * a.out_stride + (size_t)oxs * PB - sh;  // the image's byte 0
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
void launch_fmt_spp(hipStream_t s, const SaveLaunch& a) {
  constexpr int PB = SPP * sample_bytes<FMT>();
  if (a.transpose) {
    const uint32_t ntx = (uint32_t)((a.w + kSaveTile - 1) / kSaveTile);
    const uint32_t nty = (uint32_t)((a.rows + save_tile_rows(PB) - 1) / save_tile_rows(PB));
    k_save_tiles<FMT, SPP><<<dim3(ntx * nty), dim3(kSaveThreads), 0, s>>>(a, ntx);
  } else {
    const uint32_t nbx = (uint32_t)(((a.w + 3) / 4 + kSaveThreads - 1) / kSaveThreads);
    k_save_rows<FMT, SPP><<<dim3(nbx * (uint32_t)a.rows), dim3(kSaveThreads), 0, s>>>(a, nbx);
  }
}

template <int FMT>
void launch_fmt(hipStream_t s, const SaveLaunch& a) {
  switch (a.spp) {
    case 1: launch_fmt_spp<FMT, 1>(s, a); break;
    case 2: launch_fmt_spp<FMT, 2>(s, a); break;
    case 3: launch_fmt_spp<FMT, 3>(s, a); break;
    case 4: launch_fmt_spp<FMT, 4>(s, a); break;
    default: break;
  }
}

}  // namespace

// No image axis is a grid dimension; the 1-D grids (row blocks x rows, tiles) must stay below 2^31 workgroups.  The save
// entry points refuse w * h >= 2^31; the read-outs' case is argued at save_result_rows (abi_save.hip).
void launch_save(hipStream_t s, const SaveLaunch& a) {
  if (a.w <= 0 || a.rows <= 0) return;
  switch (a.format) {
    case kSaveU8: launch_fmt<kSaveU8>(s, a); break;
    case kSaveU16: launch_fmt<kSaveU16>(s, a); break;
    case kSaveF16: launch_fmt<kSaveF16>(s, a); break;
    case kSaveF32: launch_fmt<kSaveF32>(s, a); break;
    default: break;
  }
}

}  // namespace jxlh
