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
//
// The pieces between load and store live in k_save_pieces.inc, which the rect-list forms (k_save_rects.hip) share.
#include "k_save_pieces.inc"

namespace jxlh {
namespace {

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
