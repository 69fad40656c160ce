// PatchesStage (jxl/src/render/stages/patches.rs -> PatchesDictionary::add_one_row, features/patches.rs:683-759): for
// every pixel, the patches that cover it in dictionary order, each through perform_blending (blend_device.h).
//
// Layout.  The frame is cut into tiles of 64 px x 4 rows; the host bins the dictionary once per jxlh_frame_set_patches
// into a compact list of the tiles at least one patch touches, each with its patch indices in ascending order.  One
// workgroup of 256 threads per listed tile: lane = column, wave = row, so each channel's row segment is one coalesced
// 256 B access.  The patch loop is the same for the whole workgroup, so the descriptors come in through scalar loads.
// A pixel's 3 + NEC values live in registers across its patches and are written back once, and only if a patch
// covered it.  Extra channels are read from their base plane and written to a separate patched plane, so a pass over
// any rows gives the same values however often it runs.
#include "blend_device.h"
#include "jxlh_internal.h"

namespace jxlh {
namespace {

constexpr int kTileW = 64, kTileH = 4;

template <int NEC>
__global__ __launch_bounds__(256) void k_patches(PatchLaunch a, const uint32_t* __restrict__ tiles,
                                                 const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                 const PatchDev* __restrict__ desc) {
  const uint32_t t = a.tile0 + blockIdx.x;
  const uint32_t id = tiles[t];
  const int tx = (int)(id % (uint32_t)a.ntx), ty = (int)(id / (uint32_t)a.ntx);
  const int x = tx * kTileW + (int)(threadIdx.x & 63), y = ty * kTileH + (int)(threadIdx.x >> 6);
  const bool inside = x < a.w && y < a.h;
  float px[3 + NEC];
  if (inside) {
#pragma unroll
    for (int c = 0; c < 3; c++) px[c] = a.col[c][(size_t)y * a.col_stride + x];
#pragma unroll
    for (int i = 0; i < NEC; i++) px[3 + i] = a.ec_in[i][(size_t)y * a.ec_stride[i] + x];
  }
  bool hit = false;
  const uint32_t k1 = start[t + 1];
  for (uint32_t k = start[t]; k < k1; k++) {
    const PatchDev* d = desc + list[k];
    const int dx = x - d->x, dy = y - d->y;
    if (!inside || dx < 0 || dy < 0 || dx >= d->w || dy >= d->h) continue;
    // the slot by a chain of selects on a workgroup-uniform value (no dynamic index into the argument block)
    const int s = d->slot;
    const float* base = s == 0 ? a.ref[0] : s == 1 ? a.ref[1] : s == 2 ? a.ref[2] : a.ref[3];
    const size_t plane = s == 0 ? a.ref_plane[0] : s == 1 ? a.ref_plane[1] : s == 2 ? a.ref_plane[2] : a.ref_plane[3];
    const uint32_t stride = s == 0 ? a.ref_stride[0] : s == 1 ? a.ref_stride[1] : s == 2 ? a.ref_stride[2] : a.ref_stride[3];
    const float* src = base + (size_t)(d->ry + dy) * stride + (d->rx + dx);
    float fg[3 + NEC];
#pragma unroll
    for (int c = 0; c < 3 + NEC; c++) fg[c] = src[(size_t)c * plane];
    blend_pixel<NEC>(px, fg, d->blend, a.ec_alpha, a.ec_assoc);
    hit = true;
  }
  if (!hit) return;
  if (y >= a.cy0 && y < a.cy1) {
#pragma unroll
    for (int c = 0; c < 3; c++) a.col[c][(size_t)y * a.col_stride + x] = px[c];
  }
  if (y >= a.ey0 && y < a.ey1) {
#pragma unroll
    for (int i = 0; i < NEC; i++) a.ec_out[i][(size_t)y * a.ec_stride[i] + x] = px[3 + i];
  }
}

}  // namespace

void launch_patches(hipStream_t s, int num_ec, const PatchLaunch& a, uint32_t ntiles, const uint32_t* tiles,
                    const uint32_t* start, const uint32_t* list, const PatchDev* desc) {
  if (ntiles == 0) return;
  const dim3 grid(ntiles), block(256);
  switch (num_ec) {
#define JXLH_PATCHES_CASE(N) \
  case N: k_patches<N><<<grid, block, 0, s>>>(a, tiles, start, list, desc); break;
    JXLH_PATCHES_CASE(0)
    JXLH_PATCHES_CASE(1)
    JXLH_PATCHES_CASE(2)
    JXLH_PATCHES_CASE(3)
    JXLH_PATCHES_CASE(4)
    JXLH_PATCHES_CASE(5)
    JXLH_PATCHES_CASE(6)
    JXLH_PATCHES_CASE(7)
    JXLH_PATCHES_CASE(8)
#undef JXLH_PATCHES_CASE
    default: break;
  }
}

}  // namespace jxlh
