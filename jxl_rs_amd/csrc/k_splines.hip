// SplinesStage (jxl/src/render/stages/splines.rs -> Splines::draw_segments, features/spline.rs:523-656): every segment
// of the draw cache adds a Gaussian-like blob to the three colour planes, draw_segment_inner's FMA form bit for bit.
//
// Layout, as k_patches.hip: the plane is cut into bins of 64 px x 4 rows; the host bins a batch of consecutive segments
// into a compact list of the bins at least one of them touches, each with its segment indices ascending -- per pixel
// the order of the reference's stable sort by row.  One workgroup of 256 threads per listed bin: lane = column,
// wave = row.  The segment loop is the same for the whole workgroup, so the descriptors come in through scalar loads.
// A pixel's three values live in registers across the bin's segments and are written back once, and only if a segment
// touched it (an untouched -0.0 stays what it is).  Batches are launched in segment order on one stream: accumulating
// through memory between them gives the same bits.
//
// Arithmetic: sqrtf and the division are the correctly rounded ones (the compiler's default for HIP), only fmaf fuses
// (-ffp-contract=off).
#include "jxlh_internal.h"

namespace jxlh {
namespace {

// fast_erff_simd (util/fast_math.rs:64-77)
__device__ __forceinline__ float spline_erf(float v) {
  const float t = fabsf(v);
  const float p =
      fmaf(fmaf(fmaf(fmaf(t, 7.77394369e-02f, 2.05260015e-04f), t, 2.32120216e-01f), t, 2.77820801e-01f), t, 1.0f);
  const float q = 1.0f / (p * p);
  return copysignf(1.0f - q * q, v);
}

__global__ __launch_bounds__(256) void k_splines(SplineLaunch a, const uint32_t* __restrict__ bins,
                                                 const uint32_t* __restrict__ start, const uint32_t* __restrict__ list,
                                                 const SplineDev* __restrict__ seg) {
  const uint32_t t = a.bin0 + blockIdx.x;
  const uint32_t id = bins[t];
  const int tx = (int)(id % (uint32_t)a.ntx), ty = (int)(id / (uint32_t)a.ntx);
  const int x = tx * kSplineBinW + (int)(threadIdx.x % kSplineBinW), y = ty * kSplineBinH + (int)(threadIdx.x / kSplineBinW);
  const bool inside = x < a.w && y < a.h && y >= a.y0 && y < a.y1;
  const size_t at = (size_t)y * a.stride + x;
  float px[3] = {0.0f, 0.0f, 0.0f};
  if (inside) {
#pragma unroll
    for (int c = 0; c < 3; c++) px[c] = a.col[c][at];
  }
  const float fx = (float)x, fy = (float)y;
  bool hit = false;
  const uint32_t k1 = start[t + 1];
  for (uint32_t k = start[t]; k < k1; k++) {
    // three dependent scalar loads per segment: its index, its four bounds (one s_load_dwordx4), and -- only when some
    // lane is inside -- the other eight words
    const SplineDev d = seg[list[k]];
    if (!inside || x < d.x0 || x >= d.x1 || y < d.y0 || y >= d.y1) continue;
    const float dy = fy - d.cy, dx = fx - d.cx;
    const float dist = sqrtf(fmaf(dx, dx, dy * dy));
    const float a1 = fmaf(dist, 0.5f, 0.35355338f) * d.inv_sigma;
    const float a2 = fmaf(dist, 0.5f, -0.35355338f) * d.inv_sigma;
    const float f = spline_erf(a1) - spline_erf(a2);
    const float li = (d.s4i * f) * f;
#pragma unroll
    for (int c = 0; c < 3; c++) px[c] = fmaf(d.color[c], li, px[c]);
    hit = true;
  }
  if (!hit) return;
#pragma unroll
  for (int c = 0; c < 3; c++) a.col[c][at] = px[c];
}

}  // namespace

void launch_splines(hipStream_t s, const SplineLaunch& a, uint32_t nbins, const uint32_t* bins, const uint32_t* start,
                    const uint32_t* list, const SplineDev* seg) {
  if (nbins == 0) return;
  k_splines<<<dim3(nbins), dim3(256), 0, s>>>(a, bins, start, list, seg);
}

}  // namespace jxlh
