// The frame planner (jxl_rs_amd/csrc/frame_plan.h) against the code it replaced: the top of jxlh_frame_begin
// (abi_frame.hip) and modular_frame_begin (abi_modular_frame.hip), transcribed below as they were -- the argument
// checks, the geometry, the two bounds, the size of every allocation, the host-evaluated scalars -- with their own
// constants, none of them from the header.  Compared field for field over an enumeration of parameters, plus the
// invariants of an accepted plan.  Host only, no device; also built on its own under the address and undefined-behaviour
// sanitizers (tests/test_frame_plan_cpu.py).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../jxl_rs_amd/csrc/frame_plan.h"

namespace {

int g_fail = 0;
long g_cases = 0, g_ok = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      if (g_fail++ < 20) {                     \
        std::printf("FAIL %s: ", #c);          \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

// ---- the old code's world
namespace old {
constexpr int kGroupDim = 256;
constexpr int kGroupArea = 256 * 256;
inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
struct FrameDev {
  int xsize, ysize, xblocks, yblocks, subsampled, hshift[3], vshift[3], xgroups, ygroups, cmap_stride, scrap_off;
  size_t plane_stride;
  float inv_global_scale, x_dm, b_dm;
  int se_direct_ok;
};
struct Begin {
  jxlh_status status;
  bool modular;
  FrameDev f;
  size_t ngroups, plane_elems, gather_elems, nblocks, ncmap;
  int rows_per_rank;
  // the ensure() calls, in the names of their buffers; the arguments of choose_placement
  size_t planes, tmp, lf_raw, lf_sm, sigma, coeffs, raw_quant, transform_map, epf_map, ytox, ytob, mod_src;
  size_t place_plane, place_tmp, place_coeffs, place_probe;
  bool params_direct_ok;
};
int comm_rows_per_rank(int nranks, int ygroups) {
  const int n = nranks;
  return (ygroups + n - 1) / n;
}

Begin frame_begin(const jxlh_frame_params* p, int nranks, bool off) {
  Begin b;
  std::memset(&b, 0, sizeof b);
  b.status = JXLH_ERR_INVALID_ARGUMENT;
  if (!p || p->abi_version != JXLH_ABI_VERSION) return b;
  if (p->xsize == 0 || p->ysize == 0 || p->xsize > (1u << 20) || p->ysize > (1u << 20) || p->global_scale == 0 ||
      p->quant_lf == 0 || p->color_factor == 0 || p->epf_iters > 3)
    return b;
  if (p->upsampling > 1 && p->upsampling != 2 && p->upsampling != 4 && p->upsampling != 8) return b;
  if (p->upsampling > 1) {
    const uint32_t n = p->upsampling;
    if (p->xsize_upsampled > p->xsize * n || p->ysize_upsampled > p->ysize * n ||
        (p->xsize_upsampled && (p->xsize_upsampled + n - 1) / n != p->xsize) ||
        (p->ysize_upsampled && (p->ysize_upsampled + n - 1) / n != p->ysize))
      return b;
  }
  uint32_t maxhs = 0, maxvs = 0;
  for (int c = 0; c < 3; c++) {
    if (p->hshift[c] > 1 || p->vshift[c] > 1) return b;
    maxhs |= p->hshift[c];
    maxvs |= p->vshift[c];
  }
  const bool modular = (p->flags & JXLH_FRAME_MODULAR) != 0;
  b.modular = modular;
  if (modular) {
    if (p->epf_iters > 0 && !(p->epf_sigma_for_modular > 0.0f)) return b;
    if (nranks > 1) {
      b.status = JXLH_ERR_UNSUPPORTED;
      return b;
    }
  }
  FrameDev& f = b.f;
  f.xsize = (int)p->xsize;
  f.ysize = (int)p->ysize;
  f.xblocks = (int)(((p->xsize + (8u << maxhs) - 1) / (8u << maxhs)) << maxhs);
  f.yblocks = (int)(((p->ysize + (8u << maxvs) - 1) / (8u << maxvs)) << maxvs);
  f.subsampled = (maxhs | maxvs) != 0;
  for (int c = 0; c < 3; c++) {
    f.hshift[c] = (int)p->hshift[c];
    f.vshift[c] = (int)p->vshift[c];
  }
  f.xgroups = (int)((p->xsize + kGroupDim - 1) / kGroupDim);
  f.ygroups = (int)((p->ysize + kGroupDim - 1) / kGroupDim);
  f.cmap_stride = (f.xblocks + 7) / 8;
  f.plane_stride = round_up((size_t)f.xblocks * 8, 64);
  const size_t plane_elems = f.plane_stride * (size_t)f.yblocks * 8;
  const size_t gather_elems = (size_t)nranks * comm_rows_per_rank(nranks, f.ygroups) * kGroupDim * f.plane_stride;
  b.plane_elems = plane_elems;
  b.gather_elems = gather_elems;
  b.rows_per_rank = comm_rows_per_rank(nranks, f.ygroups);
  if (plane_elems >= (1ull << 30) || (!modular && (size_t)f.xgroups * f.ygroups * 3 * kGroupArea >= (1ull << 31))) {
    b.status = JXLH_ERR_UNSUPPORTED;
    return b;
  }
  b.ngroups = (size_t)f.xgroups * f.ygroups;
  b.status = JXLH_OK;
  if (modular) {  // modular_frame_begin
    const size_t plane_elems2 = f.plane_stride * (size_t)f.yblocks * 8;
    const size_t nblocks = (size_t)f.xblocks * f.yblocks;
    b.nblocks = nblocks;
    b.planes = plane_elems2;
    b.tmp = plane_elems2;
    b.mod_src = plane_elems2;
    b.sigma = nblocks;
    f.scrap_off = (int)plane_elems2;
  } else {
    const size_t nblocks = (size_t)f.xblocks * f.yblocks;
    const size_t ncmap = (size_t)f.cmap_stride * ((f.yblocks + 7) / 8);
    b.nblocks = nblocks;
    b.ncmap = ncmap;
    b.place_plane = std::max(plane_elems, gather_elems);
    b.place_tmp = std::max(plane_elems + 8 * f.plane_stride, gather_elems);
    b.place_coeffs = b.ngroups * 3 * kGroupArea;
    b.place_probe = plane_elems & ~(size_t)511;  // (choose_placement rounds what it is given)
    b.planes = std::max(plane_elems, gather_elems);
    b.tmp = std::max(plane_elems + 8 * f.plane_stride, gather_elems);
    b.lf_raw = nblocks;
    b.lf_sm = nblocks;
    b.sigma = nblocks;
    b.coeffs = b.ngroups * 3 * kGroupArea;
    b.raw_quant = nblocks;
    b.transform_map = nblocks;
    b.epf_map = nblocks;
    b.ytox = ncmap;
    b.ytob = ncmap;
    f.scrap_off = (int)plane_elems;
  }
  f.inv_global_scale = (float)(1 << 16) / (float)p->global_scale;
  f.x_dm = powf(1.0f / 1.25f, (float)p->x_qm_scale - 2.0f);
  f.b_dm = powf(1.0f / 1.25f, (float)p->b_qm_scale - 2.0f);
  const float base_x = p->base_correlation_x, base_b = p->base_correlation_b;
  {
    auto fin = [](float v) { return v == v && v > -3.0e38f && v < 3.0e38f; };
    auto bias_ok = [](float v) { return v >= 1e-6f && v <= 1e6f; };
    f.se_direct_ok = bias_ok(p->quant_biases[0]) && bias_ok(p->quant_biases[1]) && bias_ok(p->quant_biases[2]) &&
                     fin(p->quant_biases[3]) && fin(base_x) && fin(base_b) && !(p->flags & JXLH_FRAME_DENSE_DEQUANT);
    for (int i = 2; i < 128 && f.se_direct_ok; i++)
      if ((float)i - p->quant_biases[3] / (float)i == 0.0f) f.se_direct_ok = 0;
    if (off) f.se_direct_ok = 0;
    b.params_direct_ok = f.se_direct_ok != 0;
  }
  return b;
}
}  // namespace old

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// jxlh_default_frame_params' values that the planner reads (the library is not linked into the sanitizer build)
jxlh_frame_params base_params(uint32_t xsize, uint32_t ysize) {
  jxlh_frame_params p;
  std::memset(&p, 0, sizeof p);
  p.abi_version = JXLH_ABI_VERSION;
  p.xsize = xsize;
  p.ysize = ysize;
  p.global_scale = 21845;
  p.quant_lf = 16;
  p.quant_biases[0] = 1.0f - 0.05465007330715401f;
  p.quant_biases[1] = 1.0f - 0.07005449891748593f;
  p.quant_biases[2] = 1.0f - 0.049935103337343655f;
  p.quant_biases[3] = 0.145f;
  p.x_qm_scale = 3;
  p.b_qm_scale = 2;
  p.color_factor = 84;
  p.base_correlation_x = 0.0f;
  p.base_correlation_b = 1.0f;
  p.gab = 1;
  p.epf_iters = 2;
  p.epf_sigma_for_modular = 1.0f;
  return p;
}

// plan == transcription, field for field; the invariants of an accepted plan.  -> the status
jxlh_status check(const jxlh_frame_params& p, int nranks, bool off) {
  using jxlh::FramePlan;
  const FramePlan pl = jxlh::plan_frame(p, nranks, off);
  const old::Begin b = old::frame_begin(&p, nranks, off);
  g_cases++;
  const unsigned xs = p.xsize, ys = p.ysize, fl = p.flags;
  CHECK(pl.status == b.status, "%u x %u flags %u ranks %d: %d vs %d", xs, ys, fl, nranks, (int)pl.status, (int)b.status);
  if (pl.status != JXLH_OK || b.status != JXLH_OK) return pl.status;
  g_ok++;
  const old::FrameDev& f = b.f;
  CHECK(pl.modular == b.modular, "%u x %u", xs, ys);
  CHECK(pl.xblocks == f.xblocks && pl.yblocks == f.yblocks, "%u x %u: %d %d vs %d %d", xs, ys, pl.xblocks, pl.yblocks,
        f.xblocks, f.yblocks);
  CHECK(pl.xgroups == f.xgroups && pl.ygroups == f.ygroups, "%u x %u", xs, ys);
  CHECK((int)pl.subsampled == f.subsampled, "%u x %u", xs, ys);
  for (int c = 0; c < 3; c++) CHECK(pl.hshift[c] == f.hshift[c] && pl.vshift[c] == f.vshift[c], "channel %d", c);
  CHECK(pl.cmap_stride == f.cmap_stride, "%u x %u", xs, ys);
  CHECK(pl.plane_stride == f.plane_stride, "%u x %u", xs, ys);
  CHECK(pl.plane_elems == b.plane_elems, "%u x %u", xs, ys);
  CHECK(pl.scrap_off == f.scrap_off, "%u x %u", xs, ys);
  CHECK(pl.ngroups == b.ngroups && pl.nblocks == b.nblocks && pl.ncmap == (b.modular ? pl.ncmap : b.ncmap), "%u x %u", xs, ys);
  CHECK(pl.rows_per_rank == b.rows_per_rank && pl.gather_elems == b.gather_elems, "%u x %u ranks %d", xs, ys, nranks);
  CHECK(pl.planes_n == b.planes && pl.tmp_n == b.tmp, "%u x %u ranks %d", xs, ys, nranks);
  CHECK(pl.lf_n == b.lf_raw && pl.lf_n == b.lf_sm, "%u x %u", xs, ys);
  CHECK(pl.sigma_n == b.sigma && pl.coeffs_n == b.coeffs && pl.raw_quant_n == b.raw_quant, "%u x %u", xs, ys);
  CHECK(pl.map_n == b.transform_map && pl.map_n == b.epf_map, "%u x %u", xs, ys);
  CHECK(pl.cmap_n == b.ytox && pl.cmap_n == b.ytob, "%u x %u", xs, ys);
  CHECK(pl.mod_src_n == b.mod_src, "%u x %u", xs, ys);
  if (!b.modular) {
    CHECK(pl.planes_n == b.place_plane && pl.tmp_n == b.place_tmp && pl.coeffs_n == b.place_coeffs &&
              pl.probe_elems == b.place_probe,
          "%u x %u: the arguments of choose_placement", xs, ys);
  }
  CHECK(same_bits(pl.inv_global_scale, f.inv_global_scale), "global_scale %u", (unsigned)p.global_scale);
  CHECK(same_bits(pl.x_dm, f.x_dm) && same_bits(pl.b_dm, f.b_dm), "qm scales %u %u", (unsigned)p.x_qm_scale,
        (unsigned)p.b_qm_scale);
  CHECK(pl.params_direct_ok == b.params_direct_ok, "biases %g %g %g %g flags %u off %d", p.quant_biases[0],
        p.quant_biases[1], p.quant_biases[2], p.quant_biases[3], fl, (int)off);
  // ---- invariants, in 64-bit arithmetic of their own
  const uint64_t hs = p.hshift[0] | p.hshift[1] | p.hshift[2], vs = p.vshift[0] | p.vshift[1] | p.vshift[2];
  const uint64_t xb = (((uint64_t)p.xsize + (8u << hs) - 1) / (8u << hs)) << hs;
  const uint64_t yb = (((uint64_t)p.ysize + (8u << vs) - 1) / (8u << vs)) << vs;
  const uint64_t stride = (xb * 8 + 63) / 64 * 64, elems = stride * yb * 8;
  const uint64_t xg = ((uint64_t)p.xsize + 255) / 256, yg = ((uint64_t)p.ysize + 255) / 256;
  // every count fits the type FrameDev or the kernels store it in
  CHECK((uint64_t)pl.xblocks == xb && (uint64_t)pl.yblocks == yb && xb * 8 <= INT_MAX && yb * 8 <= INT_MAX, "%u x %u", xs, ys);
  CHECK((uint64_t)pl.xgroups == xg && (uint64_t)pl.ygroups == yg, "%u x %u", xs, ys);
  CHECK(pl.plane_stride == stride && stride <= INT_MAX, "%u x %u", xs, ys);
  CHECK(pl.plane_elems == elems && elems <= (uint64_t)INT_MAX && (uint64_t)pl.scrap_off == elems, "%u x %u", xs, ys);
  CHECK(elems * sizeof(float) <= 0xffffffffull, "%u x %u: 32-bit byte offsets into a plane", xs, ys);
  CHECK(pl.nblocks == xb * yb && pl.nblocks <= (uint64_t)INT_MAX, "%u x %u", xs, ys);
  CHECK(pl.ngroups == xg * yg && pl.ngroups <= (uint64_t)INT_MAX, "%u x %u", xs, ys);
  CHECK(pl.coeffs_n <= (uint64_t)INT_MAX, "%u x %u: 32-bit coefficient indices", xs, ys);
  CHECK(pl.cmap_n <= (uint64_t)INT_MAX, "%u x %u", xs, ys);
  // the frame fits its planes; tmp holds the scrap block row behind it (K1's: a Modular frame has no K1)
  CHECK(pl.planes_n >= elems && pl.tmp_n >= elems, "%u x %u", xs, ys);
  if (!pl.modular) {
    CHECK(pl.tmp_n >= (uint64_t)pl.scrap_off + 8 * stride, "%u x %u: scrap block row", xs, ys);
    CHECK(pl.planes_n >= pl.gather_elems && pl.tmp_n >= pl.gather_elems, "%u x %u ranks %d", xs, ys, nranks);
    CHECK(pl.coeffs_n == pl.ngroups * 3 * 65536, "%u x %u", xs, ys);
    CHECK(pl.probe_elems <= elems && pl.probe_elems % 512 == 0 && elems - pl.probe_elems < 512, "%u x %u", xs, ys);
  }
  // equal counts per rank cover every group row; whole bands hold the frame (so also when nranks divides unevenly)
  CHECK((uint64_t)pl.rows_per_rank * nranks >= yg && ((uint64_t)pl.rows_per_rank - 1) * nranks < yg, "%u ranks %d", ys, nranks);
  CHECK(pl.gather_elems == (uint64_t)nranks * pl.rows_per_rank * 256 * stride, "%u ranks %d", ys, nranks);
  CHECK(pl.gather_elems >= elems, "%u x %u ranks %d", xs, ys, nranks);
  return pl.status;
}

void expect(const jxlh_frame_params& p, int nranks, jxlh_status want, const char* what) {
  const jxlh_status got = check(p, nranks, false);
  CHECK(got == want, "%s: status %d, expected %d", what, (int)got, (int)want);
}

}  // namespace

int main() {
  const int kRanks[4] = {1, 2, 3, 8};
  const uint32_t kSizes[17] = {0,     1,     7,     8,           9,       255,          256,    257,        2047,
                               2048,  2049,  65535, 65536,       65537,   (1u << 20) - 1, 1u << 20, (1u << 20) + 1};
  // ---- sizes x Modular x ranks x 4:4:4 / 4:2:0
  for (uint32_t xs : kSizes)
    for (uint32_t ys : kSizes)
      for (int modular = 0; modular < 2; modular++)
        for (int nranks : kRanks)
          for (int sub = 0; sub < 2; sub++) {
            jxlh_frame_params p = base_params(xs, ys);
            if (modular) p.flags |= JXLH_FRAME_MODULAR;
            if (sub) p.hshift[0] = p.hshift[2] = p.vshift[0] = p.vshift[2] = 1;
            check(p, nranks, false);
          }
  // ---- both sides of each bound
  {
    jxlh_frame_params p = base_params(22016, 32512);  // 86 x 127 = 10 922 groups
    expect(p, 1, JXLH_OK, "22016 x 32512 VarDCT");
    p = base_params(8448, 84736);  // 33 x 331 = 10 923 groups: 10 923 x 196 608 >= 2^31
    expect(p, 1, JXLH_ERR_UNSUPPORTED, "8448 x 84736 VarDCT");
    p.flags |= JXLH_FRAME_MODULAR;  // (no coefficients: the plane bound alone)
    expect(p, 1, JXLH_OK, "8448 x 84736 Modular");
    p = base_params(32768, 32760);
    p.flags |= JXLH_FRAME_MODULAR;
    expect(p, 1, JXLH_OK, "32768 x 32760 Modular");
    p.ysize = 32768;  // plane_elems = 2^30
    expect(p, 1, JXLH_ERR_UNSUPPORTED, "32768 x 32768 Modular");
    p.flags = 0;
    expect(p, 1, JXLH_ERR_UNSUPPORTED, "32768 x 32768 VarDCT");
    for (int nranks : kRanks) {
      check(base_params(22016, 32512), nranks, false);
      check(base_params(8448, 84736), nranks, false);
    }
  }
  // ---- all shift triples over {0, 1, 2, 255}
  {
    const uint32_t kShift[4] = {0, 1, 2, 255};
    const uint32_t kXY[3][2] = {{9, 257}, {2049, 255}, {72, 40}};
    for (int h = 0; h < 64; h++)
      for (int v = 0; v < 64; v++)
        for (const auto& xy : kXY)
          for (int modular = 0; modular < 2; modular++) {
            jxlh_frame_params p = base_params(xy[0], xy[1]);
            if (modular) p.flags |= JXLH_FRAME_MODULAR;
            for (int c = 0; c < 3; c++) {
              p.hshift[c] = kShift[(h >> (2 * c)) & 3];
              p.vshift[c] = kShift[(v >> (2 * c)) & 3];
            }
            const jxlh_status st = check(p, 1, false);
            bool legal = true;
            for (int c = 0; c < 3; c++) legal &= p.hshift[c] <= 1 && p.vshift[c] <= 1;
            CHECK((st == JXLH_OK) == legal, "shifts %d %d", h, v);
          }
  }
  // ---- upsampling
  {
    const uint32_t kUps[7] = {0, 1, 2, 3, 4, 8, 16};
    const uint32_t kXY[3][2] = {{1, 1}, {300, 260}, {1u << 20, 257}};
    for (uint32_t n : kUps)
      for (const auto& xy : kXY)
        for (int i = 0; i < 5; i++)
          for (int j = 0; j < 5; j++) {
            jxlh_frame_params p = base_params(xy[0], xy[1]);
            p.upsampling = n;
            const uint32_t ux[5] = {0, n * xy[0] - n, n * xy[0] - n + 1, n * xy[0], n * xy[0] + 1};
            const uint32_t uy[5] = {0, n * xy[1] - n, n * xy[1] - n + 1, n * xy[1], n * xy[1] + 1};
            p.xsize_upsampled = ux[i];
            p.ysize_upsampled = uy[j];
            const jxlh_status st = check(p, 1, false);
            if (n == 3 || n == 16) CHECK(st == JXLH_ERR_INVALID_ARGUMENT, "upsampling %u", (unsigned)n);
            if (n >= 2 && n <= 8 && n != 3) {
              // 0 = not given; otherwise ceil(size_upsampled / n) must be the coded size
              const bool okx = ux[i] == 0 || i == 2 || i == 3;
              const bool oky = uy[j] == 0 || j == 2 || j == 3;
              CHECK((st == JXLH_OK) == (okx && oky), "upsampling %u sizes %d %d of %u x %u", (unsigned)n, i, j,
                    (unsigned)xy[0], (unsigned)xy[1]);
            }
            if (n <= 1) CHECK(st == JXLH_OK, "upsampling %u ignores the upsampled sizes", (unsigned)n);
          }
  }
  // ---- zero divisors, epf_iters, the ABI version
  {
    jxlh_frame_params p = base_params(72, 40);
    p.global_scale = 0;
    expect(p, 1, JXLH_ERR_INVALID_ARGUMENT, "global_scale 0");
    p = base_params(72, 40);
    p.quant_lf = 0;
    expect(p, 1, JXLH_ERR_INVALID_ARGUMENT, "quant_lf 0");
    p = base_params(72, 40);
    p.color_factor = 0;
    expect(p, 1, JXLH_ERR_INVALID_ARGUMENT, "color_factor 0");
    for (uint32_t it = 0; it <= 4; it++) {
      p = base_params(72, 40);
      p.epf_iters = it;
      expect(p, 1, it <= 3 ? JXLH_OK : JXLH_ERR_INVALID_ARGUMENT, "epf_iters");
    }
    p = base_params(72, 40);
    p.abi_version = JXLH_ABI_VERSION + 1;
    expect(p, 1, JXLH_ERR_INVALID_ARGUMENT, "ABI version");
    p.abi_version = 0;
    expect(p, 1, JXLH_ERR_INVALID_ARGUMENT, "ABI version 0");
    for (uint32_t gs : {1u, 2u, 65536u, 21845u, 0xffffffffu})
      for (uint32_t qm = 0; qm < 8; qm++) {
        p = base_params(72, 40);
        p.global_scale = gs;
        p.x_qm_scale = qm;
        p.b_qm_scale = 7 - qm;
        expect(p, 1, JXLH_OK, "scalars");
      }
  }
  // ---- Modular x epf_sigma_for_modular x ranks
  {
    const float kSigma[4] = {1.0f, 0.0f, -1.0f, std::numeric_limits<float>::quiet_NaN()};
    for (float sigma : kSigma)
      for (int nranks : kRanks)
        for (uint32_t it = 0; it <= 3; it++)
          for (int modular = 0; modular < 2; modular++) {
            jxlh_frame_params p = base_params(264, 264);
            if (modular) p.flags |= JXLH_FRAME_MODULAR;
            p.epf_iters = it;
            p.epf_sigma_for_modular = sigma;
            const jxlh_status st = check(p, nranks, false);
            const jxlh_status want = !modular                      ? JXLH_OK
                                     : (it > 0 && !(sigma > 0.0f)) ? JXLH_ERR_INVALID_ARGUMENT
                                     : nranks > 1                  ? JXLH_ERR_UNSUPPORTED
                                                                   : JXLH_OK;
            CHECK(st == want, "modular %d sigma %g iters %u ranks %d: %d", modular, sigma, (unsigned)it, nranks, (int)st);
          }
  }
  // ---- the parameters' share of se_direct_ok
  {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> bias = {0.9f,  1e-6f, std::nextafterf(1e-6f, 0.0f), std::nextafterf(1e-6f, 1.0f),
                               1e6f,  std::nextafterf(1e6f, 0.0f), std::nextafterf(1e6f, inf), 0.0f, -0.0f, -1.0f,
                               inf,   -inf,  nan};
    std::vector<float> b3 = {0.145f, 0.0f, -4.0f, inf, -inf, nan, 3.0e38f, -3.0e38f, std::nextafterf(3.0e38f, 0.0f),
                             std::nextafterf(4.0f, 0.0f), std::nextafterf(4.0f, 5.0f)};
    for (int i = 2; i < 128; i++) b3.push_back((float)(i * i));  // i - i^2 / i == 0: an entry of the table is zero
    b3.push_back(128.0f * 128.0f);                               // (beyond the table)
    b3.push_back(1.0f);
    int n_ok = 0, n_off = 0;
    for (int which = 0; which < 3; which++)
      for (float v : bias)
        for (uint32_t flags : {0u, (uint32_t)JXLH_FRAME_DENSE_DEQUANT})
          for (int off = 0; off < 2; off++) {
            jxlh_frame_params p = base_params(72, 40);
            p.quant_biases[which] = v;
            p.flags = flags;
            check(p, 1, off != 0);
            const bool ok = jxlh::plan_frame(p, 1, off != 0).params_direct_ok;
            CHECK(ok == (v >= 1e-6f && v <= 1e6f && !flags && !off), "bias[%d] = %g flags %u off %d", which, v,
                  (unsigned)flags, off);
            n_ok += ok;
            n_off += !ok;
          }
    for (float v : b3)
      for (int off = 0; off < 2; off++) {
        jxlh_frame_params p = base_params(72, 40);
        p.quant_biases[3] = v;
        check(p, 1, off != 0);
        const bool ok = jxlh::plan_frame(p, 1, off != 0).params_direct_ok;
        bool zero = false;
        for (int i = 2; i < 128; i++) zero |= v == (float)(i * i);
        const bool finite = v == v && v > -3.0e38f && v < 3.0e38f;
        CHECK(ok == (finite && !zero && !off), "bias[3] = %g off %d", v, off);
      }
    for (float v : {inf, -inf, nan, 3.0e38f, 0.0f, -2.5f})
      for (int which = 0; which < 2; which++) {
        jxlh_frame_params p = base_params(72, 40);
        (which ? p.base_correlation_b : p.base_correlation_x) = v;
        check(p, 1, false);
        CHECK(jxlh::plan_frame(p, 1, false).params_direct_ok == (v == 0.0f || v == -2.5f), "base correlation %g", v);
      }
    CHECK(n_ok > 0 && n_off > 0, "%d %d", n_ok, n_off);
    // a Modular frame: the flag does not reach the checks above
    jxlh_frame_params p = base_params(72, 40);
    p.flags = JXLH_FRAME_MODULAR | JXLH_FRAME_DENSE_DEQUANT;
    expect(p, 1, JXLH_OK, "Modular + dense dequant");
  }
  CHECK(g_ok > 1000 && g_cases - g_ok > 1000, "%ld of %ld accepted", g_ok, g_cases);
  if (g_fail) {
    std::printf("frame plans: %d failures\n", g_fail);
    return 1;
  }
  std::printf("frame plans: ok (%ld cases, %ld accepted)\n", g_cases, g_ok);
  return 0;
}
