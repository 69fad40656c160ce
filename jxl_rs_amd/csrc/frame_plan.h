// What jxlh_frame_begin decides before it touches the context: whether the parameters are acceptable, the frame's
// geometry, the element count of every buffer the begin allocates, and the scalars the reference evaluates on the host
// -- decided here, committed by abi_frame.hip (and abi_modular_frame.hip for a Modular frame).  Plain C++ over the
// public header: the planner is host logic, reads no environment and no context, and is tested without a device
// (tests/cpp/frame_plan.cc).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/jxl_hip.h"
#include "shard_plan.h"  // rows_per_rank: the bands of a sharded frame

namespace jxlh {

constexpr uint32_t kPlanGroupDim = 256;               // pixels per group side (kGroupDim)
constexpr size_t kPlanGroupCoeffs = 3 * 256 * 256;    // coefficients of a group, three channels (3 * kGroupArea)

struct FramePlan {
  jxlh_status status = JXLH_ERR_INVALID_ARGUMENT;  // anything but JXLH_OK: nothing below is meaningful
  bool modular = false;                            // JXLH_FRAME_MODULAR
  // ---- geometry (FrameDev's fields of the same names)
  int xblocks = 0, yblocks = 0, xgroups = 0, ygroups = 0;
  bool subsampled = false;
  int hshift[3] = {0, 0, 0}, vshift[3] = {0, 0, 0};
  int cmap_stride = 0;
  size_t plane_stride = 0;  // floats per pixel row: rows 256-byte aligned
  size_t plane_elems = 0;   // plane_stride * yblocks * 8: below 2^30, the filters address planes by 32-bit BYTE offsets
  int scrap_off = 0;        // plane_elems, where tmp[c]'s scrap block row starts
  size_t ngroups = 0, nblocks = 0, ncmap = 0;
  int rows_per_rank = 0;    // group rows of a rank's band
  size_t gather_elems = 0;  // a sharded frame is all-gathered in place with equal counts per rank: nranks whole bands
  // ---- element counts of the buffers the begin allocates (0: this kind of frame has none)
  size_t planes_n = 0;     // planes[c]
  size_t tmp_n = 0;        // tmp[c]: + one block row, the scrap tile K1 stores the blocks a sub-sampled channel does not hold into
  size_t lf_n = 0;         // lf_raw[c], lf_sm[c]
  size_t sigma_n = 0;
  size_t coeffs_n = 0;     // below 2^31: K1 uses 32-bit coefficient indices
  size_t raw_quant_n = 0;
  size_t map_n = 0;        // transform_map, epf_map
  size_t cmap_n = 0;       // ytox, ytob
  size_t mod_src_n = 0;    // a Modular frame's samples, at the planes' stride
  size_t probe_elems = 0;  // what a placement trial moves through a candidate plane (whole 512-float pieces)
  // ---- scalars, evaluated like the reference does on the host
  float inv_global_scale = 0.f;  // quantizer.rs:79-81
  float x_dm = 0.f, b_dm = 0.f;  // group.rs:395-396
  bool params_direct_ok = false;  // the parameters' share of FrameDev::se_direct_ok
};

// nranks: ranks the frame is sharded over (1 = one GPU).  no_direct_entries: the JXLH_NO_DIRECT_ENTRIES override.
inline FramePlan plan_frame(const jxlh_frame_params& p, int nranks, bool no_direct_entries) {
  FramePlan pl;
  if (p.abi_version != JXLH_ABI_VERSION) return pl;
  if (p.xsize == 0 || p.ysize == 0 || p.xsize > (1u << 20) || p.ysize > (1u << 20) || p.global_scale == 0 ||
      p.quant_lf == 0 || p.color_factor == 0 || p.epf_iters > 3)
    return pl;
  if (p.upsampling > 1 && p.upsampling != 2 && p.upsampling != 4 && p.upsampling != 8) return pl;
  if (p.upsampling > 1) {  // FrameHeader::size() = ceil(size_upsampled / upsampling) (headers/frame_header.rs:555-561)
    const uint32_t n = p.upsampling;
    if (p.xsize_upsampled > p.xsize * n || p.ysize_upsampled > p.ysize * n ||
        (p.xsize_upsampled && (p.xsize_upsampled + n - 1) / n != p.xsize) ||
        (p.ysize_upsampled && (p.ysize_upsampled + n - 1) / n != p.ysize))
      return pl;
  }
  // chroma subsampling (JPEG recompressions): jpeg_upsampling gives shifts of 0 or 1 per axis and channel,
  // relative to the most finely sampled channel (headers/frame_header.rs:252-253, :501-512)
  uint32_t maxhs = 0, maxvs = 0;
  for (int c = 0; c < 3; c++) {
    if (p.hshift[c] > 1 || p.vshift[c] > 1) return pl;
    maxhs |= p.hshift[c];
    maxvs |= p.vshift[c];
  }
  pl.modular = (p.flags & JXLH_FRAME_MODULAR) != 0;
  if (pl.modular) {  // SigmaSource::Constant divides by it (features/epf.rs:81-84); a rank would hold only its band
    if (p.epf_iters > 0 && !(p.epf_sigma_for_modular > 0.0f)) return pl;
    if (nranks > 1) {
      pl.status = JXLH_ERR_UNSUPPORTED;
      return pl;
    }
  }
  // FrameHeader::size_blocks (headers/frame_header.rs:564-569): whole blocks of the coarsest channel
  pl.xblocks = (int)(((p.xsize + (8u << maxhs) - 1) / (8u << maxhs)) << maxhs);
  pl.yblocks = (int)(((p.ysize + (8u << maxvs) - 1) / (8u << maxvs)) << maxvs);
  pl.subsampled = (maxhs | maxvs) != 0;
  for (int c = 0; c < 3; c++) {
    pl.hshift[c] = (int)p.hshift[c];
    pl.vshift[c] = (int)p.vshift[c];
  }
  pl.xgroups = (int)((p.xsize + kPlanGroupDim - 1) / kPlanGroupDim);
  pl.ygroups = (int)((p.ysize + kPlanGroupDim - 1) / kPlanGroupDim);
  pl.cmap_stride = (pl.xblocks + 7) / 8;
  pl.plane_stride = ((size_t)pl.xblocks * 8 + 63) / 64 * 64;
  pl.plane_elems = pl.plane_stride * (size_t)pl.yblocks * 8;
  pl.ngroups = (size_t)pl.xgroups * pl.ygroups;
  pl.rows_per_rank = rows_per_rank(pl.ygroups, nranks);
  pl.gather_elems = (size_t)nranks * pl.rows_per_rank * kPlanGroupDim * pl.plane_stride;
  // (a Modular frame has no coefficients)
  if (pl.plane_elems >= (1ull << 30) || (!pl.modular && pl.ngroups * kPlanGroupCoeffs >= (1ull << 31))) {
    pl.status = JXLH_ERR_UNSUPPORTED;
    return pl;
  }
  pl.scrap_off = (int)pl.plane_elems;
  pl.nblocks = (size_t)pl.xblocks * pl.yblocks;
  pl.ncmap = (size_t)pl.cmap_stride * ((pl.yblocks + 7) / 8);
  pl.sigma_n = pl.nblocks;
  if (pl.modular) {  // no coefficient buffer, LF planes, HF-meta maps or work list; never gathered
    // the samples take the coefficient buffer's place in the budget (12 B/px); rows at the planes' stride: 256-byte
    // aligned, and sample (x, y) of a full-resolution channel sits where pixel (x, y) of its plane will
    pl.planes_n = pl.tmp_n = pl.mod_src_n = pl.plane_elems;
  } else {
    pl.planes_n = std::max(pl.plane_elems, pl.gather_elems);
    pl.tmp_n = std::max(pl.plane_elems + 8 * pl.plane_stride, pl.gather_elems);
    pl.lf_n = pl.raw_quant_n = pl.map_n = pl.nblocks;
    pl.coeffs_n = pl.ngroups * kPlanGroupCoeffs;
    pl.cmap_n = pl.ncmap;
    pl.probe_elems = pl.plane_elems & ~(size_t)511;
  }
  pl.inv_global_scale = (float)(1 << 16) / (float)p.global_scale;
  pl.x_dm = powf(1.0f / 1.25f, (float)p.x_qm_scale - 2.0f);
  pl.b_dm = powf(1.0f / 1.25f, (float)p.b_qm_scale - 2.0f);
  {
    auto fin = [](float v) { return v == v && v > -3.0e38f && v < 3.0e38f; };
    auto bias_ok = [](float v) { return v >= 1e-6f && v <= 1e6f; };
    bool ok = bias_ok(p.quant_biases[0]) && bias_ok(p.quant_biases[1]) && bias_ok(p.quant_biases[2]) &&
              fin(p.quant_biases[3]) && fin(p.base_correlation_x) && fin(p.base_correlation_b) &&
              !(p.flags & JXLH_FRAME_DENSE_DEQUANT);
    // ... and the table adjust_quant_bias is read from must hold no zero (AdjTable::nofast; same IEEE operations here)
    for (int i = 2; i < 128 && ok; i++)
      if ((float)i - p.quant_biases[3] / (float)i == 0.0f) ok = false;
    pl.params_direct_ok = ok && !no_direct_entries;  // (the override: A/B runs of whole suites)
  }
  pl.status = JXLH_OK;
  return pl;
}

}  // namespace jxlh
